// kernels_msm_basis_g2.hip -- one large G2 multi-scalar multiplication over a fixed basis
// (bn_g2_basis_prepare, bn_g2_msm_basis): msm_kernels.h's fixed-basis bodies
// over Fq2 on the pairing path's two-lane layout, one lane pair per element (the table's
// lane halves, MsmIo<bn_g2>, and the pair-uniform control: msm_kernels.h).
// Once per handle:
//   k_g2_basis_build           one lane pair per base: its W(c) entries 2^(c*w) * B and its zero flag
// Per call, between the recoding, histogram, scan and scatter of kernels_msm.hip over the
// zero flags (k_msm_count_basis, k_msm_scatter_basis, k_msm_scan) and k_msm_fold_g2, k_g2_op
// and k_msm_finish_g2 as they are:
//   k_msm_basis_accumulate_g2  one lane pair per (window, bucket) key: mixed additions of its run's entries
//   k_msm_basis_chunk_g2       one lane pair per chunk of a long key's run: the chunk's sum
//   (k_g2_op add)              the buckets of the windows below the top one added row-wise (capi_msm.hip)
//   k_msm_basis_reduce_g2      one lane pair per (segment, one of two windows): its weighted sum
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "fq.h"
#define BN_SPLIT 1
#include "kernels.h"
#include "msm_kernels.h"

namespace bn {

constexpr size_t kL = MsmIo<bn_g2>::kLanes;  // lanes per element in this translation unit

__global__ void __launch_bounds__(kBlock) k_g2_basis_build(const bn_g2* __restrict__ bases, uint32_t nbases, int c,
                                                           bn_fq2* __restrict__ table, uint8_t* __restrict__ zero) {
    fold_table_init();
    msm_basis_build_body<Fq2>(lane_id() / kL, bases, nbases, c, table, zero);
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_accumulate_g2(const bn_fq2* __restrict__ table, uint32_t nbases,
                                                                    uint32_t n, int c,
                                                                    const uint32_t* __restrict__ sorted,
                                                                    const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                                    uint32_t nent, uint32_t L,
                                                                    bn_g2* __restrict__ buckets) {
    fold_table_init();
    msm_basis_accumulate_body<Fq2>(lane_id() / kL, table, nbases, n, c, sorted, offsets, nkeys, nent, L, buckets);
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_chunk_g2(const bn_fq2* __restrict__ table, uint32_t nbases,
                                                               uint32_t n, int c, const uint32_t* __restrict__ sorted,
                                                               const uint32_t* __restrict__ offsets,
                                                               const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                               uint32_t nent, uint32_t L, bn_g2* __restrict__ sums,
                                                               uint32_t nslots) {
    fold_table_init();
    msm_basis_chunk_body<Fq2>(lane_id() / kL, table, nbases, n, c, sorted, offsets, longinfo, nkeys, nent, L, sums,
                              nslots);
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_reduce_g2(const bn_g2* __restrict__ buckets, int c, uint32_t nkeys,
                                                                uint32_t nseg, bn_g2* __restrict__ parts) {
    fold_table_init();
    msm_basis_reduce_body<Fq2>(lane_id() / kL, buckets, c, nkeys, nseg, parts);
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_basis_g2)
