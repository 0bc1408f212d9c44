// kernels_msm_basis.hip -- one large G1 multi-scalar multiplication over a fixed basis
// (bn_g1_basis_prepare, bn_g1_msm_basis): msm_kernels.h's fixed-basis bodies
// over Fq, one lane per element.
// Once per handle:
//   k_g1_basis_build         one lane per base: its W(c) entries 2^(c*w) * B and its zero flag
// Per call, between the recoding, histogram, scan and scatter of kernels_msm.hip (with the
// zero flags in place of the points) and k_msm_fold, k_g1_op and k_msm_finish as they are:
//   k_msm_basis_accumulate   one lane per (window, bucket) key: mixed additions of its run's entries
//   k_msm_basis_chunk        one lane per chunk of a long key's run: the chunk's sum
//   (k_g1_op add)            the buckets of the windows below the top one added row-wise (capi_msm.hip)
//   k_msm_basis_reduce       one lane per (segment, one of two windows): its weighted sum
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "kernels.h"
#include "msm_kernels.h"

namespace bn {

__global__ void __launch_bounds__(kBlock) k_g1_basis_build(const bn_g1* __restrict__ bases, uint32_t nbases, int c,
                                                           bn_fq* __restrict__ table, uint8_t* __restrict__ zero) {
    fold_table_init();
    msm_basis_build_body<Fq>(lane_id(), bases, nbases, c, table, zero);
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_accumulate(const bn_fq* __restrict__ table, uint32_t nbases,
                                                                 uint32_t n, int c, const uint32_t* __restrict__ sorted,
                                                                 const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                                 uint32_t nent, uint32_t L, bn_g1* __restrict__ buckets) {
    fold_table_init();
    msm_basis_accumulate_body<Fq>(lane_id(), table, nbases, n, c, sorted, offsets, nkeys, nent, L, buckets);
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_chunk(const bn_fq* __restrict__ table, uint32_t nbases, uint32_t n,
                                                            int c, const uint32_t* __restrict__ sorted,
                                                            const uint32_t* __restrict__ offsets,
                                                            const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                            uint32_t nent, uint32_t L, bn_g1* __restrict__ sums,
                                                            uint32_t nslots) {
    fold_table_init();
    msm_basis_chunk_body<Fq>(lane_id(), table, nbases, n, c, sorted, offsets, longinfo, nkeys, nent, L, sums, nslots);
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_reduce(const bn_g1* __restrict__ buckets, int c, uint32_t nkeys,
                                                             uint32_t nseg, bn_g1* __restrict__ parts) {
    fold_table_init();
    msm_basis_reduce_body<Fq>(lane_id(), buckets, c, nkeys, nseg, parts);
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_basis)
