// kernels_msm_g2.hip -- the group-law kernels of the G2 multi-scalar multiplication
// (bn_g2_msm; the phases are kernels_msm.hip's): msm_kernels.h's bodies over Fq2 on the
// pairing path's two-lane layout, one lane pair per element (the pair-uniform control:
// msm_kernels.h).
//   k_msm_accumulate_g2  one lane pair per (window, bucket) key (short keys)
//   k_msm_chunk_g2       one lane pair per chunk of a long key's run (msm.h)
//   k_msm_fold_g2        one lane pair per group of partial sums of a long key, once per level
//   k_msm_reduce_g2      one lane pair per (segment, window)
//   k_msm_horner_g2      one lane pair: Horner over the window sums
//   k_msm_finish_g2      one lane pair: the returned image
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "fq.h"
#define BN_SPLIT 1
#include "kernels.h"
#include "msm_kernels.h"

namespace bn {

constexpr size_t kL = MsmIo<bn_g2>::kLanes;  // lanes per element in this translation unit

// Occupancy: the kernels carry no waves-per-SIMD attribute.  The accumulation waits on
// a 192-byte gather per addition and would take more waves, but the general jac_add
// over Fq2 needs 194 registers without scratch (two waves per SIMD); held to three
// waves (168 registers) it spills 116 bytes per lane and to four (128) 256 bytes, and
// spills cost the two-lane kernels 20-40 % (kernels.h BN_PATH_ATTR), so it stays at the
// compiler's own two waves with no scratch.
__global__ void __launch_bounds__(kBlock) k_msm_accumulate_g2(const bn_g2* __restrict__ p, size_t n,
                                                              const uint32_t* __restrict__ sorted,
                                                              const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                              uint32_t nent, uint32_t L, bn_g2* __restrict__ buckets) {
    fold_table_init();
    msm_accumulate_body<Fq2>(lane_id() / kL, p, n, sorted, offsets, nkeys, nent, L, buckets);
}
__global__ void __launch_bounds__(kBlock) k_msm_chunk_g2(const bn_g2* __restrict__ p, size_t n,
                                                         const uint32_t* __restrict__ sorted,
                                                         const uint32_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                         uint32_t nent, uint32_t L, bn_g2* __restrict__ sums,
                                                         uint32_t nslots) {
    fold_table_init();
    msm_chunk_body<Fq2>(lane_id() / kL, p, n, sorted, offsets, longinfo, nkeys, nent, L, sums, nslots);
}
__global__ void __launch_bounds__(kBlock) k_msm_fold_g2(const bn_g2* __restrict__ src, uint32_t nsrc,
                                                        const uint32_t* __restrict__ offsets,
                                                        const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                        uint32_t nent, uint32_t L, int level, bn_g2* __restrict__ dst,
                                                        uint32_t ndst, uint32_t nslots, bn_g2* __restrict__ buckets) {
    fold_table_init();
    msm_fold_body<Fq2>(lane_id() / kL, src, nsrc, offsets, longinfo, nkeys, nent, L, level, dst, ndst, nslots, buckets);
}
__global__ void __launch_bounds__(kBlock) k_msm_reduce_g2(const bn_g2* __restrict__ buckets, int c, uint32_t nkeys,
                                                          uint32_t nseg, bn_g2* __restrict__ parts) {
    fold_table_init();
    msm_reduce_body<Fq2>(lane_id() / kL, buckets, c, nkeys, nseg, parts);
}
__global__ void __launch_bounds__(64) k_msm_horner_g2(const bn_g2* __restrict__ win, int c, int finish,
                                                      bn_g2* __restrict__ out) {
    fold_table_init();
    msm_horner_body<Fq2>(lane_id() / kL, win, c, finish, out);
}
__global__ void __launch_bounds__(64) k_msm_finish_g2(const bn_g2* in, bn_g2* out) {
    fold_table_init();
    msm_finish_body<Fq2>(lane_id() / kL, in, out);
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_g2)
