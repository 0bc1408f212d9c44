// kernels_msm_g2.hip -- the group-law kernels of the G2 multi-scalar multiplication
// (bn_g2_msm; the phases are kernels_msm.hip's, the bodies msm_group.h's) on the
// pairing path's two-lane layout (fq2_split.h): lanes 2j and 2j + 1
// hold coordinates c0 and c1 of the points of element j.
//   k_msm_accumulate_g2  one lane pair per (window, bucket) key (short keys)
//   k_msm_chunk_g2       one lane pair per chunk of a long key's run (msm.h)
//   k_msm_fold_g2        one lane pair per group of partial sums of a long key, once per level
//   k_msm_reduce_g2      one lane pair per (segment, window)
//   k_msm_horner_g2      one lane pair: Horner over the window sums
//   k_msm_finish_g2      one lane pair: the returned image
// Pair-uniform control: every Fq2 product and zero test reads the partner lane over
// DPP, so both lanes of a pair must take every branch and leave every loop
// together.  The element is lane_id() / kL and every bound (the key against nkeys,
// the run clamped to nent, an entry's index against n) is computed from values the
// two lanes share; the block size is even, so a grid always covers whole pairs.
// Pairs of one wave walk runs of different lengths: the wave-uniform guards of
// jac_add (BN_ANY) see the active lanes only.  Every computed index is bounded
// against its array in the kernel; a lane pair whose index is out of range does
// nothing, and no block waits for another.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "fq.h"
#define BN_SPLIT 1
#include "kernels.h"
#include "msm_group.h"

namespace bn {

constexpr size_t kL = kPathLanes;  // lanes per element in this translation unit

// this lane's coordinates of a point's reference image
__device__ __forceinline__ G2J ld_g2(const bn_g2& a) {
    return {widen<kPt>(ld_ref2(a.x)), widen<kPt>(ld_ref2(a.y)), widen<kPt>(ld_ref2(a.z))};
}
__device__ __forceinline__ void st_g2(bn_g2& o, const G2J& r) {
    st_ref2(o.x, r.x);
    st_ref2(o.y, r.y);
    st_ref2(o.z, r.z);
}

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
    const size_t key = lane_id() / kL;
    if (key >= nkeys) return;
    uint32_t hi = offsets[key + 1];
    hi = hi < nent ? hi : nent;
    uint32_t lo = offsets[key];
    lo = lo < hi ? lo : hi;
    if (hi - lo > L) return;  // a long key: k_msm_chunk_g2 / k_msm_fold_g2 write its bucket
    const G2J acc = msm_bucket_sum<Fq2>([&](uint32_t idx) { return ld_g2(p[idx]); }, n, sorted, lo, hi);
    st_g2(buckets[key], acc);
}

// The overlong runs (msm.h; the G1 kernels are kernels_msm.hip's k_msm_chunk / k_msm_fold).
// Both lanes of a pair derive the slot, and from it the key, the chunk or group and every
// bound, from lane_id() / kL and the same loads, so they take every branch together.
__global__ void __launch_bounds__(kBlock) k_msm_chunk_g2(const bn_g2* __restrict__ p, size_t n,
                                                         const uint32_t* __restrict__ sorted,
                                                         const uint32_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                         uint32_t nent, uint32_t L, bn_g2* __restrict__ sums,
                                                         uint32_t nslots) {
    fold_table_init();
    const size_t t = lane_id() / kL;
    if (t >= nslots) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, 0, (uint32_t)t);
    if (!task.some) return;
    const G2J acc = msm_bucket_sum<Fq2>([&](uint32_t idx) { return ld_g2(p[idx]); }, n, sorted, task.lo, task.hi);
    st_g2(sums[t], acc);
}
__global__ void __launch_bounds__(kBlock) k_msm_fold_g2(const bn_g2* __restrict__ src, uint32_t nsrc,
                                                        const uint32_t* __restrict__ offsets,
                                                        const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                        uint32_t nent, uint32_t L, int level, bn_g2* __restrict__ dst,
                                                        uint32_t ndst, uint32_t nslots, bn_g2* __restrict__ buckets) {
    fold_table_init();
    const size_t t = lane_id() / kL;
    if (t >= nslots) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, level, (uint32_t)t);
    if (!task.some || task.hi > nsrc || (!task.last && t >= ndst)) return;
    const G2J acc = msm_fold_sum<Fq2>([&](uint32_t i) { return ld_g2(src[i]); }, task.lo, task.hi);
    st_g2(task.last ? buckets[task.key] : dst[t], acc);
}

// parts[s * nwin + w], so that the addition tree over the segments is k_g2_op on
// contiguous halves
__global__ void __launch_bounds__(kBlock) k_msm_reduce_g2(const bn_g2* __restrict__ buckets, int c, uint32_t nkeys,
                                                          uint32_t nseg, bn_g2* __restrict__ parts) {
    fold_table_init();
    const size_t t = lane_id() / kL;
    const uint32_t nwin = (uint32_t)msm_windows(c);
    if (t >= (size_t)nseg * nwin) return;
    const uint32_t s = (uint32_t)(t / nwin), w = (uint32_t)(t % nwin);
    st_g2(parts[t], msm_segment_sum<Fq2>([&](uint32_t key) { return ld_g2(buckets[key]); }, c, nkeys, s, w));
}

// finish != 0: the normalized image; 0: the Jacobian partial sum as it stands (a
// multi-device context adds the partials first)
__global__ void __launch_bounds__(64) k_msm_horner_g2(const bn_g2* __restrict__ win, int c, int finish,
                                                      bn_g2* __restrict__ out) {
    fold_table_init();
    if (lane_id() >= kL) return;
    G2J acc = msm_horner_sum<Fq2>([&](int w) { return ld_g2(win[w]); }, c);
    if (finish) acc = msm_finish_point(acc);
    st_g2(*out, acc);
}
// *out = the returned image of *in; in == nullptr: of zero (n == 0)
__global__ void __launch_bounds__(64) k_msm_finish_g2(const bn_g2* in, bn_g2* out) {
    fold_table_init();
    if (lane_id() >= kL) return;
    G2J a = jac_zero<Fq2>();
    if (in) a = ld_g2(*in);
    st_g2(*out, msm_finish_point(a));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_g2)
