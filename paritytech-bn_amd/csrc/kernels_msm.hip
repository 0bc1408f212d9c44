// kernels_msm.hip -- G1 multi-scalar multiplication by the bucket method:
// S = sum_i k[i] * P[i], normalized (and the recoding, histogram and scatter of the
// G2 one, whose group-law kernels are kernels_msm_g2.hip, and of the fixed-basis one of
// kernels_msm_basis.hip; the group-law bodies of both are msm_group.h's).  The phases pass data only across kernel boundaries on one
// stream (no block waits for another):
//   k_msm_count       signed-digit recoding (msm.h), histogram of the (window, bucket) keys
//   k_msm_scan        exclusive scan of the histogram -> bucket offsets and scatter cursors,
//                     and the list of the long keys (runs above the run cap, msm.h)
//   k_msm_scatter     recoding again, each entry (term index, sign) to its bucket's run
//   k_msm_accumulate  one lane per bucket: gathers its run's points and adds them (short keys)
//   k_msm_chunk       one lane per chunk of a long key's run: the chunk's sum
//   k_msm_fold        one lane per group of up to kMsmFoldFan partial sums of a long key, once
//                     per level of the tree; a key's last group writes its bucket
//   k_msm_reduce      one lane per segment of kMsmSegment buckets: sum_j (j + 1) * B_j
//   (k_g1_op add)     addition tree over each window's segments (capi_msm.hip)
//   k_msm_horner      one lane: Horner over the window sums, then normalize
// Every computed index is bounded against its array in the kernel; a lane whose
// index is out of range does nothing.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "kernels.h"
#include "msm_group.h"
#include "msm_sort.h"

namespace bn {

__device__ __forceinline__ G1J ld_g1(const bn_g1& a) {
    return {widen<kPt>(ld_ref(a.x)), widen<kPt>(ld_ref(a.y)), widen<kPt>(ld_ref(a.z))};
}
__device__ __forceinline__ void st_g1(bn_g1& o, const G1J& r) {
    st_ref(o.x, r.x);
    st_ref(o.y, r.y);
    st_ref(o.z, r.z);
}

// ---------------------------------------------------------------- recoding, histogram, scatter
// One lane per term.  kScatter = false counts the keys; true claims a position in
// each key's run (an atomic cursor: the order inside a bucket is not fixed, the
// bucket's sum and so the normalized result do not depend on it).  Zero digits and
// zero points produce no entry.  All it reads of a point is whether z is zero.
__device__ __forceinline__ bool msm_point_is_zero(const bn_g1& a) { return F_is_zero(ld_ref(a.z)); }
__device__ __forceinline__ bool msm_point_is_zero(const bn_g2& a) { return F_is_zero(ld_ref2(a.z)); }
// a fixed basis (msm_basis.h) keeps one zero flag per base in place of the points
__device__ __forceinline__ bool msm_point_is_zero(const uint8_t& flag) { return flag != 0; }
// (the wave-aggregated claim of a position in a key's run, msm_claim: msm_sort.h)
template <bool kScatter, class P>
__device__ __forceinline__ void msm_digits(const P* __restrict__ p, const bn_fr* __restrict__ k, size_t n, int c,
                                           uint32_t nkeys, uint32_t* __restrict__ counts,
                                           const uint32_t* __restrict__ offsets, uint32_t* __restrict__ sorted,
                                           uint32_t nent) {
    fold_table_init();
    const size_t i = lane_id();
    if (i >= n) return;
    if (msm_point_is_zero(p[i])) return;
    uint32_t s[8];
    fr_to_canonical(k[i], s);
    uint32_t carry = 0;
    const int nw = msm_windows(c);
    for (int w = 0; w < nw; ++w) {  // the same trip count on every lane: msm_claim's ballots see the whole wave
        const int32_t d = msm_signed_digit(msm_raw_window(s, c, w), c, &carry);
        const uint32_t key = d != 0 ? msm_key(c, w, d, (uint32_t)i) : nkeys;
        const bool has = key < nkeys;
        const uint32_t pos = msm_claim(counts, key, has);  // counts = the cursors when scattering
        if constexpr (kScatter) {
            if (has && pos < offsets[key + 1] && pos < nent) sorted[pos] = msm_entry((uint32_t)i, d);
        }
    }
}
__global__ void __launch_bounds__(kBlock) k_msm_count(const bn_g1* __restrict__ p, const bn_fr* __restrict__ k, size_t n,
                                                      int c, uint32_t nkeys, uint32_t* __restrict__ counts) {
    msm_digits<false>(p, k, n, c, nkeys, counts, nullptr, nullptr, 0);
}
__global__ void __launch_bounds__(kBlock) k_msm_scatter(const bn_g1* __restrict__ p, const bn_fr* __restrict__ k,
                                                        size_t n, int c, uint32_t nkeys, uint32_t* __restrict__ cursors,
                                                        const uint32_t* __restrict__ offsets,
                                                        uint32_t* __restrict__ sorted, uint32_t nent) {
    msm_digits<true>(p, k, n, c, nkeys, cursors, offsets, sorted, nent);
}
__global__ void __launch_bounds__(kBlock) k_msm_count_g2(const bn_g2* __restrict__ p, const bn_fr* __restrict__ k,
                                                         size_t n, int c, uint32_t nkeys,
                                                         uint32_t* __restrict__ counts) {
    msm_digits<false>(p, k, n, c, nkeys, counts, nullptr, nullptr, 0);
}
__global__ void __launch_bounds__(kBlock) k_msm_scatter_g2(const bn_g2* __restrict__ p, const bn_fr* __restrict__ k,
                                                           size_t n, int c, uint32_t nkeys,
                                                           uint32_t* __restrict__ cursors,
                                                           const uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ sorted, uint32_t nent) {
    msm_digits<true>(p, k, n, c, nkeys, cursors, offsets, sorted, nent);
}
// the same over the first n bases of a fixed basis (bn_g1_msm_basis; kernels_msm_basis.hip)
__global__ void __launch_bounds__(kBlock) k_msm_count_basis(const uint8_t* __restrict__ zero, const bn_fr* __restrict__ k,
                                                            size_t n, int c, uint32_t nkeys,
                                                            uint32_t* __restrict__ counts) {
    msm_digits<false>(zero, k, n, c, nkeys, counts, nullptr, nullptr, 0);
}
__global__ void __launch_bounds__(kBlock) k_msm_scatter_basis(const uint8_t* __restrict__ zero,
                                                              const bn_fr* __restrict__ k, size_t n, int c,
                                                              uint32_t nkeys, uint32_t* __restrict__ cursors,
                                                              const uint32_t* __restrict__ offsets,
                                                              uint32_t* __restrict__ sorted, uint32_t nent) {
    msm_digits<true>(zero, k, n, c, nkeys, cursors, offsets, sorted, nent);
}

// offsets[0 .. nkeys] = exclusive scan of counts[0 .. nkeys), cursors[key] = offsets[key];
// longinfo[0] = the number of keys with more than L entries, longinfo[1 ..] those keys in
// key order (at most nkeys; none at L = kMsmRunUnsplit).  One block (msm_sort.h msm_scan_block).
__global__ void __launch_bounds__(kMsmScanBlock) k_msm_scan(const uint32_t* __restrict__ counts, uint32_t nkeys,
                                                            uint32_t* __restrict__ offsets,
                                                            uint32_t* __restrict__ cursors, uint32_t L,
                                                            uint32_t* __restrict__ longinfo) {
    msm_scan_block(counts, nkeys, offsets, cursors, L, longinfo);
}

// ---------------------------------------------------------------- bucket accumulation
// One lane per (window, bucket): the sum of its run of sorted entries
// (msm_group.h msm_bucket_sum).  An empty bucket is zero.  A run of more than L entries is
// left to k_msm_chunk / k_msm_fold, which write its bucket.
__global__ void __launch_bounds__(kBlock) k_msm_accumulate(const bn_g1* __restrict__ p, size_t n,
                                                           const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                           uint32_t nent, uint32_t L, bn_g1* __restrict__ buckets) {
    fold_table_init();
    const size_t key = lane_id();
    if (key >= nkeys) return;
    uint32_t hi = offsets[key + 1];
    hi = hi < nent ? hi : nent;
    uint32_t lo = offsets[key];
    lo = lo < hi ? lo : hi;
    if (hi - lo > L) return;
    const G1J acc = msm_bucket_sum<Fq>([&](uint32_t idx) { return ld_g1(p[idx]); }, n, sorted, lo, hi);
    st_g1(buckets[key], acc);
}

// ---------------------------------------------------------------- overlong runs (msm.h)
// One lane per level-0 slot: the sum of one chunk of at most L entries of a long key's run
// (msm_run_task finds the key and the chunk from the slot).  A slot no key holds does
// nothing; with no long key every lane returns after one load.
__global__ void __launch_bounds__(kBlock) k_msm_chunk(const bn_g1* __restrict__ p, size_t n,
                                                      const uint32_t* __restrict__ sorted,
                                                      const uint32_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                      uint32_t nent, uint32_t L, bn_g1* __restrict__ sums,
                                                      uint32_t nslots) {
    fold_table_init();
    const size_t t = lane_id();
    if (t >= nslots) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, 0, (uint32_t)t);
    if (!task.some) return;
    const G1J acc = msm_bucket_sum<Fq>([&](uint32_t idx) { return ld_g1(p[idx]); }, n, sorted, task.lo, task.hi);
    st_g1(sums[t], acc);
}
// One lane per slot of fold level `level` >= 1: the sum of up to kMsmFoldFan consecutive
// partial sums of one long key at the level below (src[0 .. nsrc)), into the key's bucket
// when it is the key's only group, else into dst[slot] (dst[0 .. ndst)).
__global__ void __launch_bounds__(kBlock) k_msm_fold(const bn_g1* __restrict__ src, uint32_t nsrc,
                                                     const uint32_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                     uint32_t nent, uint32_t L, int level, bn_g1* __restrict__ dst,
                                                     uint32_t ndst, uint32_t nslots, bn_g1* __restrict__ buckets) {
    fold_table_init();
    const size_t t = lane_id();
    if (t >= nslots) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, level, (uint32_t)t);
    if (!task.some || task.hi > nsrc || (!task.last && t >= ndst)) return;
    const G1J acc = msm_fold_sum<Fq>([&](uint32_t i) { return ld_g1(src[i]); }, task.lo, task.hi);
    st_g1(task.last ? buckets[task.key] : dst[t], acc);
}

// ---------------------------------------------------------------- bucket reduction
// One lane per (segment, window): the segment's weighted sum (msm_group.h
// msm_segment_sum).  parts[s * nwin + w], so that the addition tree over the
// segments is k_g1_op on contiguous halves.
__global__ void __launch_bounds__(kBlock) k_msm_reduce(const bn_g1* __restrict__ buckets, int c, uint32_t nkeys,
                                                       uint32_t nseg, bn_g1* __restrict__ parts) {
    fold_table_init();
    const size_t t = lane_id();
    const uint32_t nwin = (uint32_t)msm_windows(c);
    if (t >= (size_t)nseg * nwin) return;
    const uint32_t s = (uint32_t)(t / nwin), w = (uint32_t)(t % nwin);
    st_g1(parts[t], msm_segment_sum<Fq>([&](uint32_t key) { return ld_g1(buckets[key]); }, c, nkeys, s, w));
}

// ---------------------------------------------------------------- window combination
// One lane: Horner over the window sums win[0 .. nwin) (msm_group.h msm_horner_sum).
// finish != 0: the normalized image (msm_finish_point); 0: the Jacobian partial sum
// as it stands (a multi-device context adds the partials first).
__global__ void __launch_bounds__(64) k_msm_horner(const bn_g1* __restrict__ win, int c, int finish,
                                                   bn_g1* __restrict__ out) {
    fold_table_init();
    if (lane_id() != 0) return;
    G1J acc = msm_horner_sum<Fq>([&](int w) { return ld_g1(win[w]); }, c);
    if (finish) acc = msm_finish_point(acc);
    st_g1(*out, acc);
}
// *out = the returned image of *in (msm_finish_point); in == nullptr: of zero (n == 0)
__global__ void __launch_bounds__(64) k_msm_finish(const bn_g1* in, bn_g1* out) {
    fold_table_init();
    if (lane_id() != 0) return;
    G1J a = jac_zero<Fq>();
    if (in) a = ld_g1(*in);
    st_g1(*out, msm_finish_point(a));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm)
