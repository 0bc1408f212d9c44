// kernels_msm.hip -- G1 multi-scalar multiplication by the bucket method:
// S = sum_i k[i] * P[i], normalized (and the recoding, histogram and scatter of the
// G2 one, whose group-law kernels are kernels_msm_g2.hip, and of the fixed-basis one of
// kernels_msm_basis.hip).  The recoding and the scan are defined here; the group-law
// kernels instantiate msm_kernels.h's bodies over Fq, one lane per element.  The phases
// pass data only across kernel boundaries on one stream (no block waits for another):
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
#include "msm_kernels.h"
#include "msm_sort.h"

namespace bn {

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

// ---------------------------------------------------------------- the group-law phases
// msm_kernels.h's bodies over Fq, one lane per element
__global__ void __launch_bounds__(kBlock) k_msm_accumulate(const bn_g1* __restrict__ p, size_t n,
                                                           const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                           uint32_t nent, uint32_t L, bn_g1* __restrict__ buckets) {
    fold_table_init();
    msm_accumulate_body<Fq>(lane_id(), p, n, sorted, offsets, nkeys, nent, L, buckets);
}
__global__ void __launch_bounds__(kBlock) k_msm_chunk(const bn_g1* __restrict__ p, size_t n,
                                                      const uint32_t* __restrict__ sorted,
                                                      const uint32_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                      uint32_t nent, uint32_t L, bn_g1* __restrict__ sums,
                                                      uint32_t nslots) {
    fold_table_init();
    msm_chunk_body<Fq>(lane_id(), p, n, sorted, offsets, longinfo, nkeys, nent, L, sums, nslots);
}
__global__ void __launch_bounds__(kBlock) k_msm_fold(const bn_g1* __restrict__ src, uint32_t nsrc,
                                                     const uint32_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                     uint32_t nent, uint32_t L, int level, bn_g1* __restrict__ dst,
                                                     uint32_t ndst, uint32_t nslots, bn_g1* __restrict__ buckets) {
    fold_table_init();
    msm_fold_body<Fq>(lane_id(), src, nsrc, offsets, longinfo, nkeys, nent, L, level, dst, ndst, nslots, buckets);
}
__global__ void __launch_bounds__(kBlock) k_msm_reduce(const bn_g1* __restrict__ buckets, int c, uint32_t nkeys,
                                                       uint32_t nseg, bn_g1* __restrict__ parts) {
    fold_table_init();
    msm_reduce_body<Fq>(lane_id(), buckets, c, nkeys, nseg, parts);
}
__global__ void __launch_bounds__(64) k_msm_horner(const bn_g1* __restrict__ win, int c, int finish,
                                                   bn_g1* __restrict__ out) {
    fold_table_init();
    msm_horner_body<Fq>(lane_id(), win, c, finish, out);
}
__global__ void __launch_bounds__(64) k_msm_finish(const bn_g1* in, bn_g1* out) {
    fold_table_init();
    msm_finish_body<Fq>(lane_id(), in, out);
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm)
