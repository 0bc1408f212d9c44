// kernels_msm.hip -- G1 multi-scalar multiplication by the bucket method:
// S = sum_i k[i] * P[i], normalized (and the recoding, histogram and scatter of the
// G2 one, whose group-law kernels are kernels_msm_g2.hip; the group-law bodies of both
// are msm_group.h's).  The phases pass data only across kernel boundaries on one
// stream (no block waits for another):
//   k_msm_count       signed-digit recoding (msm.h), histogram of the (window, bucket) keys
//   k_msm_scan        exclusive scan of the histogram -> bucket offsets and scatter cursors
//   k_msm_scatter     recoding again, each entry (term index, sign) to its bucket's run
//   k_msm_accumulate  one lane per bucket: gathers its run's points and adds them
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
    for (int w = 0; w < nw; ++w) {
        const int32_t d = msm_signed_digit(msm_raw_window(s, c, w), c, &carry);
        if (d == 0) continue;
        const uint32_t key = msm_key(c, w, d, (uint32_t)i);
        if (key >= nkeys) continue;
        if constexpr (!kScatter) {
            atomicAdd(&counts[key], 1u);
        } else {
            const uint32_t pos = atomicAdd(&counts[key], 1u);  // counts = the cursors here
            if (pos < offsets[key + 1] && pos < nent) sorted[pos] = msm_entry((uint32_t)i, d);
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

// offsets[0 .. nkeys] = exclusive scan of counts[0 .. nkeys), cursors[key] = offsets[key].
// One block: each thread scans a contiguous piece, the piece totals go through LDS.
__global__ void __launch_bounds__(kMsmScanBlock) k_msm_scan(const uint32_t* __restrict__ counts, uint32_t nkeys,
                                                            uint32_t* __restrict__ offsets,
                                                            uint32_t* __restrict__ cursors) {
    __shared__ uint32_t tot[kMsmScanBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nkeys + kMsmScanBlock - 1) / kMsmScanBlock;
    const uint32_t lo = t * per < nkeys ? t * per : nkeys;
    const uint32_t hi = lo + per < nkeys ? lo + per : nkeys;
    uint32_t sum = 0;
    for (uint32_t j = lo; j < hi; ++j) sum += counts[j];
    tot[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < kMsmScanBlock; d <<= 1) {  // inclusive scan of the piece totals
        const uint32_t v = t >= d ? tot[t - d] : 0u;
        __syncthreads();
        tot[t] += v;
        __syncthreads();
    }
    uint32_t run = tot[t] - sum;
    for (uint32_t j = lo; j < hi; ++j) {
        offsets[j] = run;
        cursors[j] = run;
        run += counts[j];
    }
    if (t == kMsmScanBlock - 1) offsets[nkeys] = tot[t];
}

// ---------------------------------------------------------------- bucket accumulation
// One lane per (window, bucket): the sum of its run of sorted entries
// (msm_group.h msm_bucket_sum).  An empty bucket is zero.
__global__ void __launch_bounds__(kBlock) k_msm_accumulate(const bn_g1* __restrict__ p, size_t n,
                                                           const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                           uint32_t nent, bn_g1* __restrict__ buckets) {
    fold_table_init();
    const size_t key = lane_id();
    if (key >= nkeys) return;
    uint32_t hi = offsets[key + 1];
    hi = hi < nent ? hi : nent;
    uint32_t lo = offsets[key];
    lo = lo < hi ? lo : hi;
    const G1J acc = msm_bucket_sum<Fq>([&](uint32_t idx) { return ld_g1(p[idx]); }, n, sorted, lo, hi);
    st_g1(buckets[key], acc);
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
