// kernels_msm.hip -- G1 multi-scalar multiplication by the bucket method:
// S = sum_i k[i] * P[i], normalized.  The phases pass data only across kernel
// boundaries on one stream (no block waits for another):
//   k_msm_count       signed-digit recoding (msm.h), histogram of the (window, bucket) keys
//   k_msm_scan        exclusive scan of the histogram -> bucket offsets and scatter cursors
//   k_msm_scatter     recoding again, each entry (term index, sign) to its bucket's run
//   k_msm_accumulate  one lane per bucket: gathers its run's points and adds them
//   k_msm_reduce      one lane per segment of kMsmSegment buckets: sum_j (j + 1) * B_j
//   (k_g1_op add)     addition tree over each window's segments (capi.hip)
//   k_msm_horner      one lane: Horner over the window sums, then normalize
// Every computed index is bounded against its array in the kernel; a lane whose
// index is out of range does nothing.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "kernels.h"

namespace bn {

__device__ __forceinline__ G1J ld_g1(const bn_g1& a) {
    return {widen<kPt>(ld_ref(a.x)), widen<kPt>(ld_ref(a.y)), widen<kPt>(ld_ref(a.z))};
}
__device__ __forceinline__ void st_g1(bn_g1& o, const G1J& r) {
    st_ref(o.x, r.x);
    st_ref(o.y, r.y);
    st_ref(o.z, r.z);
}
__device__ __forceinline__ G1J g1_select(bool c, const G1J& a, const G1J& b) {
    return {F_select(c, a.x, b.x), F_select(c, a.y, b.y), F_select(c, a.z, b.z)};
}
// the returned image: normalize(), and G1::zero() = (0, one, 0) for any zero point
__device__ __forceinline__ G1J msm_finish(const G1J& a) {
    const G1J r = jac_normalize(a);
    return g1_select(jac_is_zero(a), jac_zero<Fq>(), r);
}

// ---------------------------------------------------------------- recoding, histogram, scatter
// One lane per term.  kScatter = false counts the keys; true claims a position in
// each key's run (an atomic cursor: the order inside a bucket is not fixed, the
// bucket's sum and so the normalized result do not depend on it).  Zero digits and
// zero points produce no entry.
template <bool kScatter>
__device__ __forceinline__ void msm_digits(const bn_g1* __restrict__ p, const bn_fr* __restrict__ k, size_t n, int c,
                                           uint32_t nkeys, uint32_t* __restrict__ counts,
                                           const uint32_t* __restrict__ offsets, uint32_t* __restrict__ sorted,
                                           uint32_t nent) {
    fold_table_init();
    const size_t i = lane_id();
    if (i >= n) return;
    if (F_is_zero(ld_ref(p[i].z))) return;
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
// One lane per (window, bucket): walks its run of sorted entries, gathers the point,
// applies the digit's sign and adds.  jac_add is the general one: its zero
// short-cuts and doubling branch make duplicates and P + (-P) in a bucket come out
// right.  An empty bucket is zero.
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
    G1J acc = jac_zero<Fq>();
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t ent = sorted[e];
        const uint32_t idx = msm_entry_index(ent);
        if (idx >= n) continue;
        G1J pt = ld_g1(p[idx]);
        const G1J ng = jac_neg(pt);
        pt = g1_select(msm_entry_neg(ent), ng, pt);
        acc = jac_add(acc, pt);
    }
    st_g1(buckets[key], acc);
}

// ---------------------------------------------------------------- bucket reduction
// One lane per (segment, window).  Segment s of a window holds the buckets
// j0 .. j0 + len - 1 (j0 = s * kMsmSegment); bucket b weighs (b >> rs) + 1, rs the
// window's replica shift (msm.h: 0 except in the top window).  Running sums from the
// top give S = sum B_b and, adding S into T at every b that is a multiple of 2^rs,
// T = sum (weight(b) - ceil(j0 / 2^rs)) * B_b; the lane returns T + ceil(j0 / 2^rs) * S,
// the product by a (c - 1)-bit double-and-add.  parts[s * nwin + w], so that the
// addition tree over the segments is k_g1_op on contiguous halves.
__global__ void __launch_bounds__(kBlock) k_msm_reduce(const bn_g1* __restrict__ buckets, int c, uint32_t nkeys,
                                                       uint32_t nseg, bn_g1* __restrict__ parts) {
    fold_table_init();
    const size_t t = lane_id();
    const uint32_t nwin = (uint32_t)msm_windows(c);
    if (t >= (size_t)nseg * nwin) return;
    const uint32_t s = (uint32_t)(t / nwin), w = (uint32_t)(t % nwin);
    const uint32_t nb = msm_buckets(c);
    const int rs = msm_replica_shift(c, (int)w);
    const uint32_t rmask = (1u << rs) - 1u;
    const uint32_t j0 = s * kMsmSegment;
    const uint32_t len = j0 >= nb ? 0u : (nb - j0 < kMsmSegment ? nb - j0 : kMsmSegment);
    G1J sum = jac_zero<Fq>(), wsum = jac_zero<Fq>();
    for (uint32_t j = len; j-- > 0;) {
        const uint32_t key = w * nb + j0 + j;
        if (key >= nkeys) continue;
        sum = jac_add(sum, ld_g1(buckets[key]));
        const G1J a = jac_add(wsum, sum);
        wsum = g1_select(((j0 + j) & rmask) == 0, a, wsum);
    }
    const uint32_t base = (j0 + rmask) >> rs;  // ceil(j0 / 2^rs) < 2^(c-1)
    G1J m = jac_zero<Fq>();                    // base * sum
    for (int b = c - 2; b >= 0; --b) {
        m = jac_double(m);
        const G1J a = jac_add(m, sum);
        m = g1_select(((base >> b) & 1u) != 0, a, m);
    }
    st_g1(parts[t], jac_add(wsum, m));
}

// ---------------------------------------------------------------- window combination
// One lane: Horner over the window sums win[0 .. nwin) (c doublings and one addition
// per window).  finish != 0: the normalized image (msm_finish); 0: the Jacobian
// partial sum as it stands (a multi-device context adds the partials first).
__global__ void __launch_bounds__(64) k_msm_horner(const bn_g1* __restrict__ win, int c, int finish,
                                                   bn_g1* __restrict__ out) {
    fold_table_init();
    if (lane_id() != 0) return;
    const int nwin = msm_windows(c);
    G1J acc = ld_g1(win[nwin - 1]);
    for (int w = nwin - 2; w >= 0; --w) {
        for (int b = 0; b < c; ++b) acc = jac_double(acc);
        acc = jac_add(acc, ld_g1(win[w]));
    }
    if (finish) acc = msm_finish(acc);
    st_g1(*out, acc);
}
// *out = the returned image of *in (msm_finish); in == nullptr: of zero (n == 0)
__global__ void __launch_bounds__(64) k_msm_finish(const bn_g1* in, bn_g1* out) {
    fold_table_init();
    if (lane_id() != 0) return;
    G1J a = jac_zero<Fq>();
    if (in) a = ld_g1(*in);
    st_g1(*out, msm_finish(a));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm)
