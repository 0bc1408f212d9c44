// msm_fixed.h -- multi-scalar multiplications over PREPARED bases (bn_g1_prepared,
// bn_g1_msm_prepared_many): the bodies shared by kernels_msm_fixed.hip and
// the host build of tests/native/msm_fixed_emul.cpp, templates over the field F through
// curve.h's F_* (Fq: G1; a G2 instance can follow) that take functors for every load and
// store.
//
// The scalars are recoded exactly as for the bucket method (msm.h: W(c) signed digits of c
// bits).  The table holds, for every base b and window w, the affine points
//     entry (b, w, j) = (j + 1) * 2^(c*w) * bases[b],   j < 2^(c-1),
// at index ((b * W(c) + w) << (c - 1)) + j, so that
//     sum_b k_b * bases[b] = sum_b sum_w sign(d_bw) * entry(b, w, |d_bw| - 1)
// is a sum of table entries with no doubling.  The top window is stored like the others
// (its digits never exceed 2^t, msm.h msm_top_bits: the entries above are never read).  A
// base with z == 0 has a zero flag and all-zero entries, which are never added.
#pragma once
#include "msm_group.h"

namespace bn {

// The window width bn_g1_bases_prepare takes for c = 0: the fastest width of the measured
// sweep over 4 .. 10 (profiles/msm_prepared_sweep.jsonl) at every shape, 832 KiB
// of table per base.  Wider tables are faster still, as 1 / W(c), at twice the memory and
// the prepare time per bit (profiles/msm_prepared_sweep_wide.jsonl): the caller's choice.
constexpr int kMsmFixedWindow = 10;
// entry indices are 32-bit
constexpr uint64_t kMsmFixedMaxEntries = 0x7fffffffull;
// the most lanes per output of the lookup kernel (a power of two)
constexpr uint32_t kMsmFixedMaxLanes = 64;

// entries of the table of k bases at width c (0: the default); 0 for a k or c that the
// prepare call refuses
BN_INLINE uint64_t msm_fixed_entries(uint64_t k, int c) {
    if (c == 0) c = kMsmFixedWindow;
    if (k < 1 || !msm_window_ok(c)) return 0;
    const uint64_t per_base = (uint64_t)msm_windows(c) << (c - 1);
    if (k > kMsmFixedMaxEntries / per_base) return 0;
    return k * per_base;
}
// index of entry (b, w, mag - 1), mag = |digit| >= 1
BN_INLINE uint32_t msm_fixed_index(int c, uint32_t nwin, uint32_t b, uint32_t w, uint32_t mag) {
    return ((b * nwin + w) << (c - 1)) + (mag - 1u);
}
BN_INLINE bool msm_fixed_lanes_ok(int lanes) {
    return lanes >= 1 && lanes <= (int)kMsmFixedMaxLanes && (lanes & (lanes - 1)) == 0;
}
// Lanes per output when none is forced, read off the sweep (profiles/msm_prepared_sweep.jsonl,
// tools/msm_prepared_bench.py): the smallest power of two that gives the
// card 2^17 lanes (two waves on every SIMD), or 2^19 from 832 (base, window) pairs per
// output on (the geometric mean of the 416 and 1,664 pairs of k = 16 and k = 64 at c = 10,
// between which the fastest setting moves); at most kMsmFixedMaxLanes, and at most a
// quarter of the pairs, so that a lane keeps four lookups beside its share of the tree.
BN_INLINE uint32_t msm_fixed_auto_lanes(uint64_t m, uint64_t k, int c) {
    const uint64_t pairs = k * (uint64_t)msm_windows(c);
    const uint64_t target = pairs < 832 ? (1u << 17) : (1u << 19);
    uint32_t lanes = 1;
    while (lanes < kMsmFixedMaxLanes && m * lanes < target && 8ull * lanes <= pairs) lanes *= 2;
    return lanes;
}

// One lane of the table build: the 2^(c-1) entries of (base, window w), entry j stored
// normalized by store(first + j, x, y) where first + j < nent.  c * w doublings, then
// the running multiples by mixed additions of the window's own affine point (the first
// of them meets the doubling shortcut).  The base is not zero.
template <template <int> class F, class Store>
BN_INLINE void msm_fixed_build(const Jac<F>& base, int c, int w, uint32_t first, uint32_t nent, Store&& store) {
    Jac<F> p = base;
    for (int i = 0; i < c * w; ++i) p = jac_double(p);
    p = jac_normalize(p);
    Jac<F> acc = p;
    const uint32_t n = msm_buckets(c);
    for (uint32_t j = 0; j < n; ++j) {
        if (j) acc = jac_add_mixed(acc, p.x, p.y);
        const Jac<F> a = jac_normalize(acc);
        if (first + j < nent) store(first + j, a.x, a.y);
    }
}

// acc + (the entry, negated when neg) where on, else acc; decode(e, x, y) turns a fetched
// entry into its coordinates
template <template <int> class F, class Raw, class Decode>
BN_INLINE Jac<F> msm_fixed_add(const Jac<F>& acc, const Raw& e, bool neg, bool on, Decode&& decode) {
    F<2> x, y;
    decode(e, x, y);
    const F<2> ny = F_widen<2>(F_neg(y));
    const Jac<F> t = jac_add_mixed(acc, x, F_select(neg, ny, y));
    return jac_select(on, t, acc);
}

// The partial sum of lane l of L of one output.  The k * W(c) (base, window) pairs, base
// major, are cut into L contiguous runs of ceil(k * W / L), so every pair belongs to
// exactly one lane for every L >= 1.  scalar(b, s) writes the canonical words of the
// output's scalar for base b (recoded whole: the carry chain is integer-only), zero(b) is
// the base's zero flag, fetch(idx) loads entry idx < nent.  Every index of a lane follows
// from its scalars alone, so the next entry is fetched before the current one is added;
// a pair that contributes nothing (digit 0, zero base, index out of range) fetches entry 0
// and adds nothing.  Lanes of a wave that share l step through the same pairs together.
template <template <int> class F, class Scalar, class Zero, class Fetch, class Decode>
BN_INLINE Jac<F> msm_fixed_lane_sum(Scalar&& scalar, Zero&& zero, Fetch&& fetch, Decode&& decode, uint32_t k, int c,
                                    uint32_t nent, uint32_t l, uint32_t L) {
    const uint32_t nwin = (uint32_t)msm_windows(c);
    const uint64_t pairs = (uint64_t)k * nwin;
    const uint64_t per = (pairs + L - 1) / L;
    const uint64_t lo = (uint64_t)l * per < pairs ? (uint64_t)l * per : pairs;
    const uint64_t hi = lo + per < pairs ? lo + per : pairs;
    uint32_t b = (uint32_t)(lo / nwin), w = (uint32_t)(lo % nwin);
    Jac<F> acc = jac_zero<F>();
    uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t carry = 0;
    bool fresh = true, bzero = true, pending = false, pneg = false;
    auto cur = fetch(0u);
    for (uint64_t i = lo; i < lo + per; ++i) {
        const bool valid = i < hi;
        if (valid && fresh) {
            scalar(b, s);
            bzero = zero(b);
            carry = 0;
            for (uint32_t v = 0; v < w; ++v) (void)msm_signed_digit(msm_raw_window(s, c, (int)v), c, &carry);
            fresh = false;
        }
        const int32_t d = msm_signed_digit(msm_raw_window(s, c, (int)w), c, &carry);
        const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
        uint32_t idx = msm_fixed_index(c, nwin, b, w, mag ? mag : 1u);
        const bool take = valid && d != 0 && !bzero && idx < nent;
        idx = take ? idx : 0u;
        const auto next = fetch(idx);
        if (BN_ANY(pending)) acc = msm_fixed_add(acc, cur, pneg, pending, decode);
        cur = next;
        pending = take;
        pneg = d < 0;
        if (++w == nwin) {
            w = 0;
            ++b;
            fresh = true;
        }
    }
    if (BN_ANY(pending)) acc = msm_fixed_add(acc, cur, pneg, pending, decode);
    return acc;
}

}  // namespace bn
