// msm_many.h -- many small multi-scalar multiplications over FRESH bases in one launch set
// (bn_g1_msm_many): the bodies shared by kernels_msm_many.hip and the host
// build of tests/native/msm_many_emul.cpp, templates over the field F through curve.h's F_*
// (Fq: G1) that take functors for every load and store.
//
// Straus with shared doublings over msm.h's signed c-bit recoding.  Every term t of a
// launch set gets its W(c) digits, one byte each at digits[w * nt + t] (window major: the
// lanes of a wave read neighbouring bytes), and its 2^(c-1) Jacobian multiples
//     entry (t, j) = (j + 1) * P_t   at index (t << (c - 1)) + j.
// A unit is a contiguous run of at most 64 terms of one segment; its lane walks the windows
// from the top down, doubling its accumulator c times per window and adding, for every term
// of the unit, the entry of the term's digit with the digit's sign.  A segment's sum is the
// sum of its units' partials.
#pragma once
#include "msm_group.h"

namespace bn {

// A digit of the recoding lies in [-(2^(c-1) - 1), 2^(c-1)], so at c = 8 it is one of the
// 256 values -127 .. 128: the byte of 128 is that of -128, which never occurs.
BN_INLINE uint8_t msm_many_digit_byte(int32_t d) { return (uint8_t)(d & 0xff); }
BN_INLINE int32_t msm_many_digit(uint8_t b) {
    const int32_t d = (int32_t)(int8_t)b;
    return d == -128 ? 128 : d;
}
BN_INLINE bool msm_many_window_ok(int c) { return c >= 2 && c <= 8; }
// table entries and digit bytes of a launch set of nt terms
BN_INLINE uint64_t msm_many_entries(uint64_t nt, int c) { return nt << (c - 1); }
BN_INLINE uint64_t msm_many_digits(uint64_t nt, int c) { return nt * (uint64_t)msm_windows(c); }

// One lane of the table kernel: term t < nt of the set.  s = the canonical scalar's words.
// digit(i, byte) stores byte i < ndig, entry(i, point) stores entry i < nent.  A zero point
// (z == 0) gets all-zero digits, so its entries (written as zero points: every entry holds
// field elements) are never added.  The multiples are P, 2 P by jac_double, then the running
// sum + P by the general addition with P's z powers computed once.
template <template <int> class F, class Digit, class Entry>
BN_INLINE void msm_many_term(const Jac<F>& p, const uint32_t s[8], int c, uint32_t t, uint32_t nt, uint64_t ndig,
                             uint64_t nent, Digit&& digit, Entry&& entry) {
    const bool pzero = jac_is_zero(p);
    const uint32_t nwin = (uint32_t)msm_windows(c);
    uint32_t carry = 0;
    for (uint32_t w = 0; w < nwin; ++w) {
        const int32_t d = msm_signed_digit(msm_raw_window(s, c, (int)w), c, &carry);
        const uint64_t i = (uint64_t)w * nt + t;
        if (i < ndig) digit(i, pzero ? (uint8_t)0 : msm_many_digit_byte(d));
    }
    const uint32_t n = msm_buckets(c);
    const uint64_t first = (uint64_t)t << (c - 1);
    if (BN_ANY(pzero)) {
        if (pzero) {
            for (uint32_t j = 0; j < n; ++j)
                if (first + j < nent) entry(first + j, jac_zero<F>());
            return;
        }
    }
    const auto z2 = narrow<kPt>(F_sqr(p.z));
    const auto z3 = narrow<kPt>(F_mul(p.z, z2));
    Jac<F> acc = p;
    for (uint32_t j = 0; j < n; ++j) {
        if (j == 1) acc = jac_double(p);
        if (j > 1) acc = jac_add_pre(acc, p, false, z2, z3);
        if (first + j < nent) entry(first + j, acc);
    }
}

// acc + (the entry, negated when neg) where on, else acc.  The general jac_add: its zero
// shortcuts and doubling branch are what make equal terms, and P with -P, in one unit come
// out right.
template <template <int> class F>
BN_INLINE Jac<F> msm_many_add(const Jac<F>& acc, const Jac<F>& e, bool neg, bool on) {
    const Jac<F> ng = jac_neg(e);
    const Jac<F> t = jac_add(acc, jac_select(neg, ng, e));
    return jac_select(on, t, acc);
}

// The partial sum of one unit: the terms t0 .. t0 + cnt - 1 of the set (cnt <= 64).
// digit(i) loads byte i < ndig, fetch(i) loads entry i < nent as it is stored, decode turns
// a fetched entry into a point.  Every index follows from the digit bytes alone, so the next
// entry is fetched before the current one is added; a zero digit fetches the term's first
// entry and adds nothing.  The pending addition of a window is made before the doublings
// that open the next one.
template <template <int> class F, class Digit, class Fetch, class Decode>
BN_INLINE Jac<F> msm_many_unit_sum(Digit&& digit, Fetch&& fetch, Decode&& decode, int c, uint32_t t0, uint32_t cnt,
                                   uint32_t nt, uint64_t ndig, uint64_t nent) {
    const uint32_t nwin = (uint32_t)msm_windows(c);
    Jac<F> acc = jac_zero<F>();
    bool pending = false, pneg = false;
    auto cur = fetch((uint64_t)0);
    for (uint32_t w = nwin; w-- > 0;) {
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t t = t0 + i;
            const uint64_t di = (uint64_t)w * nt + t;
            const int32_t d = di < ndig ? msm_many_digit(digit(di)) : 0;
            const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
            uint64_t idx = ((uint64_t)t << (c - 1)) + (mag ? mag - 1u : 0u);
            const bool take = d != 0 && idx < nent;
            idx = idx < nent ? idx : 0;
            const auto next = fetch(idx);
            if (BN_ANY(pending)) acc = msm_many_add(acc, decode(cur), pneg, pending);
            if (i == 0 && w != nwin - 1)
                for (int b = 0; b < c; ++b) acc = jac_double(acc);
            cur = next;
            pending = take;
            pneg = d < 0;
        }
    }
    if (BN_ANY(pending)) acc = msm_many_add(acc, decode(cur), pneg, pending);
    return acc;
}

// The returned image of one segment: the sum of its units' partials part(u0 .. u1), at most
// 64 of them; none gives the zero image.
template <template <int> class F, class Load>
BN_INLINE Jac<F> msm_many_segment(Load&& part, uint32_t u0, uint32_t u1) {
    Jac<F> acc = jac_zero<F>();
    for (uint32_t u = u0; u < u1; ++u) acc = jac_add(acc, part(u));
    return msm_finish_point(acc);
}

}  // namespace bn
