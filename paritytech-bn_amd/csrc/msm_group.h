// msm_group.h -- the group-law bodies of the bucket multi-scalar multiplication,
// templates over the field F (Fq: G1, Fq2: G2) that take a functor loading a point
// by index: the sum of one bucket's run of sorted entries, the weighted sum of one
// segment of a window's buckets, Horner over the window sums, and the returned
// image.  msm_kernels.h wraps them for both groups, G2 on the two-lane layout (fq2_split.h: every
// argument must then hold the same value on both lanes of a pair, so that both
// take every branch and leave every loop together); tests/native/msm_g2_emul.cpp
// compiles them for the host with g++ alone.
#pragma once
#include "curve.h"
#include "msm.h"

namespace bn {

template <template <int> class F>
BN_INLINE Jac<F> jac_select(bool c, const Jac<F>& a, const Jac<F>& b) {
    return {F_select(c, a.x, b.x), F_select(c, a.y, b.y), F_select(c, a.z, b.z)};
}
// the returned image: normalize(), and zero() = (0, one, 0) for any zero point
template <template <int> class F>
BN_INLINE Jac<F> msm_finish_point(const Jac<F>& a) {
    const Jac<F> r = jac_normalize(a);
    return jac_select(jac_is_zero(a), jac_zero<F>(), r);
}

// The sum of one (window, bucket) key's run sorted[lo .. hi): each entry's point
// (point(index), index < n) with the digit's sign applied.  jac_add is the general
// one: its zero short-cuts and doubling branch make duplicates and P + (-P) in a
// bucket come out right.  An empty run is zero.
template <template <int> class F, class Load>
BN_INLINE Jac<F> msm_bucket_sum(Load&& point, size_t n, const uint32_t* sorted, uint32_t lo, uint32_t hi) {
    Jac<F> acc = jac_zero<F>();
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t ent = sorted[e];
        const uint32_t idx = msm_entry_index(ent);
        if (idx >= n) continue;
        Jac<F> pt = point(idx);
        const Jac<F> ng = jac_neg(pt);
        pt = jac_select(msm_entry_neg(ent), ng, pt);
        acc = jac_add(acc, pt);
    }
    return acc;
}

// An overlong run (msm.h: more than the run cap's entries) is summed in pieces: each chunk
// sorted[lo .. hi) of at most L entries by msm_bucket_sum itself, then the chunk sums by a
// tree of msm_fold_sum over at most kFan consecutive partial sums part(lo .. hi).  The
// pieces are the same points in another bracketing, so the bucket's point is the same and
// the normalized result the same bytes; jac_add's doubling branch and zero short-cuts
// cover equal and cancelling partial sums.
template <template <int> class F, uint32_t kFan = kMsmFoldFan, class Load>
BN_INLINE Jac<F> msm_fold_sum(Load&& part, uint32_t lo, uint32_t hi) {
    hi = hi < lo ? lo : (hi - lo > kFan ? lo + kFan : hi);
    Jac<F> acc = jac_zero<F>();
    for (uint32_t i = lo; i < hi; ++i) acc = jac_add(acc, part(i));
    return acc;
}

// Segment s of window w holds the buckets j0 .. j0 + len - 1 (j0 = s * kMsmSegment);
// bucket b weighs (b >> rs) + 1, rs the window's replica shift (msm.h: 0 except in
// the top window).  Running sums from the top give S = sum B_b and, adding S into T
// at every b that is a multiple of 2^rs, T = sum (weight(b) - ceil(j0 / 2^rs)) * B_b;
// the result is T + ceil(j0 / 2^rs) * S, the product by a (c - 1)-bit double-and-add.
// bucket(key) loads the sum of key < nkeys.
template <template <int> class F, class Load>
BN_INLINE Jac<F> msm_segment_sum(Load&& bucket, int c, uint32_t nkeys, uint32_t s, uint32_t w) {
    const uint32_t nb = msm_buckets(c);
    const int rs = msm_replica_shift(c, (int)w);
    const uint32_t rmask = (1u << rs) - 1u;
    const uint32_t j0 = s * kMsmSegment;
    const uint32_t len = j0 >= nb ? 0u : (nb - j0 < kMsmSegment ? nb - j0 : kMsmSegment);
    Jac<F> sum = jac_zero<F>(), wsum = jac_zero<F>();
    for (uint32_t j = len; j-- > 0;) {
        const uint32_t key = w * nb + j0 + j;
        if (key >= nkeys) continue;
        sum = jac_add(sum, bucket(key));
        const Jac<F> a = jac_add(wsum, sum);
        wsum = jac_select(((j0 + j) & rmask) == 0, a, wsum);
    }
    const uint32_t base = (j0 + rmask) >> rs;  // ceil(j0 / 2^rs) < 2^(c-1)
    Jac<F> m = jac_zero<F>();                  // base * sum
    for (int b = c - 2; b >= 0; --b) {
        m = jac_double(m);
        const Jac<F> a = jac_add(m, sum);
        m = jac_select(((base >> b) & 1u) != 0, a, m);
    }
    return jac_add(wsum, m);
}

// Horner over the window sums win(0 .. W(c)): c doublings and one addition per window
template <template <int> class F, class Load>
BN_INLINE Jac<F> msm_horner_sum(Load&& win, int c) {
    const int nwin = msm_windows(c);
    Jac<F> acc = win(nwin - 1);
    for (int w = nwin - 2; w >= 0; --w) {
        for (int b = 0; b < c; ++b) acc = jac_double(acc);
        acc = jac_add(acc, win(w));
    }
    return acc;
}

}  // namespace bn
