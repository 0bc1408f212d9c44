// pairing.h -- optimal-ate pairing pieces, one lane per pairing.
//
// Replaces src/groups/mod.rs:579-727 (G2 precomputation, Miller loop) and
// src/fields/fq12.rs:62-124, 249-266 (final exponentiation, exp_by_neg_z).
#pragma once
#include "curve.h"

namespace bn {

// storage bound of the Miller accumulator and of the final-exponentiation temporaries
constexpr int kF = 2;
template <int S, int B>
BN_INLINE Fq12<S> narrow12(const Fq12<B>& a) {
    if constexpr (kv(B) <= S) {
        return widen<S>(fq12_norm(a));
    } else {
        return widen<S>(fq12_fold(a));
    }
}

// ---------------------------------------------------------------- G2 precomputation
// AffineG2::precompute, mod.rs:701-727.  `emit(k, ell)` receives line k (0..86).
// `coeff`: the doubling step's curve constant (curve.h doubling_coeff(), or its
// per-pairing multiple from scaled_inputs below)
template <int B, int CB, typename Emit>
BN_INLINE void g2_precompute(const G2Aff<B>& q, const Fq2<CB>& coeff, Emit&& emit) {
    G2Proj r = {widen<kPt>(q.x), widen<kPt>(q.y), widen<kPt>(fq2_one())};
    const G2Base<B> qb = g2_base(q);
    int k = 0;
#pragma unroll 1
    for (int i = 0; i < BN_NAF_DIGITS; ++i) {
        emit(k++, doubling_step(r, coeff));
        if ((kNafNonzero >> i) & 1u) {  // uniform across the wave
            emit(k++, mixed_addition_step(r, g2_base_signed(qb, (kNafMinus >> i) & 1u)));
        }
    }
    G2Aff<kPt> q1 = mul_by_q(q);
    G2Aff<kPt> q2 = mul_by_q(q1);
    q2.y = fq2_neg(q2.y);
    emit(k++, mixed_addition_step(r, g2_base(q1)));
    emit(k++, mixed_addition_step(r, g2_base(q2)));
}
template <int B, typename Emit>
BN_INLINE void g2_precompute(const G2Aff<B>& q, Emit&& emit) {
    g2_precompute(q, doubling_coeff(), static_cast<Emit&&>(emit));
}

#if BN_SPLIT
// The same product f * (x0 + x4 w^3 + x2 w^4) on the two-lane layout, as six
// column sums reduced once each.  In the w-basis (f_m = coefficient of w^m:
// c0.c(m/2) for even m, c1.c((m-1)/2) for odd m; w^6 = xi)
//   out_m = f_m x0 + f_(m-3) x4 + f_(m-4) x2,  indices mod 6, times xi on a wrap,
// with xi moved onto the f side (xi f_2 .. xi f_5).  Each lane sums its
// coordinate of three Fq2 products -- six digit products, own(u) * v0 +
// partner(u) * (lane 0: K*p - v1, lane 1: v1) -- in one column sum (tower.h fq_dot6)
// and reduces once: 36 products + 6 reductions per lane instead of the 13-product
// formula's 26 + 13, and no combining adds, subtractions or folds.  The line
// side's operand forms are built once per coefficient.  The value is the
// reference's product (fq12.rs:130-196) -- the same residues.
using LineOps = LineOpsT<kLine, kLine + 1>;
template <int X>
BN_INLINE LineOps line_ops(const Fq2<X>& v_in) {
    const auto o = line_ops_of(v_in);
    return {widen<kLine>(o.y), widen<kLine + 1>(o.w)};
}
template <int F, int X>
BN_INLINE Fq12<2> fq12_mul_by_024_lazy(const Fq12<F>& f_in, const Fq2<X>& x0_in, const Fq2<X>& x4_in,
                                       const Fq2<X>& x2_in) {
    static_assert(kl(F) == 1 && kv(F) <= 2, "fq12_mul_by_024_lazy: f normalized, bound 2");
    const LineOps x0 = line_ops(x0_in), x4 = line_ops(x4_in), x2 = line_ops(x2_in);
    const Fq<2> f0 = widen<2>(f_in.c0.c0.c), f1 = widen<2>(f_in.c1.c0.c), f2 = widen<2>(f_in.c0.c1.c);
    const Fq<2> f3 = widen<2>(f_in.c1.c1.c), f4 = widen<2>(f_in.c0.c2.c), f5 = widen<2>(f_in.c1.c2.c);
    auto xi = [](const Fq<2>& u) { return fq2_fold(fq2_mul_xi(Fq2<2>{u})).c; };
    // value per lane <= 3 * (2p * 4p + 2p * 5p) = 54 p^2: the reduction is below 1.4 p
    auto out = [&](const Fq<2>& a, const LineOps& va, const Fq<2>& b, const LineOps& vb, const Fq<2>& c,
                   const LineOps& vc) {
        // this call's contract: f side below 2 p, y <= kLine p, w <= (kLine + 1) p; the
        // value per lane stays <= 54 p^2 and the reduction below 1.4 p (fq_dot6 asserts it)
        return Fq2<2>{fq_dot6(a, va, b, vb, c, vc)};
    };
    // outputs last-first, each xi*f_k made just before its first use: under the default
    // scheduler 0.7 % faster than first-first with the four xi*f_k up front
    // (k_pairing_fused 4.31 vs 4.34 ms, config 5 2.65 vs 2.70 ms, profiles/r2ax_ab_line_order.txt)
    const Fq2<2> o5 = out(f5, x0, f2, x4, f1, x2);
    const Fq2<2> o4 = out(f4, x0, f1, x4, f0, x2);
    const Fq<2> g5 = xi(f5);
    const Fq2<2> o3 = out(f3, x0, f0, x4, g5, x2);
    const Fq<2> g4 = xi(f4);
    const Fq2<2> o2 = out(f2, x0, g5, x4, g4, x2);
    const Fq<2> g3 = xi(f3);
    const Fq2<2> o1 = out(f1, x0, g4, x4, g3, x2);
    const Fq<2> g2 = xi(f2);
    const Fq2<2> o0 = out(f0, x0, g3, x4, g2, x2);
    return {{o0, o2, o4}, {o1, o3, o5}};
}
#endif

// f <- f * line(P): ell_vw.scale(Py), ell_vv.scale(Px)  (mod.rs:589)
template <int B, int PB>
BN_INLINE Fq12<kF> apply_line(const Fq12<B>& f, const Ell& c, const Fq<PB>& px, const Fq<PB>& py) {
#if BN_SPLIT
    return widen<kF>(fq12_mul_by_024_lazy(narrow12<2>(f), c.ell_0, narrow<kLine>(fq2_scale(c.ell_vw, py)),
                                          narrow<kLine>(fq2_scale(c.ell_vv, px))));
#else
    return narrow12<kF>(fq12_mul_by_024(f, c.ell_0, narrow<kLine>(fq2_scale(c.ell_vw, py)),
                                        narrow<kLine>(fq2_scale(c.ell_vv, px))));
#endif
}

// the same with the line already scaled by P (e.ell_vw = ell_vw * Py, e.ell_vv = ell_vv * Px:
// what the producers store, lines_wide.h PwEll)
template <int B>
BN_INLINE Fq12<kF> apply_line_scaled(const Fq12<B>& f, const Ell& e) {
#if BN_SPLIT
    return widen<kF>(fq12_mul_by_024_lazy(narrow12<2>(f), e.ell_0, e.ell_vw, e.ell_vv));
#else
    return narrow12<kF>(fq12_mul_by_024(f, e.ell_0, e.ell_vw, e.ell_vv));
#endif
}
BN_INLINE Fq12<kF> line_from_one_scaled(const Ell& e) {
    const Fq2<kF> z = widen<kF>(fq2_zero());
    return {{narrow<kF>(e.ell_0), z, narrow<kF>(e.ell_vv)}, {z, narrow<kF>(e.ell_vw), z}};
}

// The first step of a loop (or segment) that starts from f = one: one^2 * line
// is the line itself, x0 + x4 w^3 + x2 w^4 (w^3 = c1.c1, w^4 = c0.c2; the
// operands of apply_line), so the squaring and the sparse product are skipped
// (k_miller_seg at one pairing, 16 segments: 194 -> 177 us).  The same residues
// as fq12.rs mul_by_024 applied to Fq12::one().
template <int PB>
BN_INLINE Fq12<kF> line_from_one(const Ell& c, const Fq<PB>& px, const Fq<PB>& py) {
    const Fq2<kF> z = widen<kF>(fq2_zero());
    return {{narrow<kF>(c.ell_0), z, narrow<kF>(fq2_scale(c.ell_vv, px))},
            {z, narrow<kF>(fq2_scale(c.ell_vw, py)), z}};
}
// f^2 * line, or the line alone on the first step from f = one (wave-uniform `first`)
template <int PB>
BN_INLINE Fq12<kF> sqr_line(const Fq12<kF>& f, bool first, const Ell& c, const Fq<PB>& px, const Fq<PB>& py) {
    if (first) return line_from_one(c, px, py);
    return apply_line(narrow12<kF>(fq12_sqr(f)), c, px, py);
}

// G2Precomp::miller_loop, mod.rs:579-607.  `line(k)` returns coefficient k.
template <int PB, typename Line>
BN_INLINE Fq12<kF> miller_loop(const Fq<PB>& px, const Fq<PB>& py, Line&& line) {
    Fq12<kF> f = widen<kF>(fq12_one());
    int idx = 0;
#pragma unroll 1
    for (int i = 0; i < BN_NAF_DIGITS; ++i) {
        f = sqr_line(f, i == 0, line(idx++), px, py);
        if ((kNafNonzero >> i) & 1u) f = apply_line(f, line(idx++), px, py);
    }
    f = apply_line(f, line(idx++), px, py);
    f = apply_line(f, line(idx), px, py);
    return f;
}
// the same over lines already scaled by P (apply_line_scaled)
template <typename Line>
BN_INLINE Fq12<kF> miller_loop_scaled(Line&& line) {
    Fq12<kF> f = widen<kF>(fq12_one());
    int idx = 0;
#pragma unroll 1
    for (int i = 0; i < BN_NAF_DIGITS; ++i) {
        const Ell e = line(idx++);
        f = i == 0 ? line_from_one_scaled(e) : apply_line_scaled(narrow12<kF>(fq12_sqr(f)), e);
        if ((kNafNonzero >> i) & 1u) f = apply_line_scaled(f, line(idx++));
    }
    f = apply_line_scaled(f, line(idx++));
    f = apply_line_scaled(f, line(idx));
    return f;
}

// The shared-squaring loop of ONE product of pairs (mod.rs:609-640) over lines already
// scaled by P: all 64 digits and the two closing lines from f = one, per digit one
// squaring of the accumulator and then the line of each pair (kernels_pairing.hip
// k_miller_products; compiled for the host by tests/native/products_emul.cpp).
// `line(t, k)` returns line k (0 .. 86) of pair t < K.  K is the number of pairs the loop
// runs over, which may exceed the product's own: the callable then returns the line one
// (ell_0 = 1, ell_vw = ell_vv = 0) for the pairs past it, and for a pair with a zero
// point -- the sparse product by it is f itself, so the value is that of the live pairs
// alone, and one when there is none (K == 0 included).  The first line goes through
// line_from_one_scaled whichever it is (the line one gives one).
// `step(pos)` runs at every digit (pos = digit * 256) and line (+ 1 + pass * 64 + t): the
// kernels' issue balance (kernels.h), whose positions hold t < 64.
// So one lane pair takes products of at most kProductLaneMax terms: a larger t would run
// into the next pass's positions, and the positions must not decrease.
constexpr int kProductLaneMax = 64;
struct NoPosStep {
    BN_INLINE void operator()(uint32_t) const {}
};
template <typename Line, typename Step = NoPosStep>
BN_INLINE Fq12<kF> miller_product_scaled(int K, Line&& line, Step&& step = Step{}) {
    Fq12<kF> f = widen<kF>(fq12_one());
    int idx = 0;
#pragma unroll 1
    for (int i = 0; i < BN_NAF_DIGITS + 2; ++i) {
        const uint32_t dpos = (uint32_t)i << 8;
        step(dpos);
        const bool closing = i >= BN_NAF_DIGITS;  // the two lines after the loop: no squaring
        if (!closing && i > 0) f = narrow12<kF>(fq12_sqr(f));
        const int passes = closing ? 1 : 1 + (int)((kNafNonzero >> i) & 1u);
#pragma unroll 1
        for (int ps = 0; ps < passes; ++ps, ++idx) {
#pragma unroll 1
            for (int t = 0; t < K; ++t) {
                step(dpos + 1u + ((uint32_t)ps << 6) + (uint32_t)t);
                const Ell e = line(t, idx);
                if (i == 0 && ps == 0 && t == 0)
                    f = line_from_one_scaled(e);  // one * line (mod.rs:589 on f = one)
                else
                    f = apply_line_scaled(f, e);
            }
        }
    }
    return f;
}

// The Miller loop with the line steps inline (k_pairing_fused): the
// coefficients of g2_precompute applied as they are produced, in
// G2Precomp::miller_loop's order (mod.rs:579-607, 701-727)
// `step(i)` runs at the start of digit i (the kernels' issue balance, kernels.h)
struct NoStep {
    BN_INLINE void operator()(int) const {}
};
// `coeff`: the doubling step's curve constant (curve.h doubling_coeff(), or its
// per-pairing multiple from scaled_inputs below)
template <int B, int PB, int CB, typename Step = NoStep>
BN_INLINE Fq12<kF> miller_fused(const G2Aff<B>& q, const Fq<PB>& px, const Fq<PB>& py, const Fq2<CB>& coeff,
                                Step&& step = Step{}) {
    G2Proj r = {widen<kPt>(q.x), widen<kPt>(q.y), widen<kPt>(fq2_one())};
    const G2Base<B> qb = g2_base(q);
#if BN_LINE_CHAIN & 8
    // digit 0 outside the loop: f = one, so one^2 * line is the line itself
    // (line_from_one), then the digit's addition (NAF digit 0 is +1).  As a branch inside
    // the loop (below) this was slower; peeled, k_pairing_full is faster in every round
    // (profiles/r9_ab_line_chains.txt, mask 11 against mask 3)
    static_assert((kNafNonzero & 1u) != 0 && (kNafMinus & 1u) == 0, "miller_fused: digit 0 is +1");
    step(0);
    Fq12<kF> f = line_from_one(doubling_step(r, coeff), px, py);
    f = apply_line(f, mixed_addition_step(r, g2_base_signed(qb, false)), px, py);
    constexpr int kFirst = 1;
#else
    Fq12<kF> f = widen<kF>(fq12_one());
    constexpr int kFirst = 0;
#endif
#pragma unroll 1
    for (int i = kFirst; i < BN_NAF_DIGITS; ++i) {
        step(i);
        // (sqr_line's first-step shortcut here measured 5 % slower: 4.58 vs 4.35 ms,
        // a register-allocation change; it stays in the segment and coefficient loops)
        f = apply_line(narrow12<kF>(fq12_sqr(f)), doubling_step(r, coeff), px, py);
        if ((kNafNonzero >> i) & 1u) {
            f = apply_line(f, mixed_addition_step(r, g2_base_signed(qb, (kNafMinus >> i) & 1u)), px, py);
        }
    }
    G2Aff<kPt> q1 = mul_by_q(q);
    G2Aff<kPt> q2 = mul_by_q(q1);
    q2.y = fq2_neg(q2.y);
    f = apply_line(f, mixed_addition_step(r, g2_base(q1)), px, py);
    f = apply_line(f, mixed_addition_step(r, g2_base(q2)), px, py);
    return f;
}
template <int B, int PB, typename Step = NoStep>
BN_INLINE Fq12<kF> miller_fused(const G2Aff<B>& q, const Fq<PB>& px, const Fq<PB>& py, Step&& step = Step{}) {
    return miller_fused(q, px, py, doubling_coeff(), static_cast<Step&&>(step));
}

// ---------------------------------------------------------------- prepared G2
// G2Precomp::miller_loop (mod.rs:579-607) over the reference's own coefficients of a
// fixed Q (AffineG2::precompute, not scaled by any P: what bn_g2_precompute_many exports
// and a bn_g2_prepared table holds), each line applied as
//   mul_by_024(ell_0 * s0, ell_vw * sy, ell_vv * sx).
// Two forms (kernels_prepared.hip k_pairing_prepared; compiled for the host by
// tests/native/prepared_emul.cpp):
//   Miller form: s0 = NoScale{} (ell_0 as stored, no product), sy = y_P, sx = x_P of the
//     affine P -- apply_line's operands, so the value is G2Precomp::miller_loop's.
//   Gt form: for P = (X, Y, Z) Jacobian, s0 = Z^3, sy = Y, sx = X Z: every line is the
//     affine line times Z^3, an element of Fq*, so the Miller value is off by a power of
//     Z, which the final exponentiation sends to one (the argument above scaled_inputs
//     below, with the factor on the G1 side alone).  No inversion.
// `line(k)` returns coefficient k (0 .. 86), fetched right before its use; `step(i)` runs
// at the start of digit i (the kernels' issue balance, kernels.h).
struct NoScale {};
BN_INLINE Fq2<kLine> ell_0_scaled(const Fq2<kLine>& e, NoScale) { return e; }
template <int SB>
BN_INLINE Fq2<kLine> ell_0_scaled(const Fq2<kLine>& e, const Fq<SB>& s0) {
    return narrow<kLine>(fq2_scale(e, s0));
}
// one stored line as the loop multiplies by it (apply_line_scaled's operands).  Also what
// k_prepared_expand writes per line for the prepared terms of a product
// (kernels_prepared.hip; compiled for the host by tests/native/products_prepared_emul.cpp).
template <typename S0, int PB>
BN_INLINE Ell prepared_line_scaled(const Ell& c, const S0& s0, const Fq<PB>& sy, const Fq<PB>& sx) {
    return Ell{ell_0_scaled(c.ell_0, s0), narrow<kLine>(fq2_scale(c.ell_vw, sy)),
               narrow<kLine>(fq2_scale(c.ell_vv, sx))};
}
template <typename S0, int PB, typename Line, typename Step = NoStep>
BN_INLINE Fq12<kF> miller_prepared(Line&& line, const S0& s0, const Fq<PB>& sy, const Fq<PB>& sx,
                                   Step&& step = Step{}) {
    auto at = [&](int k) { return prepared_line_scaled(line(k), s0, sy, sx); };
    Fq12<kF> f = widen<kF>(fq12_one());
    int idx = 0;
#pragma unroll 1
    for (int i = 0; i < BN_NAF_DIGITS; ++i) {
        step(i);
        const Ell e = at(idx++);
        // digit 0: one^2 * line is the line itself (line_from_one)
        f = i == 0 ? line_from_one_scaled(e) : apply_line_scaled(narrow12<kF>(fq12_sqr(f)), e);
        if ((kNafNonzero >> i) & 1u) f = apply_line_scaled(f, at(idx++));
    }
    f = apply_line_scaled(f, at(idx++));
    f = apply_line_scaled(f, at(idx));
    return f;
}

// ---------------------------------------------------------------- scaled inputs
// Where only Gt leaves a pairing, the Miller loop can run on scaled coordinates instead
// of affine ones, which takes to_affine's inversion away.  The line steps are
// weighted-homogeneous: with x at weight 2, y at weight 3 and the twist constant b' at
// weight 6, replacing (x_P, y_P, x_Q, y_Q, b') by (l^2 x_P, l^3 y_P, l^2 x_Q, l^3 y_Q,
// l^6 b') for l in Fq* multiplies every coordinate of R and all three terms of every
// line (ell_0, ell_vw * y_P, ell_vv * x_P) by a power of l -- in doubling_step, in
// mixed_addition_step and through mul_by_q, whose constants carry no weight and whose
// conjugation fixes l.  The Miller value changes by a power of l, an element of Fq*,
// which the final exponentiation sends to one ((p - 1) divides (p^6 - 1)): the same Gt.
// (miller_prepared's Gt form above is the case of an affine, fixed Q whose lines are
// already computed: only the G1 side is scaled, l = Z_P, and since the stored ell_vw and
// ell_vv multiply y_P = Y / Z^3 and x_P = X / Z^2, the whole line is taken times Z^3:
// ell_0 Z^3, ell_vw Y, ell_vv X Z.)
// With l = N(Z_Q) Z_P, N = Z_Q.c0^2 + Z_Q.c1^2, nothing is inverted:
//   l^2 X_P / Z_P^2 = N^2 X_P,  l^3 Y_P / Z_P^3 = N^3 Y_P,
//   l / Z_Q = Z_P conj(Z_Q) = m:  l^2 X_Q / Z_Q^2 = m^2 X_Q,  l^3 Y_Q / Z_Q^3 = m^3 Y_Q.
// A point at z == one takes the same formulas (they multiply by one).  A zero z makes
// every output zero; the caller skips that pair and never uses the values.
// `coeff` is l^6 times doubling_coeff(), at its bound: what doubling_step takes.
constexpr bool kCoeffTripled = (BN_LINE_CHAIN & 1) != 0;  // coeff is l^6 * 3 b'
constexpr int kCoeff = kCoeffTripled ? 3 : 2;
using G2Coeff = Fq2<kCoeff>;
struct ScaledPair {
    Fq<2> px, py;
    G2Aff<kPt> qa;
    G2Coeff coeff;
};
// nq = N(qz) (the same value on both lanes of the split layout)
template <int NB>
BN_INLINE ScaledPair scaled_inputs(const Fq<2>& px, const Fq<2>& py, const Fq<2>& pz, const Fq2<2>& qx,
                                   const Fq2<2>& qy, const Fq2<2>& qz, const Fq<NB>& nq) {
    const auto n2 = fq_sqr(nq);
    const auto l1 = fq_mul(nq, pz);
    const auto l2 = fq_sqr(l1);
    const auto l6 = fq_mul(l2, fq_sqr(l2));
    ScaledPair a;
    a.px = fq_mul(px, n2);
    a.py = fq_mul(py, fq_mul(n2, nq));
#if BN_SPLIT
    const auto zp = fq_mul(qz.c, pz);
    const auto m = wrap2(fq_select(lane_odd(), fq_neg(zp), zp));  // Z_P conj(Z_Q)
#else
    const auto m = mk2(fq_mul(qz.c0, pz), fq_neg(fq_mul(qz.c1, pz)));
#endif
    const auto m2 = fq2_sqr(m);
    a.qa = {narrow<kPt>(fq2_mul(qx, m2)), narrow<kPt>(fq2_mul(qy, fq2_mul(m2, m)))};
    a.coeff = widen<kCoeff>(fq2_scale(doubling_coeff(), l6));
    return a;
}
#if !BN_SPLIT
BN_INLINE ScaledPair scaled_inputs(const Fq<2>& px, const Fq<2>& py, const Fq<2>& pz, const Fq2<2>& qx,
                                   const Fq2<2>& qy, const Fq2<2>& qz) {
    return scaled_inputs(px, py, pz, qx, qy, qz, fq_add(fq_sqr(qz.c0), fq_sqr(qz.c1)));
}
#endif

// One segment of the Miller loop: digits [lo, hi) starting from f = one, with
// line coefficients from index `idx` on; the last segment (hi == 64) also
// applies the two lines after the loop.  Running the loop over digits
// [0, 64) in segments g_0 .. g_(S-1) gives f = (..((g_0)^(2^len_1) g_1)^(2^len_2)
// ..) g_(S-1): squaring is a ring homomorphism, so the Horner recombination
// (kernels_wide.hip k_horner_wide) reproduces mod.rs:579-640 exactly.
template <int PB, typename Line, typename Step = NoStep>
BN_INLINE Fq12<kF> miller_segment(const Fq<PB>& px, const Fq<PB>& py, int lo, int hi, int idx, Line&& line,
                                  Step&& step = Step{}) {
    Fq12<kF> f = widen<kF>(fq12_one());
#pragma unroll 1
    for (int i = lo; i < hi; ++i) {
        step(i - lo);
        f = sqr_line(f, i == lo, line(idx++), px, py);
        if ((kNafNonzero >> i) & 1u) f = apply_line(f, line(idx++), px, py);
    }
    if (hi == BN_NAF_DIGITS) {
        f = apply_line(f, line(idx++), px, py);
        f = apply_line(f, line(idx), px, py);
    }
    return f;
}

// ---------------------------------------------------------------- final exponentiation
BN_INLINE Fq12<kF> mul12(const Fq12<kF>& a, const Fq12<kF>& b) { return narrow12<kF>(fq12_mul(a, b)); }
BN_INLINE Fq12<kF> cyc_sqr(const Fq12<kF>& a) { return narrow12<kF>(fq12_cyclotomic_sqr(a)); }

// exp_by_neg_z, fq12.rs:121-124: cyclotomic_pow by u = 4965661367192848881 (fq12.rs:249-266),
// then conjugate.  The first set bit multiplies one by self, i.e. starts at self.
BN_INLINE Fq12<kF> exp_by_neg_z(const Fq12<kF>& a) {
    constexpr uint64_t u = 4965661367192848881ull;  // bit 62 is the top set bit
    Fq12<kF> res = a;
#pragma unroll 1
    for (int bit = 61; bit >= 0; --bit) {
        res = cyc_sqr(res);
        if ((u >> bit) & 1u) res = mul12(a, res);
    }
    return fq12_conj(res);
}

// fq12.rs:62-73 (first chunk, given f != 0)
BN_INLINE Fq12<kF> fe_first_chunk(const Fq12<kF>& f) {
    Fq12<kF> b = narrow12<kF>(fq12_inv(f));
    Fq12<kF> a = fq12_conj(f);
    Fq12<kF> c = mul12(a, b);
    Fq12<kF> d = narrow12<kF>(fq12_frobenius_map<2>(c));
    return mul12(d, c);
}
// fq12.rs:75-105 (last chunk)
BN_INLINE Fq12<kF> fe_last_chunk(const Fq12<kF>& self) {
    Fq12<kF> a = exp_by_neg_z(self);
    Fq12<kF> b = cyc_sqr(a);
    Fq12<kF> c = cyc_sqr(b);
    Fq12<kF> d = mul12(c, b);
    Fq12<kF> e = exp_by_neg_z(d);
    Fq12<kF> f = cyc_sqr(e);
    Fq12<kF> g = exp_by_neg_z(f);
    Fq12<kF> h = fq12_conj(d);
    Fq12<kF> i = fq12_conj(g);
    Fq12<kF> j = mul12(i, e);
    Fq12<kF> k = mul12(j, h);
    Fq12<kF> l = mul12(k, b);
    Fq12<kF> m = mul12(k, e);
    Fq12<kF> n = mul12(self, m);
    Fq12<kF> o = narrow12<kF>(fq12_frobenius_map<1>(l));
    Fq12<kF> p = mul12(o, n);
    Fq12<kF> q = narrow12<kF>(fq12_frobenius_map<2>(k));
    Fq12<kF> r = mul12(q, p);
    Fq12<kF> s = fq12_conj(self);
    Fq12<kF> t = mul12(s, l);
    Fq12<kF> u = narrow12<kF>(fq12_frobenius_map<3>(t));
    return mul12(u, r);
}

}  // namespace bn
