// fq2_split.h -- Fq2 = Fq[u]/(u^2+1) with TWO lanes per element (BN_SPLIT;
// included by tower.h inside namespace bn).
//
// Lanes 2j and 2j+1 of a wave hold coordinate c0 and c1 of element j.  Every
// Fq2 operation below computes this lane's coordinate of the result; the
// other coordinate, when needed, comes from the partner lane over DPP
// (quad_perm [1,0,3,2]: one v_mov_b32_dpp per 32-bit digit).  Additions,
// subtractions, halving, folds and scaling by an Fq are lane-local: each lane
// does half of the unsplit work.  A product is one column sum of two digit
// products per lane, reduced once -- lane 0: a0*b0 + a1*(K*p - b1), lane 1:
// a0*b1 + a1*b0 -- i.e. exactly one coordinate of fq2_mul_sb.
//
// Why: with one lane per element a batch of 2^16 pairings is 1024 waves, one
// per SIMD, and a lone wave issues one VALU instruction every ~6 cycles
// whatever the instruction; two waves per SIMD issue the digit-wise VOP2 work
// 2.5x faster and MADs ~15 % faster (profiles/r2d_valu_ubench.jsonl).  Split
// lanes give 2048 waves for the same batch, and each lane holds half the
// state (an Fq12 is 54 VGPRs), so two waves fit the register file.
//
// Bit-exactness: each lane computes the same residue as the corresponding
// coordinate of the one-lane formulas (the same ring identities), and values
// are canonicalized only at the boundary.

template <int B>
struct Fq2 {
    Fq<B> c;  // this lane's coordinate: c0 on even lanes, c1 on odd lanes
};

BN_INLINE bool lane_odd() {
#if defined(__HIP_DEVICE_COMPILE__)
    return (__builtin_amdgcn_workitem_id_x() & 1u) != 0;
#else
    return false;
#endif
}
// the partner lane's copy of a 32-bit value (lanes 2j <-> 2j+1)
BN_INLINE uint32_t swap_pair(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
#else
    return v;
#endif
}
template <int B>
BN_INLINE Fq<B> fq_partner(const Fq<B>& a) {
    Fq<B> r;
#pragma unroll
    for (int l = 0; l < 9; ++l) r.v[l] = swap_pair(a.v[l]);
    return r;
}
// coordinate c0 (CTRL 0xA0: quad_perm [0,0,2,2]) or c1 (0xF5: [1,1,3,3]) of the
// element on both lanes of the pair: one DPP move per digit, no select
template <int CTRL>
BN_INLINE uint32_t bcast_pair(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
#else
    return v;  // host builds run one lane per element: see the host forms below
#endif
}
template <int B>
BN_INLINE Fq<B> fq_bcast_c0(const Fq<B>& a) {
    Fq<B> r;
#pragma unroll
    for (int l = 0; l < 9; ++l) r.v[l] = bcast_pair<0xA0>(a.v[l]);
    return r;
}
template <int B>
BN_INLINE Fq<B> fq_bcast_c1(const Fq<B>& a) {
    Fq<B> r;
#pragma unroll
    for (int l = 0; l < 9; ++l) r.v[l] = bcast_pair<0xF5>(a.v[l]);
    return r;
}
template <int K>
BN_INLINE Fq2<K> wrap2(const Fq<K>& x) { return {x}; }

template <int B2, int B>
BN_INLINE Fq2<B2> widen(const Fq2<B>& a) { return {widen<B2>(a.c)}; }

BN_INLINE Fq2<1> fq2_const(const Limbs9& c0, const Limbs9& c1) {
    return {fq_select(lane_odd(), fq_from_limbs<1>(c1), fq_from_limbs<1>(c0))};
}
BN_INLINE Fq2<1> fq2_zero() { return {fq_zero()}; }
BN_INLINE Fq2<1> fq2_one() { return {fq_select(lane_odd(), fq_zero(), fq_one())}; }
template <int B>
BN_INLINE Fq2<B> fq2_select(bool c, const Fq2<B>& a, const Fq2<B>& b) { return {fq_select(c, a.c, b.c)}; }
template <int A, int B>
BN_INLINE auto fq2_add(const Fq2<A>& a, const Fq2<B>& b) { return wrap2(fq_add(a.c, b.c)); }
template <int A, int B>
BN_INLINE auto fq2_sub(const Fq2<A>& a, const Fq2<B>& b) { return wrap2(fq_sub(a.c, b.c)); }
template <int B>
BN_INLINE auto fq2_neg(const Fq2<B>& a) { return wrap2(fq_neg(a.c)); }
template <int B>
BN_INLINE auto fq2_dbl(const Fq2<B>& a) { return fq2_add(a, a); }
template <int B>
BN_INLINE Fq2<2> fq2_fold(const Fq2<B>& a) { return {fq_fold(a.c)}; }
template <int B>
BN_INLINE Fq2<kv(B)> fq2_norm(const Fq2<B>& a) { return {fq_norm(a.c)}; }
template <int B>
BN_INLINE auto fq2_half(const Fq2<B>& a) { return wrap2(fq_half(a.c)); }
// fq2.rs:48-53 (s must hold the same value on both lanes of the element)
template <int A, int B>
BN_INLINE auto fq2_scale(const Fq2<A>& a, const Fq<B>& s) { return wrap2(fq_mul(a.c, s)); }
template <int L, int B>
BN_INLINE auto pre(const Fq2<B>& a) {
    if constexpr (kv(B) <= L) return a; else return fq2_fold(a);
}
// both lanes agree: element zero iff both coordinates are
template <int B>
BN_INLINE bool fq2_is_zero(const Fq2<B>& a) {
    const uint32_t z = fq_is_zero(a.c) ? 1u : 0u;
    return (z & swap_pair(z)) != 0;
}
template <int A, int B>
BN_INLINE bool fq2_eq(const Fq2<A>& a, const Fq2<B>& b) {
    const uint32_t e = fq_eq(a.c, b.c) ? 1u : 0u;
    return (e & swap_pair(e)) != 0;
}
// The two-lane products (below) run without compiler fences around them.  Rounds 2-4
// fenced their inputs and results to keep the compiler from interleaving the
// digit products of several Fq2 products; since every product is one asm statement
// (BN_DOT2_ASM) there is nothing to interleave, and the "+v" input fences only made
// the compiler copy every input it still needed (the fenced value counts as
// rewritten): k_pairing_full 6.3 % fewer instructions, scratch 716 -> 584 B/lane,
// 7.60-7.62 -> 7.47-7.49 ms (frac 0.491 -> 0.500), G2 * Fr 6.01-6.08 -> 5.82-5.86 ms
// (profiles/r5q_ab_fence.txt)

// K*p - x without a carry pass (digits < (sub_spread(L)+2)*2^29, value <= (B+1)*p)
template <int K>
BN_INLINE Fq<kenc(kv(K) + 1, sub_spread(kl(K)) + 2)> fq_neg_lazy(const Fq<K>& x) {
    constexpr Limbs9 Q = kp_spread(kv(K) + 1, sub_spread(kl(K)));
    Fq<kenc(kv(K) + 1, sub_spread(kl(K)) + 2)> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v[i] = Q.v[i] - x.v[i];
    return r;
}
// fq2_mul_split takes its w operand (lane 0: K*p - b1, lane 1: b1) as one
// v_cndmask_b32_dpp per digit -- odd lanes keep their own b1, even lanes take the
// partner's K*p - b1 through the DPP swap -- instead of a broadcast, a negation
// and a select: 9 VALU fewer per product, k_pairing_full 7.79-7.81 -> 7.73-7.75 ms
// (profiles/r3r_ab_dppsel.txt)
#if defined(__HIP_DEVICE_COMPILE__)
#define BN_DPPSEL_VCC "s_mov_b32 vcc_lo, 0xaaaaaaaa\n\ts_mov_b32 vcc_hi, 0xaaaaaaaa\n\ts_nop 1\n\t"
#define BN_DPPSEL_OP(o, a, b) "v_cndmask_b32_dpp %" #o ", %" #a ", %" #b ", vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
// w[i] = odd lane ? own[i] : the partner's neg[i].  The s_nop covers the two
// wait states a DPP read needs after the VALU write of its source (the hazard
// recognizer does not look inside inline asm).
BN_INLINE void dpp_sel_own_partner(uint32_t (&w)[9], const uint32_t (&own)[9], const uint32_t (&neg)[9]) {
    const uint32_t odd = __builtin_amdgcn_workitem_id_x() & 1u;
    asm(BN_DPPSEL_VCC BN_DPPSEL_OP(0, 9, 18) BN_DPPSEL_OP(1, 10, 19) BN_DPPSEL_OP(2, 11, 20) BN_DPPSEL_OP(3, 12, 21)
            BN_DPPSEL_OP(4, 13, 22) BN_DPPSEL_OP(5, 14, 23) BN_DPPSEL_OP(6, 15, 24) BN_DPPSEL_OP(7, 16, 25)
                BN_DPPSEL_OP(8, 17, 26)
        : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5]), "=&v"(w[6]), "=&v"(w[7]),
          "=&v"(w[8])
        : "v"(neg[0]), "v"(neg[1]), "v"(neg[2]), "v"(neg[3]), "v"(neg[4]), "v"(neg[5]), "v"(neg[6]), "v"(neg[7]),
          "v"(neg[8]), "v"(own[0]), "v"(own[1]), "v"(own[2]), "v"(own[3]), "v"(own[4]), "v"(own[5]), "v"(own[6]),
          "v"(own[7]), "v"(own[8]), "v"(odd)
        : "vcc");
}
#endif
// per-lane choice between two values of different static types (the join)
template <int A, int B>
BN_INLINE Fq<kjoin(A, B)> fq_pick(bool c, const Fq<A>& a, const Fq<B>& b) {
    Fq<kjoin(A, B)> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}

// REDC(x*y + z*w): one Montgomery reduction of a two-product column sum (the
// fq_mul column scan with a second product per column).  Column sums stay
// below 2^64 when Lx*Ly + Lz*Lw <= 6.
template <int X, int Y, int Z, int W>
BN_INLINE auto fq_dot2(const Fq<X>& x, const Fq<Y>& y, const Fq<Z>& z, const Fq<W>& w) {
    static_assert(kl(X) * kl(Y) + kl(Z) * kl(W) <= 6, "fq_dot2: column sum could overflow 64 bits");
    constexpr int BO = 1 + (int)(((long long)kv(X) * kv(Y) + (long long)kv(Z) * kv(W)) * 5908 / 1000000 + 1);
    Fq<BO> r;
#if BN_DOT2_ASM && defined(__HIP_DEVICE_COMPILE__)
    if constexpr ((BN_DOT2_ASM & 1) != 0) {
        asm(BN_ASM_DOT2 : BN_ASM_OUT9(r.v) : BN_ASM_IN9(x.v), BN_ASM_IN9(y.v), BN_ASM_IN9(z.v), BN_ASM_IN9(w.v), BN_ASM_P
            : BN_ASM_CLOBBER);
        return r;
    }
#endif
    uint32_t m[9];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        const int lo = k < 9 ? 0 : k - 8;
        const int hi = k < 9 ? k : 8;
#pragma unroll
        for (int i = lo; i <= hi; ++i) {
            acc += (uint64_t)x.v[i] * y.v[k - i];
            acc += (uint64_t)z.v[i] * w.v[k - i];
        }
#pragma unroll
        for (int i = lo; i <= hi; ++i)
            if (i < k) acc += (uint64_t)m[i] * kP29.v[k - i];
        if (k < 9) {
            m[k] = ((uint32_t)acc * BN_PINV29) & M29;
            acc += (uint64_t)m[k] * kP29.v[0];
        } else {
            r.v[k - 9] = (uint32_t)acc & M29;
        }
        acc >>= 29;
    }
    r.v[8] = (uint32_t)acc;
    return r;
}

// fq_dot2 with addends at weight R.  Columns 9..17 of
// the chain -- the ones that leave as digits 0..8 -- also take digit d of each addend
// c_j, times a small constant K_j that rides as the multiply-add's inline constant:
//   r = REDC(x*y + z*w) + sum K_j * c_j   (r * R == x*y + z*w + R * sum K_j * c_j mod p).
// Small multiples, sums and differences (a subtrahend enters as K*p - c, fq_neg_lazy)
// that would follow the product as digit-wise passes, K*p spreads and a carry pass
// cost one multiply-add per digit and leave normalized: next to the 2^58-sized
// digit products a term K_j * c_j[d] < 2^36 is invisible in the 64-bit accumulator.
// The value bound of every addend, times its multiplier, adds to the product's.
// NA of the three addends are used (the others: K == 0, any operand)
template <int NA, int K0, int K1, int K2, int X, int Y, int Z, int W, int C0, int C1, int C2>
BN_INLINE auto fq_dot2_addn(const Fq<X>& x, const Fq<Y>& y, const Fq<Z>& z, const Fq<W>& w, const Fq<C0>& c0,
                            const Fq<C1>& c1, const Fq<C2>& c2) {
    static_assert(NA >= 1 && NA <= 3 && K0 >= 1 && (NA > 1 ? K1 >= 1 : K1 == 0) && (NA > 2 ? K2 >= 1 : K2 == 0),
                  "fq_dot2_add: multipliers of the addends in use");
    static_assert(K0 <= 64 && K1 <= 64 && K2 <= 64, "fq_dot2_add: a multiplier must be an inline constant");
    // a column: 54 digit products and 9 m*p terms < 2^58 each (63 * 2^58), a carry < 2^35
    // and the addend digits, together below 2^50 < 2^58 - 2^35
    static_assert(kl(X) * kl(Y) + kl(Z) * kl(W) <= 6, "fq_dot2_add: column sum could overflow 64 bits");
    static_assert((long long)K0 * kl(C0) + (long long)K1 * kl(C1) + (long long)K2 * kl(C2) <= (1 << 20),
                  "fq_dot2_add: column sum could overflow 64 bits");
    constexpr int BP = 1 + (int)(((long long)kv(X) * kv(Y) + (long long)kv(Z) * kv(W)) * 5908 / 1000000 + 1);
    constexpr int BO = BP + K0 * kv(C0) + K1 * kv(C1) + K2 * kv(C2);
    static_assert(BO <= kMaxBound, "fq_dot2_add: the value must stay below 2^261");
    Fq<BO> r;
#if BN_DOT2_ASM && defined(__HIP_DEVICE_COMPILE__)
    if constexpr ((BN_DOT2_ASM & 1) != 0) {
        if constexpr (NA == 1) {
            asm(BN_ASM_DOT2A1 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x.v), BN_ASM_IN9(y.v), BN_ASM_IN9(z.v), BN_ASM_IN9(w.v), BN_ASM_IN9(c0.v), BN_ASM_P, "n"(K0)
                : BN_ASM_CLOBBER);
        } else if constexpr (NA == 2) {
            asm(BN_ASM_DOT2A2 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x.v), BN_ASM_IN9(y.v), BN_ASM_IN9(z.v), BN_ASM_IN9(w.v), BN_ASM_IN9(c0.v), BN_ASM_IN9(c1.v),
                  BN_ASM_P, "n"(K0), "n"(K1)
                : BN_ASM_CLOBBER);
        } else {
            asm(BN_ASM_DOT2A3 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x.v), BN_ASM_IN9(y.v), BN_ASM_IN9(z.v), BN_ASM_IN9(w.v), BN_ASM_IN9(c0.v), BN_ASM_IN9(c1.v),
                  BN_ASM_IN9(c2.v), BN_ASM_P, "n"(K0), "n"(K1), "n"(K2)
                : BN_ASM_CLOBBER);
        }
        return r;
    }
#endif
    uint32_t m[9];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        const int lo = k < 9 ? 0 : k - 8;
        const int hi = k < 9 ? k : 8;
#pragma unroll
        for (int i = lo; i <= hi; ++i) {
            acc += (uint64_t)x.v[i] * y.v[k - i];
            acc += (uint64_t)z.v[i] * w.v[k - i];
        }
#pragma unroll
        for (int i = lo; i <= hi; ++i)
            if (i < k) acc += (uint64_t)m[i] * kP29.v[k - i];
        if (k < 9) {
            m[k] = ((uint32_t)acc * BN_PINV29) & M29;
            acc += (uint64_t)m[k] * kP29.v[0];
        } else {
            acc += (uint64_t)c0.v[k - 9] * K0;
            if constexpr (NA > 1) acc += (uint64_t)c1.v[k - 9] * K1;
            if constexpr (NA > 2) acc += (uint64_t)c2.v[k - 9] * K2;
            r.v[k - 9] = k < 17 ? (uint32_t)acc & M29 : (uint32_t)acc;
        }
        acc >>= 29;
    }
    return r;
}
template <int K0, int X, int Y, int Z, int W, int C0>
BN_INLINE auto fq_dot2_add(const Fq<X>& x, const Fq<Y>& y, const Fq<Z>& z, const Fq<W>& w, const Fq<C0>& c0) {
    return fq_dot2_addn<1, K0, 0, 0>(x, y, z, w, c0, c0, c0);
}
template <int K0, int K1, int X, int Y, int Z, int W, int C0, int C1>
BN_INLINE auto fq_dot2_add(const Fq<X>& x, const Fq<Y>& y, const Fq<Z>& z, const Fq<W>& w, const Fq<C0>& c0,
                           const Fq<C1>& c1) {
    return fq_dot2_addn<2, K0, K1, 0>(x, y, z, w, c0, c1, c1);
}
template <int K0, int K1, int K2, int X, int Y, int Z, int W, int C0, int C1, int C2>
BN_INLINE auto fq_dot2_add(const Fq<X>& x, const Fq<Y>& y, const Fq<Z>& z, const Fq<W>& w, const Fq<C0>& c0,
                           const Fq<C1>& c1, const Fq<C2>& c2) {
    return fq_dot2_addn<3, K0, K1, K2>(x, y, z, w, c0, c1, c2);
}

// The same for one product (dot2_asm.inc MULA1..3): r = REDC(x*y) + sum K_j * c_j, the
// fq_mul chain with the addends' digits on columns 9..17.  Column budget: 9 digit
// products < Lx*Ly * 2^58 and 9 m*p terms < 2^58 (at most 63 * 2^58 with Lx*Ly <= 6), the
// carry and the addend digits below 2^50.
template <int NA, int K0, int K1, int K2, int X, int Y, int C0, int C1, int C2>
BN_INLINE auto fq_mul_addn(const Fq<X>& x, const Fq<Y>& y, const Fq<C0>& c0, const Fq<C1>& c1, const Fq<C2>& c2) {
    static_assert(NA >= 1 && NA <= 3 && K0 >= 1 && (NA > 1 ? K1 >= 1 : K1 == 0) && (NA > 2 ? K2 >= 1 : K2 == 0),
                  "fq_mul_add: multipliers of the addends in use");
    static_assert(K0 <= 64 && K1 <= 64 && K2 <= 64, "fq_mul_add: a multiplier must be an inline constant");
    static_assert(kl(X) * kl(Y) <= 6, "fq_mul_add: column sum could overflow 64 bits");
    static_assert((long long)K0 * kl(C0) + (long long)K1 * kl(C1) + (long long)K2 * kl(C2) <= (1 << 20),
                  "fq_mul_add: column sum could overflow 64 bits");
    constexpr int BO = mul_bound(kv(X), kv(Y)) + K0 * kv(C0) + K1 * kv(C1) + K2 * kv(C2);
    static_assert(BO <= kMaxBound, "fq_mul_add: the value must stay below 2^261");
    Fq<BO> r;
#if BN_DOT2_ASM && defined(__HIP_DEVICE_COMPILE__)
    if constexpr ((BN_DOT2_ASM & 2) != 0) {
        if constexpr (NA == 1) {
            asm(BN_ASM_MULA1 : BN_ASM_OUT9(r.v) : BN_ASM_IN9(x.v), BN_ASM_IN9(y.v), BN_ASM_IN9(c0.v), BN_ASM_P, "n"(K0)
                : BN_ASM_CLOBBER);
        } else if constexpr (NA == 2) {
            asm(BN_ASM_MULA2 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x.v), BN_ASM_IN9(y.v), BN_ASM_IN9(c0.v), BN_ASM_IN9(c1.v), BN_ASM_P, "n"(K0), "n"(K1)
                : BN_ASM_CLOBBER);
        } else {
            asm(BN_ASM_MULA3 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x.v), BN_ASM_IN9(y.v), BN_ASM_IN9(c0.v), BN_ASM_IN9(c1.v), BN_ASM_IN9(c2.v), BN_ASM_P,
                  "n"(K0), "n"(K1), "n"(K2)
                : BN_ASM_CLOBBER);
        }
        return r;
    }
#endif
    uint32_t m[9];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        const int lo = k < 9 ? 0 : k - 8;
        const int hi = k < 9 ? k : 8;
#pragma unroll
        for (int i = lo; i <= hi; ++i) acc += (uint64_t)x.v[i] * y.v[k - i];
#pragma unroll
        for (int i = lo; i <= hi; ++i)
            if (i < k) acc += (uint64_t)m[i] * kP29.v[k - i];
        if (k < 9) {
            m[k] = ((uint32_t)acc * BN_PINV29) & M29;
            acc += (uint64_t)m[k] * kP29.v[0];
        } else {
            acc += (uint64_t)c0.v[k - 9] * K0;
            if constexpr (NA > 1) acc += (uint64_t)c1.v[k - 9] * K1;
            if constexpr (NA > 2) acc += (uint64_t)c2.v[k - 9] * K2;
            r.v[k - 9] = k < 17 ? (uint32_t)acc & M29 : (uint32_t)acc;
        }
        acc >>= 29;
    }
    return r;
}
template <int K0, int X, int Y, int C0>
BN_INLINE auto fq_mul_add(const Fq<X>& x, const Fq<Y>& y, const Fq<C0>& c0) {
    return fq_mul_addn<1, K0, 0, 0>(x, y, c0, c0, c0);
}
template <int K0, int K1, int X, int Y, int C0, int C1>
BN_INLINE auto fq_mul_add(const Fq<X>& x, const Fq<Y>& y, const Fq<C0>& c0, const Fq<C1>& c1) {
    return fq_mul_addn<2, K0, K1, 0>(x, y, c0, c1, c1);
}
template <int K0, int K1, int K2, int X, int Y, int C0, int C1, int C2>
BN_INLINE auto fq_mul_add(const Fq<X>& x, const Fq<Y>& y, const Fq<C0>& c0, const Fq<C1>& c1, const Fq<C2>& c2) {
    return fq_mul_addn<3, K0, K1, K2>(x, y, c0, c1, c2);
}

// REDC(x0*y0 + x1*y1 + x2*y2 + x3*y3) [+ K0*c0 [+ K1*c1]]: one Montgomery reduction of a
// four-product column sum (dot2_asm.inc DOT4, DOT4A1, DOT4A2) -- two Fq2 products' worth of
// this lane's coordinate.  A column holds at most 9 * sum(Lx_t * Ly_t) digit products and
// 9 m*p terms below 2^58 each: under 2^64 while the sum is <= 6, as for fq_dot2.
template <int NA, int K0, int K1, int X0, int Y0, int X1, int Y1, int X2, int Y2, int X3, int Y3, int C0, int C1>
BN_INLINE auto fq_dot4_addn(const Fq<X0>& x0, const Fq<Y0>& y0, const Fq<X1>& x1, const Fq<Y1>& y1, const Fq<X2>& x2,
                            const Fq<Y2>& y2, const Fq<X3>& x3, const Fq<Y3>& y3, const Fq<C0>& c0, const Fq<C1>& c1) {
    static_assert(NA >= 0 && NA <= 2 && (NA > 0 ? K0 >= 1 : K0 == 0) && (NA > 1 ? K1 >= 1 : K1 == 0),
                  "fq_dot4: multipliers of the addends in use");
    static_assert(K0 <= 64 && K1 <= 64, "fq_dot4: a multiplier must be an inline constant");
    static_assert(kl(X0) * kl(Y0) + kl(X1) * kl(Y1) + kl(X2) * kl(Y2) + kl(X3) * kl(Y3) <= 6,
                  "fq_dot4: column sum could overflow 64 bits");
    static_assert((long long)K0 * kl(C0) + (long long)K1 * kl(C1) <= (1 << 20),
                  "fq_dot4: column sum could overflow 64 bits");
    constexpr long long S = (long long)kv(X0) * kv(Y0) + (long long)kv(X1) * kv(Y1) + (long long)kv(X2) * kv(Y2) +
                            (long long)kv(X3) * kv(Y3);
    constexpr int BO = 1 + (int)(S * 5908 / 1000000 + 1) + K0 * kv(C0) + K1 * kv(C1);
    static_assert(BO <= kMaxBound, "fq_dot4: the value must stay below 2^261");
    Fq<BO> r;
#if BN_DOT2_ASM && defined(__HIP_DEVICE_COMPILE__)
    if constexpr ((BN_DOT2_ASM & 1) != 0) {
        if constexpr (NA == 0) {
            asm(BN_ASM_DOT4 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x0.v), BN_ASM_IN9(y0.v), BN_ASM_IN9(x1.v), BN_ASM_IN9(y1.v), BN_ASM_IN9(x2.v),
                  BN_ASM_IN9(y2.v), BN_ASM_IN9(x3.v), BN_ASM_IN9(y3.v), BN_ASM_P
                : BN_ASM_CLOBBER);
        } else if constexpr (NA == 1) {
            asm(BN_ASM_DOT4A1 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x0.v), BN_ASM_IN9(y0.v), BN_ASM_IN9(x1.v), BN_ASM_IN9(y1.v), BN_ASM_IN9(x2.v),
                  BN_ASM_IN9(y2.v), BN_ASM_IN9(x3.v), BN_ASM_IN9(y3.v), BN_ASM_IN9(c0.v), BN_ASM_P, "n"(K0)
                : BN_ASM_CLOBBER);
        } else {
            asm(BN_ASM_DOT4A2 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(x0.v), BN_ASM_IN9(y0.v), BN_ASM_IN9(x1.v), BN_ASM_IN9(y1.v), BN_ASM_IN9(x2.v),
                  BN_ASM_IN9(y2.v), BN_ASM_IN9(x3.v), BN_ASM_IN9(y3.v), BN_ASM_IN9(c0.v), BN_ASM_IN9(c1.v), BN_ASM_P,
                  "n"(K0), "n"(K1)
                : BN_ASM_CLOBBER);
        }
        return r;
    }
#endif
    uint32_t m[9];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        const int lo = k < 9 ? 0 : k - 8;
        const int hi = k < 9 ? k : 8;
#pragma unroll
        for (int i = lo; i <= hi; ++i) {
            acc += (uint64_t)x0.v[i] * y0.v[k - i];
            acc += (uint64_t)x1.v[i] * y1.v[k - i];
            acc += (uint64_t)x2.v[i] * y2.v[k - i];
            acc += (uint64_t)x3.v[i] * y3.v[k - i];
        }
#pragma unroll
        for (int i = lo; i <= hi; ++i)
            if (i < k) acc += (uint64_t)m[i] * kP29.v[k - i];
        if (k < 9) {
            m[k] = ((uint32_t)acc * BN_PINV29) & M29;
            acc += (uint64_t)m[k] * kP29.v[0];
        } else {
            if constexpr (NA > 0) acc += (uint64_t)c0.v[k - 9] * K0;
            if constexpr (NA > 1) acc += (uint64_t)c1.v[k - 9] * K1;
            r.v[k - 9] = k < 17 ? (uint32_t)acc & M29 : (uint32_t)acc;
        }
        acc >>= 29;
    }
    return r;
}
template <int X0, int Y0, int X1, int Y1, int X2, int Y2, int X3, int Y3>
BN_INLINE auto fq_dot4(const Fq<X0>& x0, const Fq<Y0>& y0, const Fq<X1>& x1, const Fq<Y1>& y1, const Fq<X2>& x2,
                       const Fq<Y2>& y2, const Fq<X3>& x3, const Fq<Y3>& y3) {
    return fq_dot4_addn<0, 0, 0>(x0, y0, x1, y1, x2, y2, x3, y3, x0, x0);
}

// K0*c0 + K1*c1 [+ K2*c2] with normalized digits: the addends without a product, as
// one carry chain (dot2_asm.inc LIN2 / LIN3: per digit the carry shift, one
// multiply-add per term and the 29-bit extract).  For combinations whose multiples
// overflow a 32-bit digit (9 * b) or would need a carry pass of their own.
template <int NA, int K0, int K1, int K2, int C0, int C1, int C2>
BN_INLINE auto fq_linn(const Fq<C0>& c0, const Fq<C1>& c1, const Fq<C2>& c2) {
    static_assert((NA == 2 || NA == 3) && K0 >= 1 && K1 >= 1 && (NA > 2 ? K2 >= 1 : K2 == 0), "fq_lin: multipliers");
    static_assert(K0 <= 64 && K1 <= 64 && K2 <= 64, "fq_lin: a multiplier must be an inline constant");
    // a digit's sum < 3 * 64 * 7 * 2^29 and the carry < 2^12: far below 2^64
    constexpr int BO = K0 * kv(C0) + K1 * kv(C1) + K2 * kv(C2);
    static_assert(BO <= kMaxBound, "fq_lin: the value must stay below 2^261");
    Fq<BO> r;
#if BN_DOT2_ASM && defined(__HIP_DEVICE_COMPILE__)
    if constexpr ((BN_DOT2_ASM & 1) != 0) {
        if constexpr (NA == 2) {
            asm(BN_ASM_LIN2 : BN_ASM_OUT9(r.v) : BN_ASM_IN9(c0.v), BN_ASM_IN9(c1.v), "n"(K0), "n"(K1) : BN_ASM_CLOBBER);
        } else {
            asm(BN_ASM_LIN3 : BN_ASM_OUT9(r.v)
                : BN_ASM_IN9(c0.v), BN_ASM_IN9(c1.v), BN_ASM_IN9(c2.v), "n"(K0), "n"(K1), "n"(K2)
                : BN_ASM_CLOBBER);
        }
        return r;
    }
#endif
    uint64_t acc = 0;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        acc += (uint64_t)c0.v[d] * K0 + (uint64_t)c1.v[d] * K1;
        if constexpr (NA > 2) acc += (uint64_t)c2.v[d] * K2;
        r.v[d] = d < 8 ? (uint32_t)acc & M29 : (uint32_t)acc;
        acc >>= 29;
    }
    return r;
}
template <int K0, int K1, int C0, int C1>
BN_INLINE auto fq_lin(const Fq<C0>& c0, const Fq<C1>& c1) {
    return fq_linn<2, K0, K1, 0>(c0, c1, c1);
}
template <int K0, int K1, int K2, int C0, int C1, int C2>
BN_INLINE auto fq_lin(const Fq<C0>& c0, const Fq<C1>& c1, const Fq<C2>& c2) {
    return fq_linn<3, K0, K1, K2>(c0, c1, c2);
}

// fq2.rs:136-148 (the same residues as fq2_mul_sb): lane 0 computes
// c0 = a0*b0 + a1*(K*p - b1), lane 1 computes c1 = a1*b0 + a0*b1, both as
// own_a * Y + partner_a * W with per-lane operand choice.
// the fq_dot2 column budget of fq2_mul_split(a, b) for digit bounds La, Lb: x = a,
// y = b or its partner (Lb), z = partner of a (La), w = b or K*p - partner (fq_neg_lazy)
constexpr int split_mul_cost(int La, int Lb) {
    return La * Lb + La * (Lb > sub_spread(Lb) + 2 ? Lb : sub_spread(Lb) + 2);
}
template <int A, int B>
BN_INLINE auto fq2_mul_split(const Fq2<A>& a, const Fq2<B>& b) {
    if constexpr (split_mul_cost(kl(A), kl(B)) > 6) {
        if constexpr (split_mul_cost(kl(B), kl(A)) <= 6) return fq2_mul_split(b, a);
        else if constexpr (kl(A) >= kl(B)) return fq2_mul_split(fq2_norm(a), b);
        else return fq2_mul_split(a, fq2_norm(b));
    } else {
        const bool odd = lane_odd();
        const Fq<A> pa = fq_partner(a.c);
#if defined(__HIP_DEVICE_COMPILE__)
        const Fq<B> y = fq_bcast_c0(b.c);
        const auto nb = fq_neg_lazy(b.c);  // the odd lane's is K*p - b1
        Fq<kjoin(B, kenc(kv(B) + 1, sub_spread(kl(B)) + 2))> w;
        dpp_sel_own_partner(w.v, b.c.v, nb.v);
        (void)odd;
#else
        const Fq<B> pb = fq_partner(b.c);
        const Fq<B> y = fq_select(odd, pb, b.c);
        const auto w = fq_pick(odd, b.c, fq_neg_lazy(pb));
#endif
        return wrap2(fq_dot2(a.c, y, pa, w));
    }
}
// The cyclotomic square on the addend chains (tower.h fq12_cyclotomic_sqr).
// BN_CYC_LIN bits: 1 = the product's operand xi*b + a, 2 = the outputs n1 and n5,
// 4 = n2 through fq_lin instead of digit-wise passes.  Off by default: 116 VALU fewer
// per square, but next to the Karatsuba Fq12 products k_pairing_full then spills 108 B
// more per lane and runs 3-5 % slower (profiles/r7_ab_cyc_lin.txt).  kernels_gtpow.hip
// turns all three on, and so does kernels_pairing.hip since its Fq12 products run on
// six-product column sums (tower.h BN_FQ6_LAZY; profiles/r8_ab_fq6_lazy.txt).
#ifndef BN_CYC_LIN
#define BN_CYC_LIN 0
#endif
// fq2_cyc_xt: the partner's coordinate of tmp with the sign of -xi * tmp's cross
// term -- lane 0: tmp1, lane 1: K*p - tmp0.
template <int T>
BN_INLINE auto fq2_cyc_xt(const Fq2<T>& tmp) {
    return fq_partner(fq_pick(lane_odd(), tmp.c, fq_neg_lazy(tmp.c)));
}
// fq2_cyc_u: t - z = (a + b)(xi*b + a) - (1 + xi)*tmp - z,  tmp = a*b,  xi = 9 + u,
// per lane own(product) - 10*own(tmp) + xt - own(z).  The product is
// fq2_mul_split's column sum; the three terms enter it as 10 * (K*p - tmp), xt
// and K*p - z.  Its operand xi*b + a = 9*own(b) + (lane 0: K*p - b1, lane 1: b0)
// + own(a) is fq2_mul_xi and a carry pass, or with BN_CYC_LIN & 1 one fq_lin chain
// (9 * b overflows a 32-bit digit).  Normalized digits, value bound the product's + 39.
template <int A, int B, int T, int XT, int ZB>
BN_INLINE auto fq2_cyc_u(const Fq2<A>& a, const Fq2<B>& b, const Fq2<T>& tmp, const Fq<XT>& xt, const Fq2<ZB>& zs) {
    static_assert(kl(T) == 1 && kl(ZB) == 1, "fq2_cyc_u: normalized tmp and z");
    const bool odd = lane_odd();
    const auto s = fq2_add(a, b);
#if BN_CYC_LIN & 1
    const auto pb = fq_partner(b.c);
    const auto y2 = fq_lin<9, 1>(b.c, fq_add(fq_pick(odd, pb, fq_neg_lazy(pb)), a.c));
#else
    const auto y2 = fq_norm(fq_add(fq2_mul_xi(b).c, a.c));
    (void)odd;
#endif
    static_assert(split_mul_cost(kl(decltype(s.c)::kK), 1) <= 6, "fq2_cyc_u: column budget");
    const auto ps = fq_partner(s.c);
    const auto ntmp = fq_neg_lazy(tmp.c);
    const auto nz = fq_neg_lazy(zs.c);
#if defined(__HIP_DEVICE_COMPILE__)
    const auto y = fq_bcast_c0(y2);
    const auto ny = fq_neg_lazy(y2);
    Fq<kjoin(decltype(y2)::kK, decltype(ny)::kK)> w;
    dpp_sel_own_partner(w.v, y2.v, ny.v);
#else
    const auto py = fq_partner(y2);
    const auto y = fq_select(odd, py, y2);
    const auto w = fq_pick(odd, y2, fq_neg_lazy(py));
#endif
    return wrap2(fq_dot2_add<10, 1, 1>(s.c, y, ps, w, ntmp, xt, nz));
}
template <int A, int B>
BN_INLINE auto fq2_mul(const Fq2<A>& a_in, const Fq2<B>& b_in) {
    if constexpr (kv(A) > 40 || kv(B) > 40) return fq2_mul(pre<40>(a_in), pre<40>(b_in)); else {
    return fq2_mul_split(a_in, b_in);
    }
}
template <class R, class S>
struct Fq2Pair {
    R a;
    S b;
};
template <int A, int B, int C, int D>
BN_INLINE auto fq2_mul2(const Fq2<A>& a_in, const Fq2<B>& b_in, const Fq2<C>& c_in, const Fq2<D>& d_in) {
    if constexpr (kv(A) > 40 || kv(B) > 40 || kv(C) > 40 || kv(D) > 40) {
        return fq2_mul2(pre<40>(a_in), pre<40>(b_in), pre<40>(c_in), pre<40>(d_in));
    } else {
        auto r = fq2_mul_split(a_in, b_in);
        auto q = fq2_mul_split(c_in, d_in);
        return Fq2Pair<decltype(r), decltype(q)>{r, q};
    }
}

// fq2.rs:105-117: c0 = (a0 - a1)(a0 + a1), c1 = 2*a0*a1 -- one product per lane:
// lane 0: (a0 + K*p - a1) * (a0 + a1), lane 1: a1 * (a0 + a0).  x keeps digits
// below 3*2^29 (no carry pass: fq_mul takes a 3 x 2 digit-bound product).
template <int A>
BN_INLINE auto fq2_sqr(const Fq2<A>& a) {
    if constexpr (kv(A) > 40) return fq2_sqr(fq2_fold(a)); else {
    const bool odd = lane_odd();
    const Fq<kv(A)> own = fq_norm(a.c);
    const Fq<kv(A)> par = fq_partner(own);
    const auto x = fq_pick(odd, own, fq_sub(own, par));
    const auto y = fq_add(par, fq_select(odd, par, own));
    return wrap2(fq_mul(x, y));
    }
}
// ---------------------------------------------------------------- line-step chains
// The forms curve.h's doubling_step and mixed_addition_step run on with BN_LINE_CHAIN:
// differences of products as one column sum with one reduction, and sums of a product and
// stored values through the addend columns.  Each computes the residue of the formula in
// its comment; the integer (a multiple of p apart) and its bound are the chain's.
//
// g^2 - M * e^2 (the doubling step's g^2 - 3 e^2), both squares in fq2_sqr's one-product
// form in ONE column sum:
//   lane 0: (g0 - g1) * (g0 + g1) + (K*p + e1 - e0) * M (e0 + e1)
//   lane 1:  g1 * (g0 + g0)       + (K*p - e1)      * M (e0 + e0)
// The sums y and w are carried (digit bound 1) so that the differences x and z enter with
// fq_sub's digits below 3 * 2^29: column budget 3 + 3.
template <int M, int G, int E>
BN_INLINE auto fq2_sqr_sub_msqr(const Fq2<G>& g_in, const Fq2<E>& e_in) {
    const bool odd = lane_odd();
    const Fq<kv(G)> g = fq_norm(g_in.c), pg = fq_partner(g);
    const Fq<kv(E)> e = fq_norm(e_in.c), pe = fq_partner(e);
    const auto x = fq_pick(odd, g, fq_sub(g, pg));
    const auto y = fq_norm(fq_add(pg, fq_select(odd, pg, g)));
    const auto z = fq_pick(odd, fq_neg_lazy(e), fq_sub(pe, e));
    const auto w = fq_norm(fq_mul_small<M>(fq_add(pe, fq_select(odd, pe, e))));
    return wrap2(fq_dot2(x, y, z, w));
}
// b + c - a^2, normalized: fq2_sqr's product with its first operand negated (lane 0:
// K*p + a1 - a0, lane 1: K*p - a1) and b, c on the addend columns
template <int A, int B, int C>
BN_INLINE auto fq2_nsqr_add(const Fq2<A>& a_in, const Fq2<B>& b, const Fq2<C>& c) {
    const bool odd = lane_odd();
    const Fq<kv(A)> own = fq_norm(a_in.c), par = fq_partner(own);
    const auto x = fq_pick(odd, fq_neg_lazy(own), fq_sub(par, own));
    const auto y = fq_add(par, fq_select(odd, par, own));
    return wrap2(fq_mul_add<1, 1>(x, y, fq_norm(b.c), fq_norm(c.c)));
}
// The second operand b of a two-lane product a * b in the forms the column sum takes it
// in (fq2_mul_split's y and w): own(a) * y + partner(a) * w.
template <int Y, int W>
struct SplitOps {
    Fq<Y> y;  // b0 on both lanes
    Fq<W> w;  // lane 0: K*p - b1, lane 1: b1
};
// w from this lane's coordinate `own` and the value `neg` whose partner copy the even lane takes
template <int O, int N>
BN_INLINE Fq<kjoin(O, N)> split_w(const Fq<O>& own, const Fq<N>& neg) {
    Fq<kjoin(O, N)> w;
#if defined(__HIP_DEVICE_COMPILE__)
    dpp_sel_own_partner(w.v, own.v, neg.v);
#else
    w = fq_pick(lane_odd(), own, fq_partner(neg));
#endif
    return w;
}
// the forms of +b (NW: w carried to digit bound 1, for a sum with no column budget left)
template <bool NW = false, int B>
BN_INLINE auto split_ops(const Fq2<B>& b) {
    static_assert(kl(B) == 1, "split_ops: normalized operand");
    const auto w = split_w(b.c, fq_neg_lazy(b.c));
    if constexpr (NW) {
        return SplitOps<B, kv(decltype(w)::kK)>{fq_bcast_c0(b.c), fq_norm(w)};
    } else {
        return SplitOps<B, decltype(w)::kK>{fq_bcast_c0(b.c), w};
    }
}
// the forms of -b from b: y = K*p - b0, w = lane 0: b1, lane 1: K*p - b1 -- the same
// operand work as for +b
template <int B>
BN_INLINE auto split_ops_neg(const Fq2<B>& b) {
    static_assert(kl(B) == 1, "split_ops_neg: normalized operand");
    const auto hb = fq_neg_lazy(b.c);  // this lane's coordinate of -b
    const auto w = split_w(hb, b.c);
    return SplitOps<decltype(hb)::kK, decltype(w)::kK>{fq_bcast_c0(hb), w};
}
// a * (-nb), the product by a value held as its negation nb
template <int A, int NB>
BN_INLINE auto fq2_mul_negb(const Fq2<A>& a, const Fq2<NB>& nb) {
    static_assert(kl(A) == 1, "fq2_mul_negb: normalized operand");
    const auto o = split_ops_neg(nb);
    return wrap2(fq_dot2(a.c, o.y, fq_partner(a.c), o.w));
}
// a * b + K0 * c0 [+ K1 * c1] with the c_j on the addend columns (normalized result)
template <int K0, int A, int B, int C0>
BN_INLINE auto fq2_mul_add(const Fq2<A>& a, const Fq2<B>& b, const Fq2<C0>& c0) {
    static_assert(kl(A) == 1, "fq2_mul_add: normalized operand");
    const auto o = split_ops(b);
    return wrap2(fq_dot2_add<K0>(a.c, o.y, fq_partner(a.c), o.w, c0.c));
}
template <int K0, int K1, int A, int B, int C0, int C1>
BN_INLINE auto fq2_mul_add(const Fq2<A>& a, const Fq2<B>& b, const Fq2<C0>& c0, const Fq2<C1>& c1) {
    static_assert(kl(A) == 1, "fq2_mul_add: normalized operand");
    const auto o = split_ops(b);
    return wrap2(fq_dot2_add<K0, K1>(a.c, o.y, fq_partner(a.c), o.w, c0.c, c1.c));
}
// a * b + c * d and a * b - c * d as one four-product column sum, reduced once.  In the
// difference b's w is carried: the forms of -d take digit bound 2 on both sides
// (column budget 1 + 1 + 2 + 2).
template <int A, int B, int C, int D>
BN_INLINE auto fq2_dot_pp(const Fq2<A>& a, const Fq2<B>& b, const Fq2<C>& c, const Fq2<D>& d) {
    static_assert(kl(A) == 1 && kl(C) == 1, "fq2_dot_pp: normalized operands");
    const auto ob = split_ops(b);
    const auto od = split_ops(d);
    return wrap2(fq_dot4(a.c, ob.y, fq_partner(a.c), ob.w, c.c, od.y, fq_partner(c.c), od.w));
}
template <int A, int B, int C, int D>
BN_INLINE auto fq2_dot_pm(const Fq2<A>& a, const Fq2<B>& b, const Fq2<C>& c, const Fq2<D>& d) {
    static_assert(kl(A) == 1 && kl(C) == 1, "fq2_dot_pm: normalized operands");
    const auto ob = split_ops<true>(b);
    const auto od = split_ops_neg(d);
    return wrap2(fq_dot4(a.c, ob.y, fq_partner(a.c), ob.w, c.c, od.y, fq_partner(c.c), od.w));
}

// x * xi, xi = 9 + u (fq2.rs:19-34, 55-57): lane 0: 9a0 - a1, lane 1: 9a1 + a0.
template <int A>
BN_INLINE auto fq2_mul_xi(const Fq2<A>& a) {
    if constexpr (kv(A) > 8) {
        return fq2_mul_xi(fq2_fold(a));
    } else {
        const Fq<kv(A)> own = fq_norm(a.c);
        const auto own9 = fq_add(fq_mul_small<8>(own), own);
        const Fq<kv(A)> par = fq_partner(own);
        return wrap2(fq_add(own9, fq_pick(lane_odd(), par, fq_neg_lazy(par))));
    }
}
// fq2.rs:59-68: odd powers conjugate: lane 1 negates (c1 * (p-1) == -c1)
template <int B>
BN_INLINE auto fq2_conj(const Fq2<B>& a) {
    const Fq<kv(B)> own = fq_norm(a.c);
    return wrap2(fq_select(lane_odd(), fq_neg(own), own));
}
// fq2.rs:119-130: t = (c0^2 + c1^2)^-1 on both lanes, then (c0 t, -c1 t); Quad: both
// lane pairs of every quad hold the same element (fq_inv_quad)
template <bool Quad = false, int B>
BN_INLINE auto fq2_inv(const Fq2<B>& a_in) {
    auto a = pre<40>(a_in);
    const auto sq = fq_sqr(a.c);
    const auto t = fq_inv<Quad>(fq_add(sq, fq_partner(sq)));  // the same norm on both lanes
    const auto r = fq_mul(a.c, t);
    return wrap2(fq_select(lane_odd(), fq_neg(r), r));
}
