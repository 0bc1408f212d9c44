// msm_basis.h -- one large multi-scalar multiplication over a FIXED BASIS (bn_g1_basis,
// bn_g1_msm_basis, bn_g2_basis, bn_g2_msm_basis): the bodies shared by
// kernels_msm_basis.hip, kernels_msm_basis_g2.hip and the host builds of
// tests/native/msm_basis_emul.cpp and msm_basis_g2_emul.cpp, templates over the field F
// through curve.h's F_* (Fq: G1; Fq2: G2) that take functors for every load and store.
//
// The scalars are recoded exactly as for the bucket method (msm.h: W(c) signed digits of c
// bits, the keys msm_key(c, w, d, index), the top window's replicas, the run split).  The
// table holds, for every base b and window w, the one affine point
//     entry (b, w) = 2^(c*w) * bases[b]
// so that a digit d of window w is the addition of sign(d) * entry (b, w) into bucket |d|,
// and that bucket weighs |d| whatever the window: the buckets of the windows below the top
// one are added row-wise (the top window's slots are replicas, msm.h, and keep their own
// weights), two windows are reduced, and nothing is doubled after the table is built.
//
// Layout: window-major, entry (b, w) at index w * nbases + b, 64 bytes (x, y as reference
// images) in an allocation aligned to more than that, so an entry is one aligned 64-byte
// read.  The accumulation's gather is random in b whichever way the table is laid out (the
// entries of a bucket are whatever terms drew that digit); window-major makes the build's
// stores of neighbouring lanes contiguous, and keeps the entries a prefix call of n < nbases
// terms can touch in W(c) dense ranges of n entries.  A base with z == 0 has a zero flag and
// all-zero entries, which are never added.
//
// G2 (F = Fq2): the same index, 128 bytes per entry, stored as the two halves a lane pair
// reads, [x.c0, y.c0 | x.c1, y.c1], so each lane's gather is again one aligned 64-byte read
// (kernels_msm_basis_g2.hip).  A base may be any point of the twist, also one outside the
// order-r subgroup, as everywhere in the G2 group API: the order of E'(Fq2) is r * (2p - r),
// which is odd, so no point has even order, no doubling of the build turns a nonzero base
// into zero, and every entry of an unflagged base is a real affine point.
#pragma once
#include "msm_fixed.h"

namespace bn {

constexpr uint64_t kMsmBasisMaxBases = 1ull << 26;  // the entry index keeps bit 31 for the sign (msm.h)
// entry indices, and the n * W(c) sorted positions of a call, are 32-bit
constexpr uint64_t kMsmBasisMaxEntries = 0x7fffffffull;

// The window width bn_g1_basis_prepare takes for c = 0, from the number of bases (a call
// usually runs over all of them): the fastest width of the measured sweep over 9 .. 16 at
// the nearest measured size (profiles/msm_basis_widths.jsonl, tools/msm_bench.py --basis
// --basis-windows), the steps at the geometric means between measured sizes
// whose best width differs.  It follows bn_g1_msm's table but for 11 at 2^12 and 14 still at
// 2^19; 15 and 16 tie at 2^20, 14 and 15 at 2^19, 12 to 14 at 2^17.
BN_INLINE int msm_basis_auto_window(uint64_t nbases) {
    if (nbases < 2048) return 10;    // 2^11
    if (nbases < 8192) return 11;    // 2^13
    if (nbases < 92682) return 12;   // 2^16.5
    if (nbases < 741455) return 14;  // 2^19.5
    return 16;
}
// The width bn_g2_basis_prepare takes for c = 0: the table of the G2 basis form's own width
// sweep over 9 .. 16 (profiles/msm_basis_g2_widths.jsonl, tools/msm_bench.py --basis --group g2
// --basis-windows), the steps at the geometric means between measured sizes
// whose best width differs (measured at 1, 2^10, 2^12, 2^14 and 2^16 .. 2^20 bases).  It is
// narrower than bn_g2_msm's table at both ends: 9 up to 2^10 (the buckets written, collapsed
// and reduced whatever n is are the floor), 14 still at 2^19 and 15 at 2^20, where 16 is 0.19 ms
// behind.
BN_INLINE int msm_basis_auto_window_g2(uint64_t nbases) {
    if (nbases < 2048) return 9;     // 2^11
    if (nbases < 32768) return 11;   // 2^15
    if (nbases < 92682) return 12;   // 2^16.5
    if (nbases < 741455) return 14;  // 2^19.5
    return 15;
}
// entries of the table of nbases bases at the width c itself, which no default stands in for
// (the library resolves a group's default before it asks: capi_msm.hip MsmBasis<P>); 0 for an
// nbases or c that the prepare call refuses, c == 0 among them
BN_INLINE uint64_t msm_basis_entries_at(uint64_t nbases, int c) {
    if (nbases < 1 || nbases > kMsmBasisMaxBases) return 0;
    if (!msm_window_ok(c)) return 0;
    const uint64_t nwin = (uint64_t)msm_windows(c);
    if (nbases > kMsmBasisMaxEntries / nwin) return 0;
    return nbases * nwin;
}
// the same with c == 0 taken as the G1 default: the G1 emulator's form (tests/native); the
// library calls msm_basis_entries_at
BN_INLINE uint64_t msm_basis_entries(uint64_t nbases, int c) {
    return msm_basis_entries_at(nbases, c ? c : msm_basis_auto_window(nbases));
}
// index of entry (b, w)
BN_INLINE uint32_t msm_basis_index(uint32_t nbases, uint32_t b, uint32_t w) { return w * nbases + b; }

// One lane of the table build: the W(c) entries of one base, entry w stored normalized by
// store(w, x, y).  c doublings and a normalization per window; the next window starts from
// the normalized point (the same point, a cheaper image).  The base is not zero.
template <template <int> class F, class Store>
BN_INLINE void msm_basis_build(const Jac<F>& base, int c, Store&& store) {
    const int nwin = msm_windows(c);
    Jac<F> p = jac_normalize(base);
    for (int w = 0; w < nwin; ++w) {
        if (w) {
            for (int i = 0; i < c; ++i) p = jac_double(p);
            p = jac_normalize(p);
        }
        store((uint32_t)w, p.x, p.y);
    }
}

// The sum of the sorted entries [lo, hi) of one key of window w (a whole run, or one chunk of
// an overlong one): each entry's table point with the digit's sign applied to y, by mixed
// additions (msm_fixed.h msm_fixed_add: jac_add_mixed's shortcuts make duplicates and B, -B
// in one bucket come out right).  word(e) loads sorted entry e in [lo, hi); fetch(idx) loads
// the table point of base idx < n in this window; decode turns it into coordinates.  The
// next entry's word and point are loaded before the current addition is issued, so the
// gather's latency runs under the addition; an index out of range adds nothing and loads
// base 0's point, and so does the step past the run's end.  An empty run is zero.
template <template <int> class F, class Word, class Fetch, class Decode>
BN_INLINE Jac<F> msm_basis_run_sum(Word&& word, Fetch&& fetch, Decode&& decode, uint32_t n, uint32_t lo, uint32_t hi) {
    Jac<F> acc = jac_zero<F>();
    uint32_t e = lo;
    uint32_t ent = e < hi ? word(e) : 0u;
    bool pending = e < hi && msm_entry_index(ent) < n;
    bool pneg = msm_entry_neg(ent);
    auto cur = fetch(pending ? msm_entry_index(ent) : 0u);
    while (e < hi) {
        ++e;
        const bool more = e < hi;
        ent = more ? word(e) : 0u;
        const bool take = more && msm_entry_index(ent) < n;
        const auto next = fetch(take ? msm_entry_index(ent) : 0u);
        if (BN_ANY(pending)) acc = msm_fixed_add(acc, cur, pneg, pending, decode);
        cur = next;
        pending = take;
        pneg = msm_entry_neg(ent);
    }
    return acc;
}

// the two windows that are reduced after the collapse: the collapsed row (window 0's slots,
// weights j + 1) and the top window (its replica weights)
BN_INLINE uint32_t msm_basis_reduce_window(int c, uint32_t which) { return which ? (uint32_t)msm_windows(c) - 1u : 0u; }

}  // namespace bn
