// kernels_prepared.hip -- pairings against prepared G2 points (bn_g2_prepared; G2Precomp,
// mod.rs:566-607): the table's fill and the throughput kernel that reads it.
// Pairing-path layout (two lanes per pairing, fq2_split.h; `n` counts
// pairings, the grid has kPathLanes threads per pairing).  G1 values are held by both lanes.
// Built as kernels_pairing.hip is: the same BN_FOLD_LDS / BN_FQ6_LAZY / BN_CYC_LIN, so the
// Fq12 product, square and cyclotomic square of the final exponentiation here are the
// ones k_pairing_full runs and k_fq12_vm_pairing checks (tests/test_gpu_fq6_lazy.py).
// Keep the three defaults below equal to that unit's.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#ifndef BN_FQ6_LAZY
#define BN_FQ6_LAZY 3
#endif
#ifndef BN_CYC_LIN
#if BN_FQ6_LAZY == 3
#define BN_CYC_LIN 7
#else
#define BN_CYC_LIN 0
#endif
#endif
#include "fq.h"
#define BN_SPLIT 1
#include "kernels.h"
#include "lines_wide.h"
#include "fe_vm.h"

namespace bn {

__global__ void __launch_bounds__(kBlock) k_g1_fill_one(bn_g1* __restrict__ out, size_t n) {
    const size_t i = lane_id();
    if (i >= n) return;
    // Fq::one() = R mod p and 2 R mod p (G1::one() = (1, 2, 1), mod.rs:381-392)
    const uint32_t one[8] = {0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u,
                             0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};
    const uint32_t two[8] = {0x8b1e1b3au, 0xa6ba871bu, 0xeb8e167bu, 0x14f1d651u,
                             0xf0f28c58u, 0xccdd46deu, 0x340fbe5eu, 0x1c14ef83u};
    st_words(&out[i].x, one);
    st_words(&out[i].y, two);
    st_words(&out[i].z, one);
}

// Lane 2j + c of the fill's pair j holds coordinate c of its 87 x 3 coefficients in the
// lane-strided workspace; it writes them as the table's contiguous 9-digit runs.
__global__ void __launch_bounds__(kBlock) k_prepared_repack(const uint32_t* __restrict__ coeffs,
                                                            const uint8_t* __restrict__ flags, size_t m,
                                                            uint32_t* __restrict__ table, uint8_t* __restrict__ zero) {
    const size_t l = lane_id(), j = l / kL, c = l % kL, nl = kL * m;
    if (j >= m) return;
    if (c == 0) zero[j] = flags[l];  // the G1 side is G1::one(): the flag is "q[j] is zero"
    uint32_t* row = table + j * (size_t)kPreparedWords + c * 9;
#pragma unroll 1
    for (int k = 0; k < BN_NUM_COEFFS; ++k)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const Fq2<kLine> x = ld_fq2<kLine>(coeffs, nl, l, k * 6 + 2 * e);
#pragma unroll
            for (int w = 0; w < 9; ++w) row[k * kPreparedLineWords + e * 18 + w] = x.c.v[w];
        }
}

// this lane's coordinate of one Fq2 of the table: nine contiguous digits
__device__ __forceinline__ Fq2<kLine> ld_prepared(const uint32_t* __restrict__ w) {
    Fq2<kLine> x;
#pragma unroll
    for (int d = 0; d < 9; ++d) x.c.v[d] = w[d];
    return x;
}

// One pairing per lane pair against point qidx[i] of the table: the launch shape of
// k_pairing_full (kPairBlock threads, two waves per SIMD, issue balance per digit) without
// the line steps -- the running G2 point, its base and the curve constant are not held.
// Each line is loaded right before the loop multiplies by it (pairing.h miller_prepared).
// FinalExp: Gt form (P's Jacobian coordinates as they are: s0 = Z^3, sy = Y, sx = X Z, no
// inversion), then k_pairing_full's tail: the Miller value to slot 0, the step program,
// the Gt image out.  Otherwise the Miller form: a G1-only to_affine (mod.rs:199-216; when
// every P of the wave has z == one its inverse is one and no inversion runs, as
// pair_to_affine) and the Miller value out -- G2Precomp::miller_loop's.
// A zero P or a zero table point (qzero) gives one.  An index >= nq is clamped to 0 before
// any address is formed; its row is the zero image and BN_ERR_INVALID_ARGUMENT is set.
template <bool FinalExp>
__global__ void BN_PATH_ATTR __launch_bounds__(kPairBlock)
k_pairing_prepared(const bn_g1* __restrict__ p, const uint32_t* __restrict__ table, const uint8_t* __restrict__ qzero,
                   uint32_t nq, const uint32_t* __restrict__ qidx, size_t n, const uint32_t* __restrict__ prog,
                   int nsteps, uint32_t* __restrict__ slots, bn_gt* __restrict__ out, int* __restrict__ err) {
    fold_table_init();
    const Balance bal = balance_init();
    const size_t l = lane_id(), i = l / kL, nl = kL * n;
    if (i >= n) return;
    const uint32_t jr = qidx ? qidx[i] : 0u;
    const bool bad = jr >= nq;
    const uint32_t j = bad ? 0u : jr;
    const uint32_t* row = table + (size_t)j * kPreparedWords + (l % kL) * 9;
    auto line = [&](int k) {
        mem_fence();  // load right before use: the 87 lines are never held at once
        const uint32_t* w = row + k * kPreparedLineWords;
        return Ell{ld_prepared(w), ld_prepared(w + 18), ld_prepared(w + 36)};
    };
    auto step = [&](int d) { balance_step(bal, (uint32_t)d); };

    uint32_t wz[8];
    ld_words(&p[i].z, wz);
    const bool skip = words_zero(wz) || qzero[j] != 0 || bad;
    const Fq<2> pz = fq_load_ref(wz), px = ld_ref(p[i].x), py = ld_ref(p[i].y);
    if constexpr (FinalExp) {
        Fq12<kF> f = miller_prepared(line, fq_mul(fq_sqr(pz), pz), py, fq_mul(px, pz), step);
        if (skip) f = widen<kF>(fq12_one());
        // f == 0: the reference's final_exponentiation returns None and pairing() panics
        // (fq12.rs:63-72) -> zero Gt and the error bit, as k_pairing_full
        const bool zero = !skip && fq12_is_zero(f);
        st_fq12(slots, nl, l, f);
        const Fq12<kF> r = fq12_vm_run(prog, nsteps, slots, nl, l, bal, 1u << 20, false);
        if (bad) {
            if ((l % kL) == 0) err_or(err, BN_ERR_INVALID_ARGUMENT);
            st_gt_zero(out[i]);
        } else if (zero) {
            if ((l % kL) == 0) err_or(err, BN_ERR_FE_ZERO);
            st_gt_zero(out[i]);
        } else if (skip) {
            st_gt(out[i], fq12_one());
        } else {
            st_gt(out[i], r);
        }
    } else {
        Fq<2> t;
        if (BN_ALL(words_one(wz)))  // wave-uniform
            t = widen<2>(fq_one());
        else
            t = fq_inv(pz);
        const auto t2 = fq_sqr(t);
        Fq12<kF> f = miller_prepared(line, NoScale{}, fq_mul(py, fq_mul(t2, t)), fq_mul(px, t2), step);
        if (skip) f = widen<kF>(fq12_one());
        if (bad) {
            if ((l % kL) == 0) err_or(err, BN_ERR_INVALID_ARGUMENT);
            st_gt_zero(out[i]);
        } else {
            st_gt(out[i], f);
        }
    }
}

// The prepared terms of a launch set of bn_pairing_batch_prepared_many: prepared slot s < np is
// term pterm[s] of p against point pidx[s] of the table; its 87 lines are written as the
// products' loop multiplies by them (pairing.h prepared_line_scaled in k_pairing_prepared's Gt
// form: ell_0 Z^3, ell_vw Y, ell_vv X Z of the Jacobian P, no inversion) into `coeffs` in the
// producers' lane-strided layout (lane stride kL * np), and the term's flag (P zero or table
// point zero) into flags[kL * s + c].  The host has checked every index; one >= nq is still
// clamped before any address is formed.
// kExpandSplit lane pairs share a term: lane pair g = r * np + s takes lines r, r + 29, r + 58
// (a wave's lane pairs are neighbouring slots at one r, so the stores stay coalesced) and forms
// Z^3 and X Z itself.  With one lane pair per term the kernel was a chain of 87 load - scale -
// store rounds, 0.245 ms at 3,072 terms where the GPU is nearly empty.
// Loads and stores bound it, not issue: no two-waves-per-SIMD attribute, so its 71 VGPRs let
// two blocks share a CU.
constexpr int kExpandSplit = 29;
static_assert(BN_NUM_COEFFS % kExpandSplit == 0, "k_prepared_expand: every lane pair the same number of lines");
__global__ void __launch_bounds__(kPairBlock)
k_prepared_expand(const bn_g1* __restrict__ p, const uint32_t* __restrict__ pterm, const uint32_t* __restrict__ pidx,
                  const uint32_t* __restrict__ table, const uint8_t* __restrict__ qzero, uint32_t nq, size_t np,
                  uint32_t* __restrict__ coeffs, uint8_t* __restrict__ flags) {
    fold_table_init();
    const size_t l = lane_id(), g = l / kL, nl = kL * np;
    if (g >= np * kExpandSplit) return;
    const size_t s = g % np, ls = s * kL + l % kL;  // the slot, and this lane's place in its arrays
    const int r = (int)(g / np);
    const uint32_t jr = pidx[s], j = jr < nq ? jr : 0u;
    const uint32_t* row = table + (size_t)j * kPreparedWords + (l % kL) * 9;
    const bn_g1& pt = p[pterm[s]];
    uint32_t wz[8];
    ld_words(&pt.z, wz);
    if (r == 0) flags[ls] = words_zero(wz) || qzero[j] != 0 || jr >= nq ? 1 : 0;
    const Fq<2> pz = fq_load_ref(wz), px = ld_ref(pt.x), py = ld_ref(pt.y);
    const auto s0 = fq_mul(fq_sqr(pz), pz), sx = fq_mul(px, pz);
#pragma unroll
    for (int i = 0; i < BN_NUM_COEFFS / kExpandSplit; ++i) {
        const int k = r + i * kExpandSplit;
        const uint32_t* w = row + k * kPreparedLineWords;
        const Ell e = prepared_line_scaled(Ell{ld_prepared(w), ld_prepared(w + 18), ld_prepared(w + 36)}, s0, py, sx);
        st_fq2(coeffs, nl, ls, k * 6 + 0, e.ell_0);
        st_fq2(coeffs, nl, ls, k * 6 + 2, e.ell_vw);
        st_fq2(coeffs, nl, ls, k * 6 + 4, e.ell_vv);
    }
}

// out[i] = p[term[i]], i < n: the G1 points of a launch set's fresh terms, contiguous, for the
// producers (bn_pairing_batch_prepared_many_dev; the host form compacts while it stages).
// One thread per 16-byte sixth of a point.
__global__ void __launch_bounds__(kBlock) k_g1_gather(const bn_g1* __restrict__ p, const uint32_t* __restrict__ term,
                                                      size_t n, bn_g1* __restrict__ out) {
    constexpr size_t kParts = sizeof(bn_g1) / sizeof(uint4);
    const size_t t = lane_id(), i = t / kParts, part = t % kParts;
    if (i >= n) return;
    reinterpret_cast<uint4*>(out + i)[part] = reinterpret_cast<const uint4*>(p + term[i])[part];
}

// out[t] = the G2 point of term t < n of a wide launch set (bn_pairing_batch_prepared_many's wide
// path), for k_pairing_latency: fresh point map[t] of the set's nf at q, or,
// with kMapRegionB set, point map[t] & 0x7fffffff of the handle's nq at hq.  One thread per
// 16-byte twelfth of a point.  The host has checked every index; a table index >= nq is still
// clamped to 0 and a fresh index >= nf gives the zero image, before any address is formed.
__global__ void __launch_bounds__(kBlock) k_g2_gather(const bn_g2* __restrict__ q, size_t nf,
                                                      const bn_g2* __restrict__ hq, uint32_t nq,
                                                      const uint32_t* __restrict__ map, size_t n,
                                                      bn_g2* __restrict__ out) {
    constexpr size_t kParts = sizeof(bn_g2) / sizeof(uint4);
    const size_t t = lane_id(), i = t / kParts, part = t % kParts;
    if (i >= n) return;
    const uint32_t w = map[i], k = w & ~kMapRegionB;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (w & kMapRegionB)
        v = reinterpret_cast<const uint4*>(hq + (k < nq ? k : 0u))[part];
    else if (k < nf)
        v = reinterpret_cast<const uint4*>(q + k)[part];
    reinterpret_cast<uint4*>(out + i)[part] = v;
}

void launch_prepared_expand(const bn_g1* p, const uint32_t* pterm, const uint32_t* pidx, const uint32_t* table,
                            const uint8_t* qzero, uint32_t nq, size_t np, uint32_t* coeffs, uint8_t* flags,
                            hipStream_t s) {
    k_prepared_expand<<<grid_pair(kPathLanes * np * kExpandSplit), kPairBlock, 0, s>>>(p, pterm, pidx, table, qzero, nq,
                                                                                       np, coeffs, flags);
}
void launch_g1_gather(const bn_g1* p, const uint32_t* term, size_t n, bn_g1* out, hipStream_t s) {
    k_g1_gather<<<grid_for(n * (sizeof(bn_g1) / sizeof(uint4))), kBlock, 0, s>>>(p, term, n, out);
}
void launch_g2_gather(const bn_g2* q, size_t nf, const bn_g2* hq, uint32_t nq, const uint32_t* map, size_t n,
                      bn_g2* out, hipStream_t s) {
    k_g2_gather<<<grid_for(n * (sizeof(bn_g2) / sizeof(uint4))), kBlock, 0, s>>>(q, nf, hq, nq, map, n, out);
}

void launch_pairing_prepared(bool final_exp, const bn_g1* p, const uint32_t* table, const uint8_t* qzero, uint32_t nq,
                             const uint32_t* qidx, size_t n, const uint32_t* prog, int nsteps, uint32_t* slots,
                             bn_gt* out, int* err, hipStream_t s) {
    const unsigned grid = grid_pair(kPathLanes * n);
    if (final_exp)
        k_pairing_prepared<true><<<grid, kPairBlock, 0, s>>>(p, table, qzero, nq, qidx, n, prog, nsteps, slots, out, err);
    else
        k_pairing_prepared<false><<<grid, kPairBlock, 0, s>>>(p, table, qzero, nq, qidx, n, prog, nsteps, slots, out, err);
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(prepared)
