// products_prepared_emul.cpp -- TEST INFRASTRUCTURE: the data path of
// bn_pairing_batch_prepared_many for ONE product, compiled for the host CPU in the one-lane
// layout: a fresh term's lines are g2_precompute's scaled by the affine P as the producers store
// them; a prepared term's are the unscaled lines of its table point (given by the caller) taken through
// prepared_line_scaled with s0 = Z^3, sy = Y, sx = X Z of the Jacobian P (what k_prepared_expand
// writes); the terms are looked up through a map word per term (bit 31: prepared region, low
// bits: the slot) and multiplied in by miller_product_scaled (the loop body of
// k_miller_products_mapped).  tests/test_pairing_products_prepared_emul.py compares the values
// with the oracle's without a GPU.  Nothing in the product links this.
#include <stdint.h>

#include <vector>

#include "../../paritytech-bn_amd/csrc/pairing.h"

using namespace bn;

static Fq<2> ld(const uint32_t* w) { return fq_load_ref(w); }
static Fq2<2> ld2(const uint32_t* w) { return {ld(w), ld(w + 8)}; }
template <int B>
static void st12(const Fq12<B>& a, uint32_t* w) {
    const Fq2<B>* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    for (int k = 0; k < 6; ++k) {
        fq_store_ref(c[k]->c0, w + 16 * k);
        fq_store_ref(c[k]->c1, w + 16 * k + 8);
    }
}

extern "C" {
// fresh: nf pairs, 48 words each (affine P.x, P.y: 8 words each; affine Q.x, Q.y: 16 each).
// table: the reference's coefficients of nq prepared points (87 x (ell_0, ell_vw, ell_vv), 16
// words each: what bn_g2_precompute_many exports and a bn_g2_prepared table holds).
// pp: np Jacobian G1 points (x, y, z: 8 words each) and pidx: their table indices -- the
// prepared slots.  map: k_terms words in term order.  dead[t] != 0 gives term t the line one
// (the kernel's flag); the loop iterates to k_iter >= k_terms terms, those past k_terms taking
// the line one.  out: the Miller value (96 words).  Returns the number of lines fetched by the
// loop, or -1 for a map word outside its region.
int ppe_miller_product(const uint32_t* fresh, int nf, const uint32_t* table, int nq, const uint32_t* pp,
                       const uint32_t* pidx, int np, const uint32_t* map, int k_terms, const uint8_t* dead,
                       int k_iter, uint32_t* out) {
    std::vector<Ell> region_a((size_t)nf * BN_NUM_COEFFS), region_b((size_t)np * BN_NUM_COEFFS);
    for (int t = 0; t < nf; ++t) {
        const uint32_t* w = fresh + (size_t)t * 48;
        const Fq<2> px = ld(w), py = ld(w + 8);
        const G2Aff<2> qa = {ld2(w + 16), ld2(w + 32)};
        g2_precompute(qa, [&](int k, const Ell& e) {
            region_a[(size_t)t * BN_NUM_COEFFS + k] = {e.ell_0, narrow<kLine>(fq2_scale(e.ell_vw, py)),
                                                       narrow<kLine>(fq2_scale(e.ell_vv, px))};
        });
    }
    std::vector<Ell> rows((size_t)nq * BN_NUM_COEFFS);  // the table: unscaled lines
    for (size_t r = 0; r < rows.size(); ++r) {
        const uint32_t* w = table + r * 48;
        rows[r] = {widen<kLine>(ld2(w)), widen<kLine>(ld2(w + 16)), widen<kLine>(ld2(w + 32))};
    }
    for (int s = 0; s < np; ++s) {  // k_prepared_expand
        if ((int)pidx[s] >= nq) return -1;
        const uint32_t* w = pp + (size_t)s * 24;
        const Fq<2> x = ld(w), y = ld(w + 8), z = ld(w + 16);
        const auto s0 = fq_mul(fq_sqr(z), z), sx = fq_mul(x, z);
        for (int k = 0; k < BN_NUM_COEFFS; ++k)
            region_b[(size_t)s * BN_NUM_COEFFS + k] =
                prepared_line_scaled(rows[(size_t)pidx[s] * BN_NUM_COEFFS + k], s0, y, sx);
    }
    for (int t = 0; t < k_terms; ++t) {
        const int slot = (int)(map[t] & 0x7fffffffu);
        if (slot >= ((map[t] >> 31) ? np : nf)) return -1;
    }
    const Ell one_line = {widen<kLine>(fq2_one()), widen<kLine>(fq2_zero()), widen<kLine>(fq2_zero())};
    int fetched = 0;
    const Fq12<kF> f = miller_product_scaled(k_iter, [&](int t, int k) {
        ++fetched;
        if (t >= k_terms || dead[t]) return one_line;
        const size_t slot = map[t] & 0x7fffffffu;
        return ((map[t] >> 31) ? region_b : region_a)[slot * BN_NUM_COEFFS + k];
    });
    st12(f, out);
    return fetched;
}
}
