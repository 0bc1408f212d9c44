// products_emul.cpp -- TEST INFRASTRUCTURE: the loop body of k_miller_products
// (pairing.h miller_product_scaled: one squaring per digit, then the line of each of the
// product's pairs) compiled for the host CPU in the one-lane layout, over lines from
// g2_precompute scaled by P as the producers store them (ell_0, ell_vw * Py, ell_vv * Px).
// tests/test_pairing_products_emul.py compares its Miller value with the oracle's
// miller_loop_batch without a GPU.  Nothing in the product links this.
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
// pairs: k_pairs affine pairs, 48 words each (P.x, P.y: 8 words each; Q.x, Q.y: 16 words
// each), reference images.  dead[t] != 0 gives pair t the line one, as the kernel does for
// a pair whose flag is set.  The loop iterates to k_iter >= k_pairs pairs: those past
// k_pairs take the line one (the kernel's padding to the wave's largest product).
// out: the Miller value (96 words).  Returns the number of lines fetched.
int pe_miller_product(const uint32_t* pairs, int k_pairs, const uint8_t* dead, int k_iter, uint32_t* out) {
    std::vector<Ell> lines((size_t)k_pairs * BN_NUM_COEFFS);
    for (int t = 0; t < k_pairs; ++t) {
        const uint32_t* w = pairs + (size_t)t * 48;
        const Fq<2> px = ld(w), py = ld(w + 8);
        const G2Aff<2> qa = {ld2(w + 16), ld2(w + 32)};
        g2_precompute(qa, [&](int k, const Ell& e) {
            lines[(size_t)t * BN_NUM_COEFFS + k] = {e.ell_0, narrow<kLine>(fq2_scale(e.ell_vw, py)),
                                                    narrow<kLine>(fq2_scale(e.ell_vv, px))};
        });
    }
    const Ell one_line = {widen<kLine>(fq2_one()), widen<kLine>(fq2_zero()), widen<kLine>(fq2_zero())};
    int fetched = 0;
    const Fq12<kF> f = miller_product_scaled(k_iter, [&](int t, int k) {
        ++fetched;
        return t < k_pairs && !dead[t] ? lines[(size_t)t * BN_NUM_COEFFS + k] : one_line;
    });
    st12(f, out);
    return fetched;
}
}
