// prepared_emul.cpp -- TEST INFRASTRUCTURE: the loop body of k_pairing_prepared (pairing.h
// miller_prepared) compiled for the host CPU in the one-lane layout, over the unscaled lines
// of g2_precompute of an affine Q (what a bn_g2_prepared table holds), in both forms.
// tests/test_prepared_emul.py compares the values with the oracle's without a GPU.
// Nothing in the product links this.
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
// q: an affine G2 point (x, y: 16 words each), p: a G1 point (x, y, z: 8 words each), reference
// images.  gt_form == 0, the Miller form: (p.x, p.y) are taken as the affine coordinates (z is
// not read) and ell_0 is applied as stored.  gt_form != 0, the Gt form: p is Jacobian and the
// lines are scaled by s0 = Z^3, sy = Y, sx = X Z, as the kernel does before a final
// exponentiation.  out: the Miller value (96 words).  Returns the number of lines fetched.
int pp_miller_prepared(const uint32_t* q, const uint32_t* p, int gt_form, uint32_t* out) {
    std::vector<Ell> lines(BN_NUM_COEFFS);
    const G2Aff<2> qa = {ld2(q), ld2(q + 16)};
    g2_precompute(qa, [&](int k, const Ell& e) { lines[k] = e; });
    int fetched = 0;
    auto line = [&](int k) {
        ++fetched;
        return lines[k];
    };
    const Fq<2> x = ld(p), y = ld(p + 8), z = ld(p + 16);
    Fq12<kF> f;
    if (gt_form)
        f = miller_prepared(line, fq_mul(fq_sqr(z), z), y, fq_mul(x, z));
    else
        f = miller_prepared(line, NoScale{}, y, x);
    st12(f, out);
    return fetched;
}
}
