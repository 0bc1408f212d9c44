// scaled_emul.cpp -- TEST INFRASTRUCTURE: the pairing on scaled inputs (pairing.h
// scaled_inputs -> miller_fused with the per-pairing curve constant -> the final
// exponentiation) compiled for the host CPU from the engine's device headers, so
// tests/test_scaled_inputs_model.py can compare the exact formulas k_pairing_full runs
// with the oracle's pairing without a GPU.  Nothing in the product links this.
#include <stdint.h>

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
static bool words_zero(const uint32_t* w, int n) {
    uint32_t o = 0;
    for (int i = 0; i < n; ++i) o |= w[i];
    return o == 0;
}

extern "C" {
// p: a Jacobian G1 point (x, y, z: 24 words), q: a Jacobian G2 point (x, y, z: 48 words),
// both as reference memory images -> the Gt image (96 words).  Returns 1 when a zero
// point made the pairing one (the kernel's `skip`), else 0.
int se_pairing_scaled(const uint32_t* p, const uint32_t* q, uint32_t* out) {
    // as k_pairing_full: the prologue and the loop run on a zero point's values too (every
    // scaled coordinate is then zero), and the Miller value is replaced by one after them
    const bool skip = words_zero(p + 16, 8) || words_zero(q + 32, 16);
    const ScaledPair a = scaled_inputs(ld(p), ld(p + 8), ld(p + 16), ld2(q), ld2(q + 16), ld2(q + 32));
    Fq12<kF> f = miller_fused(a.qa, a.px, a.py, a.coeff);
    if (skip) f = widen<kF>(fq12_one());
    st12(fe_last_chunk(fe_first_chunk(f)), out);
    return skip ? 1 : 0;
}
}
