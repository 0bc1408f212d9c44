// msm_many_emul.cpp -- TEST INFRASTRUCTURE (tests/test_msm_many_emul.py): the bodies of
// csrc/msm_many.h compiled for the host over Fq and the plan of csrc/msm_many_plan.h, and
// the whole bn_g1_msm_many pipeline around them in plain loops -- per launch set the table
// "kernel" over its terms, the unit "kernel" over the plan's units, the finish "kernel" over
// its segments -- with every value passing between the phases as a reference image or a
// digit byte, as between the device's kernels.  Nothing in the product links this.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../paritytech-bn_amd/csrc/msm_many.h"
#include "../../paritytech-bn_amd/csrc/msm_many_plan.h"

using namespace bn;

namespace {

constexpr int PW = 24;  // words per G1 image

Jac<Fq> ld(const uint32_t* w) {
    return {widen<kPt>(fq_load_ref(w)), widen<kPt>(fq_load_ref(w + 8)), widen<kPt>(fq_load_ref(w + 16))};
}
void st(const Jac<Fq>& a, uint32_t* w) {
    fq_store_ref(a.x, w);
    fq_store_ref(a.y, w + 8);
    fq_store_ref(a.z, w + 16);
}
struct Raw {
    uint32_t w[PW];
};

}  // namespace

extern "C" {

// the byte of digit d and back (msm_many_digit_byte, msm_many_digit)
int msm_many_emul_digit_roundtrip(int d) { return msm_many_digit(msm_many_digit_byte(d)); }

// out[j] = the returned image of sum over off[j] <= i < off[j+1] of p[i] * scal[i] (scal:
// canonical scalars, 8 words each) at window width c with T terms per unit forced (0: the
// automatic choice at `lanes`) and launch sets of at most `chunk` terms; 0, or -1 for
// arguments the library refuses, -2 where the plan would send a segment to the alone path
int msm_many_emul_run(const uint32_t* p, const uint32_t* scal, const size_t* off, size_t m, int c, unsigned T,
                      size_t chunk, size_t lanes, uint32_t* out) {
    if (!msm_many_window_ok(c) || T > kMsmManyMaxUnitTerms || msm_many_offsets_refusal(off, m)) return -1;
    const MsmManyLimits lim = {T, kMsmManyMaxSegment, chunk ? chunk : 1, lanes, 16, SIZE_MAX};
    const MsmManyPlan plan = msm_many_plan(lim, off, m);
    std::vector<uint32_t> words(plan.words + 1, 0x7fffffffu);
    msm_many_fill(plan, off, words.data());
    for (const MsmManyItem& it : plan.items) {
        if (!it.packed) return -2;
        const size_t lo = off[it.j0];
        const uint32_t nt = (uint32_t)(off[it.j1] - lo);
        const uint64_t ndig = msm_many_digits(nt, c), nent = msm_many_entries(nt, c);
        std::vector<uint8_t> digits(ndig + 1, 0);
        std::vector<uint32_t> table((nent + 1) * PW, 0), parts((it.units + 1) * PW, 0);
        for (uint32_t t = 0; t < nt; ++t)
            msm_many_term<Fq>(
                ld(p + (lo + t) * PW), scal + (lo + t) * 8, c, t, nt, ndig, nent,
                [&](uint64_t i, uint8_t b) { digits[i] = b; },
                [&](uint64_t i, const Jac<Fq>& e) { st(e, &table[i * PW]); });
        const uint32_t* unit_off = words.data() + it.words_at;
        const uint32_t* seg_unit = unit_off + it.units + 1;
        for (size_t u = 0; u < it.units; ++u) {
            const uint32_t t0 = unit_off[u], cnt = unit_off[u + 1] - t0;
            if (t0 + cnt > nt || cnt > kMsmManyMaxUnitTerms) return -3;
            st(msm_many_unit_sum<Fq>(
                   [&](uint64_t i) { return digits[i]; },
                   [&](uint64_t i) {
                       Raw e;
                       memcpy(e.w, &table[i * PW], sizeof e.w);
                       return e;
                   },
                   [](const Raw& e) { return ld(e.w); }, c, t0, cnt, nt, ndig, nent),
               &parts[u * PW]);
        }
        for (size_t j = it.j0; j < it.j1; ++j) {
            const uint32_t u0 = seg_unit[j - it.j0], u1 = seg_unit[j - it.j0 + 1];
            if (u1 < u0 || u1 > it.units || u1 - u0 > kMsmManyMaxUnits) return -3;
            st(msm_many_segment<Fq>([&](uint32_t u) { return ld(&parts[(size_t)u * PW]); }, u0, u1), out + j * PW);
        }
    }
    return 0;
}
}
