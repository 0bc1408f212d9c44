// msm_fixed_emul.cpp -- TEST INFRASTRUCTURE (tests/test_msm_fixed_emul.py): the bodies
// of csrc/msm_fixed.h and curve.h's jac_add_mixed compiled for the host over Fq, and the
// prepared-bases pipeline around them in plain loops -- table build, per-lane partial sums
// for a given number of lanes per output, halving tree, finish -- with every value passing
// between the phases as a reference image, as between the device's kernels.  Nothing in
// the product links this.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../paritytech-bn_amd/csrc/msm_fixed.h"

using namespace bn;

namespace {

constexpr int PW = 24;  // words per G1 image
constexpr int EW = 16;  // words per table entry: x, y

Jac<Fq> ld(const uint32_t* w) {
    return {widen<kPt>(fq_load_ref(w)), widen<kPt>(fq_load_ref(w + 8)), widen<kPt>(fq_load_ref(w + 16))};
}
void st(const Jac<Fq>& a, uint32_t* w) {
    fq_store_ref(a.x, w);
    fq_store_ref(a.y, w + 8);
    fq_store_ref(a.z, w + 16);
}
struct Raw {
    uint32_t w[EW];
};
void decode(const Raw& e, Fq<2>& x, Fq<2>& y) {
    x = fq_load_ref(e.w);
    y = fq_load_ref(e.w + 8);
}

}  // namespace

extern "C" {

unsigned long long msm_fixed_emul_entries(unsigned long long k, int c) { return msm_fixed_entries(k, c); }
unsigned msm_fixed_emul_auto_lanes(unsigned long long m, unsigned long long k, int c) {
    return msm_fixed_auto_lanes(m, k, c);
}

// out = acc + (x, y) [negated] by jac_add_mixed, as a Jacobian image
void msm_fixed_emul_add_mixed(const uint32_t* acc, const uint32_t* entry, int neg, uint32_t* out) {
    Raw e;
    memcpy(e.w, entry, sizeof e.w);
    st(msm_fixed_add<Fq>(ld(acc), e, neg != 0, true, decode), out);
}

// out[j] = the returned image of sum_b bases[b] * scal[j * k + b] for j < m (scal: canonical
// scalars, 8 words each) through a table of width c and L lanes per output; 0, or -1 for
// arguments the library refuses
int msm_fixed_emul_run(const uint32_t* bases, unsigned k, const uint32_t* scal, unsigned m, int c, unsigned L,
                       uint32_t* out) {
    const uint64_t nent64 = msm_fixed_entries(k, c);
    if (!nent64 || c == 0 || !msm_fixed_lanes_ok((int)L)) return -1;
    const uint32_t nent = (uint32_t)nent64, nwin = (uint32_t)msm_windows(c);
    // the table: one "lane" per (base, window)
    std::vector<uint32_t> table((size_t)nent * EW, 0);
    std::vector<uint8_t> zero(k, 0);
    for (uint32_t b = 0; b < k; ++b) {
        const Jac<Fq> base = ld(bases + (size_t)b * PW);
        zero[b] = jac_is_zero(base) ? 1 : 0;
        if (zero[b]) continue;
        for (uint32_t w = 0; w < nwin; ++w)
            msm_fixed_build<Fq>(base, c, (int)w, msm_fixed_index(c, nwin, b, w, 1), nent,
                                [&](uint32_t idx, const Fq<kPt>& x, const Fq<kPt>& y) {
                                    fq_store_ref(x, &table[(size_t)idx * EW]);
                                    fq_store_ref(y, &table[(size_t)idx * EW + 8]);
                                });
    }
    // the lanes' partial sums, parts[l * m + j]
    std::vector<uint32_t> parts((size_t)L * m * PW);
    auto fetch = [&](uint32_t idx) {
        Raw e;
        memcpy(e.w, &table[(size_t)idx * EW], sizeof e.w);
        return e;
    };
    for (uint32_t l = 0; l < L; ++l)
        for (uint32_t j = 0; j < m; ++j) {
            auto scalar = [&](uint32_t b, uint32_t* s) { memcpy(s, scal + ((size_t)j * k + b) * 8, 32); };
            auto is_zero = [&](uint32_t b) { return zero[b] != 0; };
            st(msm_fixed_lane_sum<Fq>(scalar, is_zero, fetch, decode, k, c, nent, l, L),
               &parts[((size_t)l * m + j) * PW]);
        }
    // halving addition tree over the lanes (contiguous halves), then the returned image
    for (uint32_t n = L; n > 1;) {
        const uint32_t h = (n + 1) / 2;
        for (size_t i = 0; i < (size_t)(n - h) * m; ++i)
            st(jac_add(ld(&parts[i * PW]), ld(&parts[((size_t)h * m + i) * PW])), &parts[i * PW]);
        n = h;
    }
    for (uint32_t j = 0; j < m; ++j) st(msm_finish_point(ld(&parts[(size_t)j * PW])), out + (size_t)j * PW);
    return 0;
}
}
