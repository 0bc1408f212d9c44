// msm_g2_emul.cpp -- TEST INFRASTRUCTURE (tests/test_msm_g2_emul.py): the shared
// bodies of csrc/msm_group.h compiled for the host over Fq2 (and over Fq), and the
// whole bucket pipeline around them in plain loops -- recode, sort by key, per-bucket
// sum, per-segment reduction, segment tree, Horner, finish -- with every value
// passing between the phases as a reference image, as between the device's kernels.
// Nothing in the product links this.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../paritytech-bn_amd/csrc/msm_group.h"

using namespace bn;

namespace {

// a group's point images: W 32-bit words per coordinate
struct G1Io {
    static constexpr int W = 8;
    static Jac<Fq> ld(const uint32_t* w) {
        return {widen<kPt>(fq_load_ref(w)), widen<kPt>(fq_load_ref(w + 8)), widen<kPt>(fq_load_ref(w + 16))};
    }
    static void st(const Jac<Fq>& a, uint32_t* w) {
        fq_store_ref(a.x, w);
        fq_store_ref(a.y, w + 8);
        fq_store_ref(a.z, w + 16);
    }
};
struct G2Io {
    static constexpr int W = 16;
    static Fq2<kPt> ld2(const uint32_t* w) { return widen<kPt>(Fq2<2>{fq_load_ref(w), fq_load_ref(w + 8)}); }
    static void st2(const Fq2<kPt>& a, uint32_t* w) {
        fq_store_ref(a.c0, w);
        fq_store_ref(a.c1, w + 8);
    }
    static Jac<Fq2> ld(const uint32_t* w) { return {ld2(w), ld2(w + 16), ld2(w + 32)}; }
    static void st(const Jac<Fq2>& a, uint32_t* w) {
        st2(a.x, w);
        st2(a.y, w + 16);
        st2(a.z, w + 32);
    }
};

// out = the returned image of sum p[i] * k[i] (k: canonical scalars, 8 words each) by the
// bucket pipeline at window width c; 0, or -1 for a width outside the supported range
template <template <int> class F, class Io>
int pipeline(const uint32_t* p, const uint32_t* k, uint32_t n, int c, uint32_t* out) {
    if (!msm_window_ok(c)) return -1;
    constexpr int PW = 3 * Io::W;  // words per point
    const uint32_t nwin = (uint32_t)msm_windows(c), nkeys = msm_num_keys(c);
    const uint32_t nseg = (msm_buckets(c) + kMsmSegment - 1) / kMsmSegment;
    auto point = [&](uint32_t i) { return Io::ld(p + (size_t)i * PW); };
    // recode, histogram, exclusive scan, scatter (zero digits and zero points: no entry)
    std::vector<uint32_t> counts(nkeys, 0), offsets(nkeys + 1, 0), sorted;
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t i = 0; i < n; ++i) {
            if (jac_is_zero(point(i))) continue;
            int32_t d[kMsmMaxWindows];
            msm_recode(k + (size_t)i * 8, c, d);
            for (uint32_t w = 0; w < nwin; ++w) {
                if (d[w] == 0) continue;
                const uint32_t key = msm_key(c, (int)w, d[w], i);
                if (pass == 0) ++counts[key];
                else sorted[counts[key]++] = msm_entry(i, d[w]);
            }
        }
        if (pass == 0) {
            for (uint32_t j = 0; j < nkeys; ++j) offsets[j + 1] = offsets[j] + counts[j];
            sorted.assign(offsets[nkeys], 0);
            for (uint32_t j = 0; j < nkeys; ++j) counts[j] = offsets[j];  // the cursors
        }
    }
    const uint32_t nent = (uint32_t)sorted.size();
    // per-bucket sums
    std::vector<uint32_t> buckets((size_t)nkeys * PW);
    for (uint32_t key = 0; key < nkeys; ++key)
        Io::st(msm_bucket_sum<F>(point, n, sorted.data(), offsets[key], offsets[key + 1] < nent ? offsets[key + 1] : nent),
               &buckets[(size_t)key * PW]);
    // per-segment reduction, parts[s * nwin + w]
    std::vector<uint32_t> parts((size_t)nseg * nwin * PW);
    auto bucket = [&](uint32_t key) { return Io::ld(&buckets[(size_t)key * PW]); };
    for (uint32_t s = 0; s < nseg; ++s)
        for (uint32_t w = 0; w < nwin; ++w)
            Io::st(msm_segment_sum<F>(bucket, c, nkeys, s, w), &parts[((size_t)s * nwin + w) * PW]);
    // halving addition tree over the segments (odd tail carried)
    for (uint32_t m = nseg; m > 1;) {
        const uint32_t h = (m + 1) / 2;
        for (size_t i = 0; i < (size_t)(m - h) * nwin; ++i)
            Io::st(jac_add(Io::ld(&parts[i * PW]), Io::ld(&parts[((size_t)h * nwin + i) * PW])), &parts[i * PW]);
        m = h;
    }
    // Horner over the windows, the returned image
    auto win = [&](int w) { return Io::ld(&parts[(size_t)w * PW]); };
    Io::st(msm_finish_point(msm_horner_sum<F>(win, c)), out);
    return 0;
}

}  // namespace

extern "C" {
int msm_g2_emul_g2(const uint32_t* p, const uint32_t* k, unsigned n, int c, uint32_t* out) {
    return pipeline<Fq2, G2Io>(p, k, n, c, out);
}
int msm_g2_emul_g1(const uint32_t* p, const uint32_t* k, unsigned n, int c, uint32_t* out) {
    return pipeline<Fq, G1Io>(p, k, n, c, out);
}
unsigned msm_g2_emul_segment() { return kMsmSegment; }
}
