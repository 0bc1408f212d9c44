// msm_basis_g2_emul.cpp -- TEST INFRASTRUCTURE (tests/test_msm_basis_g2_emul.py): the bodies of
// csrc/msm_basis.h, msm_group.h, msm.h and curve.h's jac_add_mixed compiled for the host over
// Fq2, and the fixed-basis pipeline around them in plain loops, in the host's launch order --
// table build, recoding over the zero flags, histogram, scan, scatter, accumulation by mixed
// additions through the prefetch-shaped loop body, chunks and fold levels at a given run cap,
// the collapse of the windows below the top one, the reduction of two windows, the trees,
// the finish -- with every value passing between the phases as a reference image, as between
// the device's kernels.  Nothing in the product links this.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../paritytech-bn_amd/csrc/msm_basis.h"

using namespace bn;

namespace {

constexpr int PW = 48;  // words per G2 image
constexpr int EW = 32;  // words per table entry: the lane halves [x.c0, y.c0 | x.c1, y.c1]

Fq2<kPt> ld2(const uint32_t* w) { return widen<kPt>(Fq2<2>{fq_load_ref(w), fq_load_ref(w + 8)}); }
void st2(const Fq2<kPt>& a, uint32_t* w) {
    fq_store_ref(a.c0, w);
    fq_store_ref(a.c1, w + 8);
}
Jac<Fq2> ld(const uint32_t* w) { return {ld2(w), ld2(w + 16), ld2(w + 32)}; }
void st(const Jac<Fq2>& a, uint32_t* w) {
    st2(a.x, w);
    st2(a.y, w + 16);
    st2(a.z, w + 32);
}
struct Raw {
    uint32_t w[EW];
};
// the two lanes' halves put together
void decode(const Raw& e, Fq2<2>& x, Fq2<2>& y) {
    x = {fq_load_ref(e.w), fq_load_ref(e.w + 16)};
    y = {fq_load_ref(e.w + 8), fq_load_ref(e.w + 24)};
}

// table[msm_basis_index(nbases, b, w)] and zero[b] of the nbases bases at width c
void build(const uint32_t* bases, uint32_t nbases, int c, std::vector<uint32_t>& table, std::vector<uint8_t>& zero) {
    const uint32_t nwin = (uint32_t)msm_windows(c);
    table.assign((size_t)nbases * nwin * EW, 0);
    zero.assign(nbases, 0);
    for (uint32_t b = 0; b < nbases; ++b) {
        const Jac<Fq2> base = ld(bases + (size_t)b * PW);
        zero[b] = jac_is_zero(base) ? 1 : 0;
        if (zero[b]) continue;
        msm_basis_build<Fq2>(base, c, [&](uint32_t w, const Fq2<kPt>& x, const Fq2<kPt>& y) {
            uint32_t* e = &table[(size_t)msm_basis_index(nbases, b, w) * EW];
            fq_store_ref(x.c0, e);
            fq_store_ref(y.c0, e + 8);
            fq_store_ref(x.c1, e + 16);
            fq_store_ref(y.c1, e + 24);
        });
    }
}

}  // namespace

extern "C" {

int msm_basis_g2_emul_auto_window(unsigned long long nbases) { return msm_basis_auto_window_g2(nbases); }

// out[(w * nbases + b) * 32 ..] = entry (b, w) in the table's lane-half layout; flags[b] = the zero flag; 0, or -1
// for arguments the library refuses
int msm_basis_g2_emul_table(const uint32_t* bases, unsigned nbases, int c, uint32_t* out, uint8_t* flags) {
    if (!msm_basis_entries_at(nbases, c)) return -1;
    std::vector<uint32_t> table;
    std::vector<uint8_t> zero;
    build(bases, nbases, c, table, zero);
    memcpy(out, table.data(), table.size() * 4);
    memcpy(flags, zero.data(), zero.size());
    return 0;
}

// out = the returned image of sum_{i < n} bases[i] * k[i] (k: canonical scalars, 8 words each)
// over a table of all nbases bases at width c and run cap `cap` (0: the default rule;
// kMsmRunUnsplit: never split).  stats[0] = long keys, stats[1] = fold levels launched.  0, or
// -1 for refused arguments.
int msm_basis_g2_emul_run(const uint32_t* bases, unsigned nbases, const uint32_t* k, unsigned n, int c, unsigned cap,
                          uint32_t* out, uint32_t* stats) {
    if (!msm_basis_entries_at(nbases, c) || n > nbases || (cap != kMsmRunUnsplit && cap > kMsmRunMax)) return -1;
    stats[0] = stats[1] = 0;
    if (n == 0) {
        st(msm_finish_point(jac_zero<Fq2>()), out);
        return 0;
    }
    std::vector<uint32_t> table;
    std::vector<uint8_t> zero;
    build(bases, nbases, c, table, zero);
    const uint32_t nwin = (uint32_t)msm_windows(c), nkeys = msm_num_keys(c), nb = msm_buckets(c);
    const uint32_t nseg = (nb + kMsmSegment - 1) / kMsmSegment;
    // the host's plan
    uint32_t L = cap ? cap : msm_run_cap_default(n, c);
    const int levels = msm_fold_levels(n, L);
    if (levels == 0) L = kMsmRunUnsplit;
    const uint32_t nent_bound = n * nwin;
    // recode, histogram, exclusive scan, scatter (zero digits and flagged bases: no entry)
    std::vector<uint32_t> counts(nkeys, 0), offsets((size_t)nkeys + 1, 0), longkeys, sorted;
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t i = 0; i < n; ++i) {
            if (zero[i]) continue;
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
            for (uint32_t j = 0; j < nkeys; ++j) {
                offsets[j + 1] = offsets[j] + counts[j];
                if (counts[j] > L) longkeys.push_back(j);
            }
            sorted.assign(offsets[nkeys], 0);
            for (uint32_t j = 0; j < nkeys; ++j) counts[j] = offsets[j];  // the cursors
        }
    }
    const uint32_t nent = offsets[nkeys], nlong = (uint32_t)longkeys.size();
    stats[0] = nlong, stats[1] = (uint32_t)levels;
    // one "lane" per key or chunk: mixed additions of its entries' table points in window w
    auto run_sum = [&](uint32_t w, uint32_t lo, uint32_t hi) {
        const uint32_t* row = &table[(size_t)msm_basis_index(nbases, 0, w) * EW];
        return msm_basis_run_sum<Fq2>([&](uint32_t e) { return sorted[e]; },
                                     [&](uint32_t idx) {
                                         Raw r;
                                         memcpy(r.w, row + (size_t)(idx < n ? idx : 0) * EW, sizeof r.w);
                                         return r;
                                     },
                                     decode, n, lo, hi);
    };
    // a long key's bucket stays poisoned until a fold writes it
    std::vector<uint32_t> buckets((size_t)nkeys * PW, 0xdeadbeefu);
    for (uint32_t key = 0; key < nkeys; ++key) {
        if (offsets[key + 1] - offsets[key] > L) continue;
        st(run_sum((uint32_t)msm_key_window(c, key), offsets[key], offsets[key + 1]), &buckets[(size_t)key * PW]);
    }
    if (levels) {
        uint32_t slots = msm_level_slots(nent_bound, nkeys, L, 0);
        std::vector<uint32_t> a((size_t)slots * PW, 0xdeadbeefu), b;
        for (uint32_t t = 0; t < slots; ++t) {
            const MsmRunTask task = msm_run_task(longkeys.data(), offsets.data(), nlong, nkeys, nent, L, 0, t);
            if (task.some) st(run_sum((uint32_t)msm_key_window(c, task.key), task.lo, task.hi), &a[(size_t)t * PW]);
        }
        for (int lv = 1; lv <= levels; ++lv) {
            const uint32_t nsrc = slots;
            slots = msm_level_slots(nent_bound, nkeys, L, lv);
            b.assign((size_t)slots * PW, 0xdeadbeefu);
            auto part = [&](uint32_t i) { return ld(&a[(size_t)i * PW]); };
            for (uint32_t t = 0; t < slots; ++t) {
                const MsmRunTask task = msm_run_task(longkeys.data(), offsets.data(), nlong, nkeys, nent, L, lv, t);
                if (!task.some || task.hi > nsrc) continue;
                st(msm_fold_sum<Fq2>(part, task.lo, task.hi), task.last ? &buckets[(size_t)task.key * PW] : &b[(size_t)t * PW]);
            }
            a.swap(b);
        }
    }
    // rows[0 .. width) = the sum of m rows of `width` points by a halving tree in place (odd tail carried)
    auto tree = [&](uint32_t* rows, uint32_t m, uint32_t width) {
        while (m > 1) {
            const uint32_t h = (m + 1) / 2;
            for (size_t i = 0; i < (size_t)(m - h) * width; ++i)
                st(jac_add(ld(rows + i * PW), ld(rows + ((size_t)h * width + i) * PW)), rows + i * PW);
            m = h;
        }
    };
    // the collapse: the rows of windows 0 .. W - 2 into window 0's
    tree(buckets.data(), nwin - 1, nb);
    // two windows reduced, parts[s * 2 + which]
    std::vector<uint32_t> parts((size_t)nseg * 2 * PW);
    auto bucket = [&](uint32_t key) { return ld(&buckets[(size_t)key * PW]); };
    for (uint32_t sg = 0; sg < nseg; ++sg)
        for (uint32_t which = 0; which < 2; ++which)
            st(msm_segment_sum<Fq2>(bucket, c, nkeys, sg, msm_basis_reduce_window(c, which)), &parts[((size_t)sg * 2 + which) * PW]);
    tree(parts.data(), nseg, 2);
    tree(parts.data(), 2, 1);
    st(msm_finish_point(ld(parts.data())), out);
    return 0;
}
}
