// msm_split_emul.cpp -- TEST INFRASTRUCTURE (tests/test_msm_split_emul.py): the split of
// overlong bucket runs compiled for the host.  (1) The plan of csrc/msm.h (run cap, chunk and
// group positions, levels, array bounds) walked slot by slot over a given histogram exactly
// as the device's lanes walk it, with its invariants checked here.  (2) The whole bucket
// pipeline in plain loops over Fq and Fq2 with the bodies of csrc/msm_group.h, the long keys
// summed by chunks and fold levels through the same msm_run_task the kernels call, every
// value passing between the phases as a reference image.  Built as a shared object for
// ctypes, or with -DMSM_SPLIT_EMUL_MAIN as a stand-alone program (the plan checks over
// generated histograms) that can run under -fsanitize=address,undefined.  Nothing in the
// product links this.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#ifdef MSM_SPLIT_EMUL_MAIN
#include "../../paritytech-bn_amd/csrc/msm.h"  // the plan alone: integer code
#else
#include "../../paritytech-bn_amd/csrc/msm_group.h"
#endif

using namespace bn;

namespace {

struct Scan {
    std::vector<uint32_t> offsets, longkeys;
    uint32_t nent;
};
// what k_msm_scan leaves: the exclusive scan and the long keys in key order
Scan scan(const uint32_t* counts, uint32_t nkeys, uint32_t L) {
    Scan s;
    s.offsets.assign((size_t)nkeys + 1, 0);
    for (uint32_t j = 0; j < nkeys; ++j) {
        s.offsets[j + 1] = s.offsets[j] + counts[j];
        if (counts[j] > L) s.longkeys.push_back(j);
    }
    s.nent = s.offsets[nkeys];
    return s;
}

// The invariants of the plan over one histogram, as the host of n terms would launch it with
// nent_bound >= the entries.  0, or the negative number of the first one violated.
// info[0] = long keys, info[1] = the level at which the last key finished, info[2] = the
// level-0 slots in use (highest + 1), info[3] = the host's levels, info[4] = its level-0 bound.
int plan_check(const uint32_t* counts, uint32_t nkeys, uint32_t L, uint32_t n, uint32_t nent_bound, uint32_t* info) {
    if (L == 0 || L == kMsmRunUnsplit) return -1;
    const Scan s = scan(counts, nkeys, L);
    if (s.nent > nent_bound) return -2;
    for (uint32_t j = 0; j < nkeys; ++j)
        if (counts[j] > n) return -3;  // a bucket holds at most one entry per term
    const uint32_t nlong = (uint32_t)s.longkeys.size();
    const int levels = msm_fold_levels(n, L);
    info[0] = nlong, info[1] = 0, info[2] = 0, info[3] = (uint32_t)levels, info[4] = 0;
    if (nlong > msm_long_keys_bound(nent_bound, nkeys, L)) return -4;
    if (levels == 0) return nlong ? -5 : 0;  // the host launches nothing: no key may be long
    if (levels > kMsmMaxFoldLevels) return -6;
    const uint32_t* lk = s.longkeys.data();
    const uint32_t* off = s.offsets.data();
    auto task_at = [&](int level, uint32_t t) { return msm_run_task(lk, off, nlong, nkeys, s.nent, L, level, t); };
    auto is_long = [&](uint32_t key) { return key < nkeys && counts[key] > L; };
    // level 0: every entry of a long run in exactly one chunk, no other entry in any
    uint32_t slots = msm_level_slots(nent_bound, nkeys, L, 0);
    info[4] = slots;
    std::vector<uint32_t> covered(s.nent, 0), owner((size_t)slots, 0);  // owner: key + 1 of a written slot
    for (uint32_t t = 0; t < 2 * slots + 64; ++t) {
        const MsmRunTask k = task_at(0, t);
        if (!k.some) continue;
        if (t >= slots) return -10;  // outside the reserved bound
        if (k.last || !is_long(k.key)) return -11;
        if (k.lo >= k.hi || k.hi - k.lo > L) return -12;
        if (k.lo < off[k.key] || k.hi > off[k.key + 1]) return -13;
        for (uint32_t e = k.lo; e < k.hi; ++e) ++covered[e];
        owner[t] = k.key + 1;
        info[2] = t + 1;
    }
    for (uint32_t key = 0; key < nkeys; ++key)
        for (uint32_t e = off[key]; e < off[key + 1]; ++e)
            if (covered[e] != (is_long(key) ? 1u : 0u)) return -14;
    // the fold levels: every slot written below is read exactly once, by its own key; every
    // long key writes its bucket at exactly one level
    std::vector<uint32_t> finished(nkeys, 0);
    for (int lv = 1; lv <= levels; ++lv) {
        const uint32_t below = slots;
        slots = msm_level_slots(nent_bound, nkeys, L, lv);
        if (slots > below) return -20;  // the two arrays are reused level after level
        std::vector<uint32_t> next((size_t)slots, 0), used((size_t)below, 0);
        for (uint32_t t = 0; t < 2 * slots + 64; ++t) {
            const MsmRunTask k = task_at(lv, t);
            if (!k.some) continue;
            if (t >= slots) return -21;
            if (!is_long(k.key)) return -22;
            if (k.lo >= k.hi || k.hi - k.lo > kMsmFoldFan || k.hi > below) return -23;
            for (uint32_t i = k.lo; i < k.hi; ++i) {
                if (owner[i] != k.key + 1) return -24;  // unwritten, or another key's
                ++used[i];
            }
            if (k.last) {
                if (++finished[k.key] != 1) return -25;
                if (k.hi - k.lo < 2) return -26;  // a key's last group folds all it has left: at least two
                info[1] = (uint32_t)lv;
            } else {
                next[t] = k.key + 1;
            }
        }
        for (uint32_t i = 0; i < below; ++i)
            if (used[i] != (owner[i] ? 1u : 0u)) return -27;
        owner.swap(next);
    }
    for (uint32_t i = 0; i < slots; ++i)
        if (owner[i]) return -30;  // a partial sum left over: more levels than the host launches
    for (uint32_t key = 0; key < nkeys; ++key)
        if (finished[key] != (is_long(key) ? 1u : 0u)) return -31;
    return 0;
}

#ifndef MSM_SPLIT_EMUL_MAIN
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
// bucket pipeline at window width c and run cap `cap` (0: the default rule; kMsmRunUnsplit:
// never split), in the host's launch order.  stats[0] = long keys, stats[1] = fold levels
// launched.  0, or -1 for a width or cap outside the supported range.
template <template <int> class F, class Io>
int pipeline(const uint32_t* p, const uint32_t* k, uint32_t n, int c, uint32_t cap, uint32_t* out, uint32_t* stats) {
    if (!msm_window_ok(c) || (cap != kMsmRunUnsplit && cap > kMsmRunMax)) return -1;
    constexpr int PW = 3 * Io::W;  // words per point
    const uint32_t nwin = (uint32_t)msm_windows(c), nkeys = msm_num_keys(c);
    const uint32_t nseg = (msm_buckets(c) + kMsmSegment - 1) / kMsmSegment;
    auto point = [&](uint32_t i) { return Io::ld(p + (size_t)i * PW); };
    // the host's plan
    uint32_t L = cap ? cap : msm_run_cap_default(n, c);
    const int levels = msm_fold_levels(n, L);
    if (levels == 0) L = kMsmRunUnsplit;
    const uint32_t nent_bound = n * nwin;
    // recode, histogram, exclusive scan, scatter (zero digits and zero points: no entry)
    std::vector<uint32_t> counts(nkeys, 0), sorted;
    Scan s;
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
            s = scan(counts.data(), nkeys, L);
            sorted.assign(s.nent, 0);
            for (uint32_t j = 0; j < nkeys; ++j) counts[j] = s.offsets[j];  // the cursors
        }
    }
    const uint32_t nent = s.nent, nlong = (uint32_t)s.longkeys.size();
    stats[0] = nlong, stats[1] = (uint32_t)levels;
    // per-bucket sums of the short keys (k_msm_accumulate); a long key's stays poisoned until a fold writes it
    std::vector<uint32_t> buckets((size_t)nkeys * PW, 0xdeadbeefu);
    for (uint32_t key = 0; key < nkeys; ++key) {
        if (s.offsets[key + 1] - s.offsets[key] > L) continue;
        Io::st(msm_bucket_sum<F>(point, n, sorted.data(), s.offsets[key], s.offsets[key + 1]), &buckets[(size_t)key * PW]);
    }
    // the long keys: chunk sums (k_msm_chunk), then the fold levels (k_msm_fold), slot by slot
    if (levels) {
        uint32_t slots = msm_level_slots(nent_bound, nkeys, L, 0);
        std::vector<uint32_t> a((size_t)slots * PW, 0xdeadbeefu), b;
        for (uint32_t t = 0; t < slots; ++t) {
            const MsmRunTask task = msm_run_task(s.longkeys.data(), s.offsets.data(), nlong, nkeys, nent, L, 0, t);
            if (task.some) Io::st(msm_bucket_sum<F>(point, n, sorted.data(), task.lo, task.hi), &a[(size_t)t * PW]);
        }
        for (int lv = 1; lv <= levels; ++lv) {
            const uint32_t nsrc = slots;
            slots = msm_level_slots(nent_bound, nkeys, L, lv);
            b.assign((size_t)slots * PW, 0xdeadbeefu);
            auto part = [&](uint32_t i) { return Io::ld(&a[(size_t)i * PW]); };
            for (uint32_t t = 0; t < slots; ++t) {
                const MsmRunTask task = msm_run_task(s.longkeys.data(), s.offsets.data(), nlong, nkeys, nent, L, lv, t);
                if (!task.some || task.hi > nsrc) continue;
                Io::st(msm_fold_sum<F>(part, task.lo, task.hi), task.last ? &buckets[(size_t)task.key * PW] : &b[(size_t)t * PW]);
            }
            a.swap(b);
        }
    }
    // per-segment reduction, parts[s * nwin + w]
    std::vector<uint32_t> parts((size_t)nseg * nwin * PW);
    auto bucket = [&](uint32_t key) { return Io::ld(&buckets[(size_t)key * PW]); };
    for (uint32_t sg = 0; sg < nseg; ++sg)
        for (uint32_t w = 0; w < nwin; ++w)
            Io::st(msm_segment_sum<F>(bucket, c, nkeys, sg, w), &parts[((size_t)sg * nwin + w) * PW]);
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
#endif  // !MSM_SPLIT_EMUL_MAIN

}  // namespace

extern "C" {
int msm_split_emul_plan_check(const uint32_t* counts, unsigned nkeys, unsigned L, unsigned n, unsigned nent_bound,
                              uint32_t* info) {
    return plan_check(counts, nkeys, L, n, nent_bound, info);
}
#ifndef MSM_SPLIT_EMUL_MAIN
int msm_split_emul_g1(const uint32_t* p, const uint32_t* k, unsigned n, int c, unsigned cap, uint32_t* out,
                      uint32_t* stats) {
    return pipeline<Fq, G1Io>(p, k, n, c, cap, out, stats);
}
int msm_split_emul_g2(const uint32_t* p, const uint32_t* k, unsigned n, int c, unsigned cap, uint32_t* out,
                      uint32_t* stats) {
    return pipeline<Fq2, G2Io>(p, k, n, c, cap, out, stats);
}
#endif
unsigned msm_split_emul_cap_default(unsigned n, int c) { return msm_run_cap_default(n, c); }
int msm_split_emul_levels(unsigned n, unsigned L) { return msm_fold_levels(n, L); }
unsigned msm_split_emul_level_slots(unsigned nent, unsigned nkeys, unsigned L, int level) {
    return msm_level_slots(nent, nkeys, L, level);
}
unsigned msm_split_emul_fan() { return kMsmFoldFan; }
unsigned msm_split_emul_run_min() { return kMsmRunMin; }
int msm_split_emul_max_levels() { return kMsmMaxFoldLevels; }
}

#ifdef MSM_SPLIT_EMUL_MAIN
// The plan checks over generated histograms: the shapes of tests/test_msm_split_emul.py and
// random ones from a fixed xorshift stream.  Prints what failed; exit status 0 when all hold.
int main() {
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (uint32_t)(x >> 32);
    };
    int bad = 0, runs = 0;
    auto run = [&](const std::vector<uint32_t>& counts, uint32_t L, const char* what) {
        uint32_t n = 1, nent = 0, info[5];
        for (uint32_t v : counts) n = v > n ? v : n, nent += v;
        const int rc = plan_check(counts.data(), (uint32_t)counts.size(), L, n, nent + rnd() % 5, info);
        ++runs;
        if (rc != 0) {
            printf("%s: L = %u, %zu keys, n = %u: invariant %d\n", what, L, counts.size(), n, rc);
            ++bad;
        }
    };
    for (uint32_t L : {1u, 2u, 3u, 7u, 64u}) {
        for (uint32_t cnt : {L, L + 1, L * 32 - 1, L * 32, L * 32 + 1, L * 1024 - 1, L * 1024, L * 1024 + 1}) {
            run({cnt}, L, "one key");
            run({0, cnt, 0}, L, "one key between empty ones");
            run({cnt, 1, cnt + 1, 0, L, cnt}, L, "long and short alternating");
        }
        for (int it = 0; it < 200; ++it) {
            std::vector<uint32_t> counts(1 + rnd() % 40);
            for (uint32_t& v : counts) v = rnd() % 4 == 0 ? rnd() % (L * 40 + 2) : rnd() % (L + 2);
            run(counts, L, "random");
        }
    }
    printf("msm_split_emul: %d plan checks, %d failed\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
