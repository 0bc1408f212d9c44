// msm_basis_many_emul.cpp -- TEST INFRASTRUCTURE (tests/test_msm_basis_many_emul.py): the
// batched fixed-basis pipeline (bn_g1_msm_basis_many) in plain loops over the index arithmetic
// of csrc/msm_basis_many.h and the bodies of msm.h, msm_group.h and msm_basis.h compiled for
// the host, in the host's launch order: per launch set of S vectors the histogram, the scans,
// the scatter, the accumulation, chunks and fold levels at a given run cap, the collapse of
// the windows over rows of S * 2^(c-1) buckets, the reduction of two windows with the vector
// innermost, the trees on widths 2 S and S, the finish.  Every "lane" loop runs over the
// kernel's lane index and decodes it with the header's functions; every array has exactly the
// size the host plan allocates, and every access is recorded, so the test can assert that no
// stage touches an index past its array.  Nothing in the product links this.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../paritytech-bn_amd/csrc/msm_basis_many.h"

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

// An array of `size` elements of `unit` words each that records the highest element index any
// stage asked for (hi = that index + 1); an index past the array is recorded and served from
// a spare element, so that the run goes on and the test reports it.
struct Tracked {
    std::vector<uint32_t> w;
    uint64_t size = 0, hi = 0;
    int unit = 1;
    void alloc(uint64_t n, int u, uint32_t fill) {
        size = n, unit = u, hi = 0;
        w.assign((size_t)(n + 1) * u, fill);
    }
    uint32_t* at(uint64_t i) {
        hi = std::max(hi, i + 1);
        return &w[(size_t)(i < size ? i : size) * unit];
    }
};

void build(const uint32_t* bases, uint32_t nbases, int c, std::vector<uint32_t>& table, std::vector<uint8_t>& zero) {
    const uint32_t nwin = (uint32_t)msm_windows(c);
    table.assign((size_t)nbases * nwin * EW, 0);
    zero.assign(nbases, 0);
    for (uint32_t b = 0; b < nbases; ++b) {
        const Jac<Fq> base = ld(bases + (size_t)b * PW);
        zero[b] = jac_is_zero(base) ? 1 : 0;
        if (zero[b]) continue;
        msm_basis_build<Fq>(base, c, [&](uint32_t w, const Fq<kPt>& x, const Fq<kPt>& y) {
            uint32_t* e = &table[(size_t)msm_basis_index(nbases, b, w) * EW];
            fq_store_ref(x, e);
            fq_store_ref(y, e + 8);
        });
    }
}

}  // namespace

extern "C" {

unsigned long long msm_basis_many_emul_set(unsigned long long m, unsigned long long n, int c, unsigned long long max_keys,
                                           unsigned long long forced) {
    return msm_basis_many_set(m, n, c, max_keys, forced);
}

// out[j * 24 ..] = the returned image of sum_{i < n} bases[i] * k[(j * k_stride + i) * 8 ..]
// (canonical scalars, 8 words each), j < m, over a table of all nbases bases at width c, run
// cap `cap` (0: the default rule; kMsmRunUnsplit: never split) and `forced` vectors per launch
// set (0: the default).  nlong[j] = the long keys of vector j.  stats = {fold levels, S, launch
// sets}; touched / alloc = per array (keys, sorted, buckets, run_a, run_b, parts) the highest
// index + 1 any stage asked for over all sets, and the elements the host plan allocates.
// 0, or -1 for refused arguments.
int msm_basis_many_emul_run(const uint32_t* bases, unsigned nbases, const uint32_t* k, unsigned long long k_stride,
                            unsigned m, unsigned n, int c, unsigned cap, unsigned forced, uint32_t* out, uint32_t* nlong,
                            uint32_t* stats, unsigned long long* touched, unsigned long long* alloc) {
    if (c == 0 || !msm_basis_entries(nbases, c) || n > nbases || k_stride < n ||
        (cap != kMsmRunUnsplit && cap > kMsmRunMax))
        return -1;
    for (int a = 0; a < 6; ++a) touched[a] = alloc[a] = 0;
    stats[0] = stats[1] = stats[2] = 0;
    for (unsigned j = 0; j < m; ++j) nlong[j] = 0;
    if (m == 0) return 0;
    if (n == 0) {
        for (unsigned j = 0; j < m; ++j) st(msm_finish_point(jac_zero<Fq>()), out + (size_t)j * PW);
        return 0;
    }
    std::vector<uint32_t> table;
    std::vector<uint8_t> zero;
    build(bases, nbases, c, table, zero);
    const uint32_t nwin = (uint32_t)msm_windows(c), nkeys = msm_num_keys(c), nb = msm_buckets(c);
    const uint32_t nseg = (nb + kMsmSegment - 1) / kMsmSegment;
    // one vector's plan (capi_msm.hip msm_plan_at) and the set size
    uint32_t L = cap ? cap : msm_run_cap_default(n, c);
    const int levels = msm_fold_levels(n, L);
    if (levels == 0) L = kMsmRunUnsplit;
    const uint32_t nent = n * nwin;
    const uint32_t sa = msm_basis_many_slots(nent, nkeys, L, levels, 0), sb = msm_basis_many_slots(nent, nkeys, L, levels, 1);
    const uint32_t S = (uint32_t)msm_basis_many_set(m, n, c, 0, forced);
    const uint64_t words = msm_basis_many_words(nkeys);
    stats[0] = (uint32_t)levels, stats[1] = S;
    // the workspace, as msm_basis_many_grow sizes it; poisoned so that a slot read before it is written shows
    Tracked keys, sorted, buckets, run_a, run_b, parts;
    keys.alloc(S * words, 1, 0xdeadbeefu);
    sorted.alloc((uint64_t)S * nent, 1, 0xdeadbeefu);
    buckets.alloc((uint64_t)S * nkeys, PW, 0xdeadbeefu);
    run_a.alloc((uint64_t)S * sa, PW, 0xdeadbeefu);
    run_b.alloc((uint64_t)S * sb, PW, 0xdeadbeefu);
    parts.alloc((uint64_t)nseg * 2 * S, PW, 0xdeadbeefu);
    Tracked* arrays[6] = {&keys, &sorted, &buckets, &run_a, &run_b, &parts};
    for (int a = 0; a < 6; ++a) alloc[a] = arrays[a]->size;

    // rows[0 .. width) = the sum of r rows of `width` points by a halving tree in place (msm_tree)
    auto tree = [&](Tracked& buf, uint32_t r, uint64_t width) {
        while (r > 1) {
            const uint32_t h = (r + 1) / 2;
            for (uint64_t i = 0; i < (uint64_t)(r - h) * width; ++i)
                st(jac_add(ld(buf.at(i)), ld(buf.at((uint64_t)h * width + i))), buf.at(i));
            r = h;
        }
    };
    for (uint32_t off = 0; off < m; off += S) {
        const uint32_t sc = std::min(m - off, S);
        ++stats[2];
        const uint32_t* kset = k + (size_t)off * k_stride * 8;
        // the 2-D memset: every vector's counts
        for (uint32_t v = 0; v < sc; ++v)
            for (uint32_t j = 0; j < nkeys; ++j) *keys.at(msm_basis_many_counts_at(nkeys, v) + j) = 0;
        // count, scan, scatter: one lane per (vector, term), one block per vector
        for (int pass = 0; pass < 2; ++pass) {
            for (uint64_t t = 0; t < (uint64_t)sc * n; ++t) {
                const MsmBasisManyLane at = msm_basis_many_lane(t, n, sc);
                if (at.v >= sc || zero[at.i]) continue;
                int32_t d[kMsmMaxWindows];
                msm_recode(kset + ((size_t)at.v * k_stride + at.i) * 8, c, d);
                const uint64_t first = pass ? msm_basis_many_cursors_at(nkeys, at.v) : msm_basis_many_counts_at(nkeys, at.v);
                for (uint32_t w = 0; w < nwin; ++w) {
                    if (d[w] == 0) continue;
                    const uint32_t key = msm_key(c, (int)w, d[w], at.i);
                    const uint32_t pos = (*keys.at(first + key))++;
                    if (pass && pos < *keys.at(msm_basis_many_offsets_at(nkeys, at.v) + key + 1) && pos < nent)
                        *sorted.at(msm_basis_many_sorted_at(nent, at.v) + pos) = msm_entry(at.i, d[w]);
                }
            }
            if (pass == 0) {
                for (uint32_t v = 0; v < sc; ++v) {
                    uint32_t run = 0, rank = 0;
                    const uint64_t cnt = msm_basis_many_counts_at(nkeys, v), cur = msm_basis_many_cursors_at(nkeys, v);
                    const uint64_t ofs = msm_basis_many_offsets_at(nkeys, v), lng = msm_basis_many_longinfo_at(nkeys, v);
                    for (uint32_t j = 0; j < nkeys; ++j) {
                        const uint32_t cj = *keys.at(cnt + j);
                        *keys.at(ofs + j) = run;
                        *keys.at(cur + j) = run;
                        run += cj;
                        if (cj > L) *keys.at(lng + 1 + rank++) = j;
                    }
                    *keys.at(ofs + nkeys) = run;
                    *keys.at(lng) = rank;
                    nlong[off + v] = rank;
                }
            }
        }
        // a vector's block as msm_run_task and the run sums read it (within the recorded block)
        auto offsets_of = [&](uint32_t v) { return keys.at(msm_basis_many_offsets_at(nkeys, v)); };
        auto longinfo_of = [&](uint32_t v) { return keys.at(msm_basis_many_longinfo_at(nkeys, v)); };
        auto run_sum = [&](uint32_t v, uint32_t w, uint32_t lo, uint32_t hi) {
            const uint32_t* row = &table[(size_t)msm_basis_index(nbases, 0, w) * EW];
            const uint64_t region = msm_basis_many_sorted_at(nent, v);
            return msm_basis_run_sum<Fq>([&](uint32_t e) { return *sorted.at(region + e); },
                                         [&](uint32_t idx) {
                                             Raw r;
                                             memcpy(r.w, row + (size_t)(idx < n ? idx : 0) * EW, sizeof r.w);
                                             return r;
                                         },
                                         decode, n, lo, hi);
        };
        // the buckets of this set start poisoned: a long key's stays so until a fold writes it
        for (uint64_t i = 0; i < (uint64_t)sc * nkeys; ++i)
            for (int j = 0; j < PW; ++j) buckets.w[(size_t)i * PW + j] = 0xdeadbeefu;
        // accumulate: one lane per (vector, key)
        for (uint64_t t = 0; t < (uint64_t)sc * nkeys; ++t) {
            const MsmBasisManyLane at = msm_basis_many_lane(t, nkeys, sc);
            if (at.v >= sc) continue;
            const uint32_t* offsets = offsets_of(at.v);
            uint32_t hi = std::min(offsets[at.i + 1], nent), lo = std::min(offsets[at.i], hi);
            if (hi - lo > L) continue;
            st(run_sum(at.v, (uint32_t)msm_key_window(c, at.i), lo, hi), buckets.at(msm_basis_many_bucket(c, sc, at.v, at.i)));
        }
        if (levels) {
            // chunks: one lane per (vector, level-0 slot)
            for (uint64_t t = 0; t < (uint64_t)sc * sa; ++t) {
                const MsmBasisManyLane at = msm_basis_many_lane(t, sa, sc);
                if (at.v >= sc) continue;
                const uint32_t* li = longinfo_of(at.v);
                const MsmRunTask task = msm_run_task(li + 1, offsets_of(at.v), li[0], nkeys, nent, L, 0, at.i);
                if (task.some)
                    st(run_sum(at.v, (uint32_t)msm_key_window(c, task.key), task.lo, task.hi), run_a.at((uint64_t)at.v * sa + at.i));
            }
            for (int lv = 1; lv <= levels; ++lv) {
                const bool odd = lv & 1;
                Tracked& src = odd ? run_a : run_b;
                Tracked& dst = odd ? run_b : run_a;
                const uint32_t src_slots = odd ? sa : sb, dst_slots = lv == levels ? 0u : (odd ? sb : sa);
                const uint32_t slots = msm_level_slots(nent, nkeys, L, lv);
                for (uint64_t t = 0; t < (uint64_t)sc * slots; ++t) {
                    const MsmBasisManyLane at = msm_basis_many_lane(t, slots, sc);
                    if (at.v >= sc) continue;
                    const uint32_t* li = longinfo_of(at.v);
                    const MsmRunTask task = msm_run_task(li + 1, offsets_of(at.v), li[0], nkeys, nent, L, lv, at.i);
                    if (!task.some || task.hi > src_slots || (!task.last && at.i >= dst_slots)) continue;
                    const Jac<Fq> acc =
                        msm_fold_sum<Fq>([&](uint32_t i) { return ld(src.at((uint64_t)at.v * src_slots + i)); }, task.lo, task.hi);
                    st(acc, task.last ? buckets.at(msm_basis_many_bucket(c, sc, at.v, task.key))
                                      : dst.at((uint64_t)at.v * dst_slots + at.i));
                }
            }
        }
        // the collapse for all vectors at once, the reduction, the trees, the finish
        tree(buckets, nwin - 1, (uint64_t)sc * nb);
        for (uint64_t t = 0; t < (uint64_t)nseg * 2 * sc; ++t) {
            const MsmBasisManyPart at = msm_basis_many_part(t, sc);
            auto bucket = [&](uint32_t key) { return ld(buckets.at(msm_basis_many_bucket(c, sc, at.v, key))); };
            st(msm_segment_sum<Fq>(bucket, c, nkeys, at.s, msm_basis_reduce_window(c, at.which)), parts.at(t));
        }
        tree(parts, nseg, 2ull * sc);
        tree(parts, 2, sc);
        for (uint32_t v = 0; v < sc; ++v) st(msm_finish_point(ld(parts.at(v))), out + (size_t)(off + v) * PW);
    }
    for (int a = 0; a < 6; ++a) touched[a] = arrays[a]->hi;
    return 0;
}
}
