// msm_many_plan_main.cpp -- stand-alone checks of csrc/msm_many_plan.h (the refusals, the
// launch sets, the units and the words of bn_g1_msm_many), built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_msm_many_plan.py.  Prints "msm many plan ok" when
// every check holds.
#include "../../paritytech-bn_amd/csrc/msm_many_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

using namespace bn;

#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                \
        }                                                           \
    } while (0)

static const uint32_t kUnset = 0x7fffffffu;  // the value of no word

static std::vector<size_t> offsets_of(const std::vector<size_t>& sizes) {
    std::vector<size_t> off(1, 0);
    for (size_t s : sizes) off.push_back(off.back() + s);
    return off;
}
static MsmManyLimits limits(uint32_t unit, size_t max = 1024, size_t chunk = size_t(1) << 17,
                            size_t pack_long_from = SIZE_MAX) {
    return {unit, max, chunk, size_t(1) << 17, 16, pack_long_from};
}

// Every invariant of a plan and its words: the items cover the segments in order; a segment
// is alone exactly when it is longer than max; a packed set respects the chunk (but for a
// single segment) and is cut at segment boundaries; every term of a set lands in exactly one
// unit, of one segment; at most 64 units per segment and 64 terms per unit; the words
// written are exactly plan.words.
static void check_plan(const MsmManyLimits& lim, const std::vector<size_t>& off) {
    const size_t m = off.size() - 1;
    const MsmManyPlan plan = msm_many_plan(lim, off.data(), m);
    const size_t max = msm_many_effective_max(lim, off.data(), m);
    size_t nlong = 0;
    for (size_t s = 0; s < m; ++s) nlong += off[s + 1] - off[s] > lim.max ? 1 : 0;
    CHECK(max == (nlong >= lim.pack_long_from ? kMsmManyMaxSegment : (lim.max < 4096 ? lim.max : 4096)));
    std::vector<uint32_t> w(plan.words + 1, kUnset);  // an exact-size buffer: ASan watches its end
    msm_many_fill(plan, off.data(), w.data());
    CHECK(w[plan.words] == kUnset);
    for (size_t i = 0; i < plan.words; ++i) CHECK(w[i] != kUnset);
    size_t j = 0, words = 0;
    for (const MsmManyItem& it : plan.items) {
        CHECK(it.j0 == j && it.j1 > it.j0 && it.j1 <= m);
        j = it.j1;
        if (!it.packed) {
            CHECK(it.j1 == it.j0 + 1 && off[it.j1] - off[it.j0] > max);
            continue;
        }
        const size_t nt = off[it.j1] - off[it.j0];
        CHECK(it.j1 == it.j0 + 1 || nt <= lim.chunk);
        CHECK(it.j1 - it.j0 <= kMsmManyMaxSetSegments);
        CHECK(it.words_at == words);
        words += it.units + 1 + (it.j1 - it.j0) + 1;
        CHECK(it.T >= 1 && it.T <= kMsmManyMaxUnitTerms);
        if (lim.unit) CHECK(it.T == lim.unit);
        CHECK(nt <= plan.set_terms && it.units <= plan.set_units);
        const uint32_t* unit_off = w.data() + it.words_at;
        const uint32_t* seg_unit = unit_off + it.units + 1;
        CHECK(unit_off[0] == 0 && unit_off[it.units] == nt);
        CHECK(seg_unit[0] == 0 && seg_unit[it.j1 - it.j0] == it.units);
        for (size_t s = it.j0; s < it.j1; ++s) {
            const size_t len = off[s + 1] - off[s];
            CHECK(len <= max);
            const uint32_t u0 = seg_unit[s - it.j0], u1 = seg_unit[s - it.j0 + 1];
            CHECK(u0 <= u1 && u1 - u0 <= kMsmManyMaxUnits);
            CHECK((u1 == u0) == (len == 0));
            // the segment's units tile exactly its terms, in order
            CHECK(unit_off[u0] == off[s] - off[it.j0] && unit_off[u1] == off[s + 1] - off[it.j0]);
            size_t lo = len, hi = 0;
            for (uint32_t u = u0; u < u1; ++u) {
                const size_t cnt = unit_off[u + 1] - unit_off[u];
                CHECK(unit_off[u + 1] > unit_off[u] && cnt <= kMsmManyMaxUnitTerms);
                CHECK(cnt <= (it.T > (len + 63) / 64 ? it.T : (len + 63) / 64));
                lo = cnt < lo ? cnt : lo;
                hi = cnt > hi ? cnt : hi;
            }
            if (u1 > u0) CHECK(hi - lo <= 1);  // nearly equal
            if (len && len <= it.T) CHECK(u1 - u0 == 1);
        }
    }
    CHECK(j == m && words == plan.words);
}

static void test_refusals() {
    const size_t good[] = {0, 2, 2, 5};
    CHECK(msm_many_offsets_refusal(good, 3) == nullptr);
    CHECK(msm_many_offsets_refusal(good, 0) == nullptr);
    CHECK(msm_many_offsets_refusal(nullptr, 1) != nullptr);
    const size_t first[] = {1, 2};
    CHECK(std::string(msm_many_offsets_refusal(first, 1)) == "offsets[0] must be 0");
    const size_t down[] = {0, 3, 2, 5};
    CHECK(std::string(msm_many_offsets_refusal(down, 3)) == "offsets must not decrease");
    const size_t big[] = {0, kMsmManyMaxTerms + 1};
    CHECK(std::string(msm_many_offsets_refusal(big, 1)) == "more than 2^26 terms");
    const size_t edge[] = {0, kMsmManyMaxTerms};
    CHECK(msm_many_offsets_refusal(edge, 1) == nullptr);
    // m above the limit is refused before the array is read (one entry only here)
    const size_t one[] = {0};
    CHECK(std::string(msm_many_offsets_refusal(one, kMsmManyMaxTerms + 1)) == "more than 2^26 segments");
}

static void test_unit_cuts() {
    for (uint32_t T : {1u, 2u, 3u, 16u, 64u}) {
        std::vector<size_t> lens = {0, 1, T - 1, T, T + 1, 64 * (size_t)T, 64 * (size_t)T + 1, 4096};
        for (size_t len : lens) {
            if (len > 4096) continue;
            check_plan(limits(T, 4096), offsets_of({len}));
            const size_t t = msm_many_segment_unit(len, T);
            CHECK(t >= T && t <= 64 && msm_many_segment_units(len, T) <= 64);
            if (len <= 64 * (size_t)T) CHECK(t == T);
            CHECK(msm_many_segment_units(len, T) * t >= len);
        }
        check_plan(limits(T, 4096), offsets_of(lens));
        CHECK(msm_many_segment_units(64 * (size_t)T, T) == 64);
        if (64 * (size_t)T + 1 <= 4096) CHECK(msm_many_segment_unit(64 * (size_t)T + 1, T) == T + 1);
    }
    CHECK(msm_many_segment_unit(4096, 1) == 64 && msm_many_segment_units(4096, 1) == 64);
    // the automatic T: 1 up to the lane target, then the smallest that keeps the lanes, capped
    const MsmManyLimits a = limits(0);
    CHECK(msm_many_auto_unit(a, 0) == 1 && msm_many_auto_unit(a, 1) == 1 && msm_many_auto_unit(a, size_t(1) << 17) == 1);
    CHECK(msm_many_auto_unit(a, (size_t(1) << 17) + 1) == 2 && msm_many_auto_unit(a, size_t(1) << 19) == 4);
    CHECK(msm_many_auto_unit(a, size_t(1) << 26) == 16);
}

static void test_sets_and_routing() {
    // a forced small chunk: sets end at segment boundaries, a single segment may exceed it
    const MsmManyPlan p = msm_many_plan(limits(2, 1024, 8), offsets_of({4, 4, 4, 9, 1, 0, 0}).data(), 7);
    CHECK(p.items.size() == 4);
    CHECK(p.items[0].j0 == 0 && p.items[0].j1 == 2 && p.items[1].j1 == 3 && p.items[2].j1 == 4 && p.items[3].j1 == 7);
    for (const MsmManyItem& it : p.items) CHECK(it.packed);
    CHECK(p.set_terms == 9 && p.items[2].units == 5);
    check_plan(limits(2, 1024, 8), offsets_of({4, 4, 4, 9, 1, 0, 0}));
    // segments above max run alone, between packed sets
    const std::vector<size_t> off = offsets_of({3, 1025, 1024, 2000, 0});
    const MsmManyPlan q = msm_many_plan(limits(0, 1024), off.data(), 5);
    CHECK(q.items.size() == 5);
    CHECK(q.items[0].packed && !q.items[1].packed && q.items[2].packed && !q.items[3].packed && q.items[4].packed);
    check_plan(limits(0, 1024), off);
    const MsmManyPlan all = msm_many_plan(limits(0, 4096), off.data(), 5);
    CHECK(all.items.size() == 1 && all.items[0].packed);
    check_plan(limits(0, 4096), off);
    const MsmManyPlan none = msm_many_plan(limits(0, 0), offsets_of({1, 0, 2}).data(), 3);  // max 0: only empty ones pack
    CHECK(none.items.size() == 3 && !none.items[0].packed && none.items[1].packed && !none.items[2].packed);
    // from pack_long_from segments above max on, those of at most 4096 terms are packed too
    const std::vector<size_t> lng = offsets_of({2000, 5, 1025, 4097, 3000});
    const MsmManyPlan few = msm_many_plan(limits(0, 1024, size_t(1) << 17, 5), lng.data(), 5);   // four above max
    CHECK(few.items.size() == 5 && !few.items[0].packed && few.items[1].packed && !few.items[4].packed);
    const MsmManyPlan lots = msm_many_plan(limits(0, 1024, size_t(1) << 17, 4), lng.data(), 5);
    CHECK(lots.items.size() == 3 && lots.items[0].packed && lots.items[0].j1 == 3 && !lots.items[1].packed &&
          lots.items[2].packed);
    check_plan(limits(0, 1024, size_t(1) << 17, 4), lng);
    check_plan(limits(0, 1024, size_t(1) << 17, 5), lng);
    // no segments at all
    const size_t z[] = {0};
    CHECK(msm_many_plan(limits(0), z, 0).items.empty());
    // more empty segments than one set holds
    check_plan(limits(0), std::vector<size_t>(kMsmManyMaxSetSegments + 3, 0));
}

static void test_random() {
    std::mt19937 rng(8310);
    for (int round = 0; round < 200; ++round) {
        const size_t m = rng() % 40;
        std::vector<size_t> sizes(m);
        for (size_t& s : sizes) {
            const uint32_t kind = rng() % 8;
            s = kind == 0 ? 0 : kind == 1 ? rng() % 4097 : rng() % 70;
        }
        const uint32_t units[] = {0, 1, 2, 7, 16, 64};
        const size_t maxes[] = {0, 16, 1024, 4096};
        const size_t chunks[] = {1, 8, 64, 5000, size_t(1) << 17};
        const size_t froms[] = {0, 1, 3, SIZE_MAX};
        MsmManyLimits lim = {units[rng() % 6], maxes[rng() % 4], chunks[rng() % 5], size_t(1) << (rng() % 18), 16,
                             froms[rng() % 4]};
        check_plan(lim, offsets_of(sizes));
    }
}

int main() {
    test_refusals();
    test_unit_cuts();
    test_sets_and_routing();
    test_random();
    printf("msm many plan ok\n");
    return 0;
}
