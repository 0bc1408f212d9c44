// msm_many_plan.h -- the host-side planning of bn_g1_msm_many (capi_msm.hip; DESIGN.md
// §8d): the refusals of its offsets, which segments share a launch set of the packed path
// and which run alone, the cut of every packed segment into units, and the words a set's
// kernels read.  Pure: the standard library only, every limit passed in, so it runs (and is
// tested) without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#pragma GCC visibility push(hidden)  // nothing here is part of the library's interface
namespace bn {

constexpr size_t kMsmManyMaxTerms = size_t(1) << 26;     // n and m of a call
constexpr size_t kMsmManyMaxSegment = 4096;              // the longest packed segment
constexpr uint32_t kMsmManyMaxUnits = 64;                // units (partial sums) per segment
constexpr uint32_t kMsmManyMaxUnitTerms = 64;            // terms per unit
constexpr size_t kMsmManyMaxSetSegments = size_t(1) << 20;  // segments per launch set
constexpr int kMsmManyMinWindow = 2, kMsmManyMaxWindow = 8;  // the digits are stored as bytes

struct MsmManyLimits {
    uint32_t unit;     // bn_set_msm_many_unit: terms per unit, 1 .. 64; 0: chosen per set (lanes, unit_auto_max)
    size_t max;        // bn_set_msm_many_max: longer segments run alone; at most kMsmManyMaxSegment
    size_t chunk;      // the most terms of a launch set (a single segment may exceed it); >= 1
    size_t lanes;      // automatic units: the lanes a set should give the card
    uint32_t unit_auto_max;  // ... and the most terms per unit the automatic choice takes
    // a call with at least this many segments above max packs those of at most
    // kMsmManyMaxSegment terms too (many long segments fill the card, a few run faster
    // alone); SIZE_MAX: never
    size_t pack_long_from;
};

// One item of a call's work, segments [j0, j1).  packed: one launch set -- the table kernel
// over its terms, the unit kernel over its `units` units of at most T terms (longer
// segments: max(T, ceil(len / 64))), the finish kernel over its segments; its words start
// at words_at: units + 1 set-relative term offsets of the units (they tile the set's terms
// in order), then j1 - j0 + 1 unit offsets of the segments.  Otherwise j1 == j0 + 1: one
// segment above the call's effective max on the single-MSM path.
struct MsmManyItem {
    size_t j0, j1;
    bool packed;
    uint32_t T;
    size_t units, words_at;
};
struct MsmManyPlan {
    std::vector<MsmManyItem> items;
    size_t words = 0;                          // of all packed items
    size_t set_terms = 0, set_units = 0;       // the largest of any packed item
};

// offsets: m + 1 host entries, non-decreasing from 0, m and offsets[m] at most 2^26.  The
// refusal's message, or null.  m is checked before offsets is read.
inline const char* msm_many_offsets_refusal(const size_t* off, size_t m) {
    if (m > kMsmManyMaxTerms) return "more than 2^26 segments";
    if (!off) return "null offsets";
    if (off[0] != 0) return "offsets[0] must be 0";
    for (size_t j = 0; j < m; ++j) {
        if (off[j + 1] < off[j]) return "offsets must not decrease";
        if (off[j + 1] > kMsmManyMaxTerms) return "more than 2^26 terms";
    }
    return nullptr;
}

// terms per unit of a segment of len terms at the set's T: at most 64 units, and at most 64
// terms each for len <= kMsmManyMaxSegment
inline uint32_t msm_many_segment_unit(size_t len, uint32_t T) {
    const size_t floor = (len + kMsmManyMaxUnits - 1) / kMsmManyMaxUnits;
    return (uint32_t)(floor > T ? floor : T);
}
inline size_t msm_many_segment_units(size_t len, uint32_t T) {
    const size_t t = msm_many_segment_unit(len, T);
    return (len + t - 1) / t;
}
// The automatic T of a launch set of nt terms: the smallest that keeps the set's lanes at
// the target (with few terms T = 1: the shortest chain), at most unit_auto_max.
inline uint32_t msm_many_auto_unit(const MsmManyLimits& lim, size_t nt) {
    const size_t lanes = lim.lanes ? lim.lanes : 1;
    const size_t t = (nt + lanes - 1) / lanes;
    const size_t cap = lim.unit_auto_max ? lim.unit_auto_max : 1;
    return (uint32_t)(t < 1 ? 1 : (t > cap ? cap : t));
}

// the longest segment the call packs: lim.max, or kMsmManyMaxSegment when the call has
// pack_long_from or more segments above lim.max
inline size_t msm_many_effective_max(const MsmManyLimits& lim, const size_t* off, size_t m) {
    const size_t max = lim.max < kMsmManyMaxSegment ? lim.max : kMsmManyMaxSegment;
    size_t nlong = 0;
    for (size_t j = 0; j < m; ++j) nlong += off[j + 1] - off[j] > max ? 1 : 0;
    return nlong >= lim.pack_long_from ? kMsmManyMaxSegment : max;
}

// The caller has checked the offsets.  Sets are cut at segment boundaries.
inline MsmManyPlan msm_many_plan(const MsmManyLimits& lim, const size_t* off, size_t m) {
    MsmManyPlan plan;
    const size_t max = msm_many_effective_max(lim, off, m);
    const size_t chunk = lim.chunk ? lim.chunk : 1;
    for (size_t j = 0; j < m;) {
        if (off[j + 1] - off[j] > max) {
            plan.items.push_back({j, j + 1, false, 0, 0, 0});
            ++j;
            continue;
        }
        size_t e = j + 1;
        while (e < m && e - j < kMsmManyMaxSetSegments && off[e + 1] - off[e] <= max && off[e + 1] - off[j] <= chunk) ++e;
        const size_t nt = off[e] - off[j];
        uint32_t T = lim.unit ? lim.unit : msm_many_auto_unit(lim, nt);
        if (T > kMsmManyMaxUnitTerms) T = kMsmManyMaxUnitTerms;
        size_t units = 0;
        for (size_t s = j; s < e; ++s) units += msm_many_segment_units(off[s + 1] - off[s], T);
        plan.items.push_back({j, e, true, T, units, plan.words});
        plan.words += (units + 1) + (e - j + 1);
        if (nt > plan.set_terms) plan.set_terms = nt;
        if (units > plan.set_units) plan.set_units = units;
        j = e;
    }
    return plan;
}

// The words of every packed item into w (plan.words of them).  A segment's units are of
// nearly equal size: the first len % units of them have one term more.
inline void msm_many_fill(const MsmManyPlan& plan, const size_t* off, uint32_t* w) {
    for (const MsmManyItem& it : plan.items) {
        if (!it.packed) continue;
        uint32_t* unit_off = w + it.words_at;
        uint32_t* seg_unit = unit_off + it.units + 1;
        size_t u = 0, t = 0;
        for (size_t s = it.j0; s < it.j1; ++s) {
            seg_unit[s - it.j0] = (uint32_t)u;
            const size_t len = off[s + 1] - off[s];
            const size_t nu = msm_many_segment_units(len, it.T);
            for (size_t i = 0; i < nu; ++i) {
                unit_off[u++] = (uint32_t)t;
                t += len / nu + (i < len % nu ? 1 : 0);
            }
        }
        unit_off[u] = (uint32_t)t;
        seg_unit[it.j1 - it.j0] = (uint32_t)u;
    }
}

}  // namespace bn
#pragma GCC visibility pop
