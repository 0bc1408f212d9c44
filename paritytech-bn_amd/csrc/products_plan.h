// products_plan.h -- the host-side planning of bn_pairing_batch_many and
// bn_pairing_batch_prepared_many (capi_products.hip): which
// products share a launch set, the refusals of the control arrays, and the offset and
// map words a set's kernels read.  Pure: the standard library and the public header
// only, every limit passed in, so it runs (and is tested) without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/bn254mi.h"

#pragma GCC visibility push(hidden)  // nothing here is part of the library's interface
namespace bn {

struct ProductsLimits {
    size_t chunk;           // kChunk: the most products of a launch set
    size_t lane_max;        // kProductLaneMax: the most terms of a packed product
    size_t products_min;    // bn_set_products_min
    size_t products_chunk;  // bn_set_products_chunk: the most terms of a launch set
    // the wide path; a limit left out means "wide path off"
    size_t wide_max = 0;     // bn_set_products_wide_max: the most terms of a call that takes it
    size_t latency_max = 0;  // bn_set_latency_max: the most pairs of one k_pairing_latency launch
};

// One unit of a call's work, products [j0, j1).  packed: one launch set of the packed
// path -- the producers over its terms, k_miller_products(_mapped) (a lane pair per
// product), the final exponentiation over its products; every product has at most
// lane_max terms, together at most products_chunk (a single product may exceed that), and
// there are at most `chunk` products.  Its j1 - j0 + 1 set-relative offset words start at
// off_at.  Otherwise j1 == j0 + 1: one product on the single-product path.
// With prepared terms (qidx) a set has nf fresh terms (the call's fresh terms f0 .. f0 +
// nf - 1, which is where their points start in the compacted q) and np prepared ones, and
// its map words start at map_at: the term map (nf + np words), the prepared slots' terms
// and table indices (np each), the fresh slots' terms (nf).
// wide (never with packed): one launch set of the wide path (§6d) -- k_pairing_latency's
// Miller values of its terms, k_fq12_products_wide (a 16-lane group per product), the final
// exponentiation; at most products_wide_terms(lim) terms, cut at product boundaries, and at
// most `chunk` products.  Its offset words are a packed set's; with qidx its map words are
// the nf + np gather words of products_wide_fill.
struct ProductsItem {
    size_t j0, j1;
    bool packed;
    size_t off_at;
    size_t nf, np, f0, map_at;
    bool wide = false;
    bool alone() const { return !packed && !wide; }
};
struct ProductsPlan {
    std::vector<ProductsItem> items;
    size_t off_words = 0, map_words = 0;
};

// W: the most terms of a wide set -- one k_pairing_latency launch within a launch set's terms
inline size_t products_wide_terms(const ProductsLimits& lim) {
    const size_t w = lim.latency_max < lim.products_chunk ? lim.latency_max : lim.products_chunk;
    return w < lim.chunk ? w : lim.chunk;
}
// The wide path's plan of a call it takes (products_plan decides that): every product of at
// most `elig` terms in wide sets, cut at product boundaries at W terms and `chunk` products;
// every other product (the plain form only) alone, which ends the set in front of it.
inline ProductsPlan products_plan_wide(const ProductsLimits& lim, const size_t* off, size_t m, const uint32_t* qidx,
                                       size_t elig) {
    const size_t W = products_wide_terms(lim);
    ProductsPlan plan;
    size_t f0 = 0;
    for (size_t j = 0; j < m;) {
        if (off[j + 1] - off[j] > elig) {
            plan.items.push_back({j, j + 1, false, 0, 0, 0, 0, 0});
            ++j;
            continue;
        }
        size_t e = j + 1;
        while (e < m && e - j < lim.chunk && off[e + 1] - off[e] <= elig && off[e + 1] - off[j] <= W) ++e;
        const size_t nt = off[e] - off[j];
        size_t nf = 0;
        if (qidx)
            for (size_t i = off[j]; i < off[e]; ++i) nf += qidx[i] == BN_QIDX_FRESH ? 1 : 0;
        plan.items.push_back({j, e, false, plan.off_words, nf, nt - nf, f0, plan.map_words, true});
        f0 += nf;
        plan.off_words += e - j + 1;
        if (qidx) plan.map_words += nt;
        j = e;
    }
    return plan;
}

// qidx: the prepared form, where every product is packed (its check has refused products
// above lane_max).  Without it, calls with fewer than products_min short products run each
// alone (a lone two-lane chain takes milliseconds where the single-product path's 16-lane
// groups take 0.8 ms), and so does every product above lane_max.
// The wide path (wide_max > 0) comes first.  The prepared form takes it with every product
// when W >= lane_max (so every product fits a set) and the call has at most wide_max terms.
// The plain form takes it when products_min != 0 (0 keeps its meaning: every short product
// packed), W > 0, and the products of at most min(lane_max, W) terms are at least two (one
// alone is the same kernels on the single-product path) of together at most wide_max terms;
// the others run alone.  In every other case the plan is the one described above.
inline ProductsPlan products_plan(const ProductsLimits& lim, const size_t* off, size_t m, const uint32_t* qidx) {
    const size_t W = products_wide_terms(lim);
    if (lim.wide_max > 0 && W > 0) {
        if (qidx) {
            if (W >= lim.lane_max && off[m] <= lim.wide_max) return products_plan_wide(lim, off, m, qidx, lim.lane_max);
        } else if (lim.products_min != 0) {
            const size_t elig = lim.lane_max < W ? lim.lane_max : W;
            size_t count = 0, terms = 0;
            for (size_t j = 0; j < m; ++j)
                if (off[j + 1] - off[j] <= elig) ++count, terms += off[j + 1] - off[j];
            if (count >= 2 && terms <= lim.wide_max) return products_plan_wide(lim, off, m, nullptr, elig);
        }
    }
    bool pack = qidx != nullptr;
    if (!pack) {
        size_t nshort = 0;
        for (size_t j = 0; j < m; ++j) nshort += off[j + 1] - off[j] <= lim.lane_max ? 1 : 0;
        pack = nshort > 0 && nshort >= lim.products_min;
    }
    ProductsPlan plan;
    size_t f0 = 0;
    for (size_t j = 0; j < m;) {
        if (!pack || off[j + 1] - off[j] > lim.lane_max) {
            plan.items.push_back({j, j + 1, false, 0, 0, 0, 0, 0});
            ++j;
            continue;
        }
        size_t e = j + 1;
        while (e < m && e - j < lim.chunk && off[e + 1] - off[e] <= lim.lane_max &&
               off[e + 1] - off[j] <= lim.products_chunk)
            ++e;
        const size_t nt = off[e] - off[j];
        size_t nf = 0;
        if (qidx)
            for (size_t i = off[j]; i < off[e]; ++i) nf += qidx[i] == BN_QIDX_FRESH ? 1 : 0;
        plan.items.push_back({j, e, true, plan.off_words, nf, nt - nf, f0, plan.map_words});
        f0 += nf;
        plan.off_words += e - j + 1;
        if (qidx) plan.map_words += 3 * nt;
        j = e;
    }
    return plan;
}

// offsets: m + 1 host entries, non-decreasing from 0.  The refusal's message, or null.
inline const char* products_offsets_refusal(const size_t* off, size_t m) {
    if (!off) return "null offsets";
    if (off[0] != 0) return "offsets[0] must be 0";
    for (size_t j = 0; j < m; ++j)
        if (off[j + 1] < off[j]) return "offsets must not decrease";
    return nullptr;
}
// the prepared form's terms: no product above lane_max, every index fresh or below the
// handle's nq points; *nf = the call's fresh terms
inline const char* products_terms_refusal(const uint32_t* qidx, const size_t* off, size_t m, size_t lane_max, size_t nq,
                                          size_t* nf) {
    for (size_t j = 0; j < m; ++j)
        if (off[j + 1] - off[j] > lane_max) return "a product of more than 64 terms; use bn_pairing_batch";
    *nf = 0;
    for (size_t i = 0; i < off[m]; ++i) {
        if (qidx[i] == BN_QIDX_FRESH) ++*nf;
        else if (qidx[i] >= nq) return "prepared-point index out of range";
    }
    return nullptr;
}

// The words of every packed item: its set-relative 32-bit offsets into off_w (a wide item's
// too) and, with qidx, its term words into map_w (region_b: kMapRegionB, the mark of a prepared slot).
// compact_p: the host form stages a set's G1 points fresh first, then prepared, so
// prepared slot k's term is nf + k; otherwise terms are the caller's, set-relative.
inline void products_fill(const ProductsPlan& plan, const size_t* off, const uint32_t* qidx, bool compact_p,
                          uint32_t region_b, uint32_t* off_w, uint32_t* map_w) {
    for (const ProductsItem& it : plan.items) {
        if (it.alone()) continue;
        const size_t lo = off[it.j0], nt = off[it.j1] - lo;
        for (size_t j = it.j0; j <= it.j1; ++j) off_w[it.off_at + (j - it.j0)] = (uint32_t)(off[j] - lo);
        if (!qidx || it.wide) continue;
        uint32_t* map = map_w + it.map_at;
        uint32_t* pterm = map + nt;
        uint32_t* pidx = pterm + it.np;
        uint32_t* fterm = pidx + it.np;
        size_t kf = 0, kp = 0;
        for (size_t t = 0; t < nt; ++t) {
            const uint32_t qi = qidx[lo + t];
            if (qi == BN_QIDX_FRESH) {
                fterm[kf] = (uint32_t)t;
                map[t] = (uint32_t)kf++;
            } else {
                pterm[kp] = (uint32_t)(compact_p ? it.nf + kp : t);
                pidx[kp] = qi;
                map[t] = region_b | (uint32_t)kp++;
            }
        }
    }
}

// The gather words of every wide item of the prepared form, one per term in term order
// (k_g2_gather): a fresh term's is its index among the set's fresh terms (its point in the
// compacted q from f0 on), a prepared term's is `mark` plus its table index.
inline void products_wide_fill(const ProductsPlan& plan, const size_t* off, const uint32_t* qidx, uint32_t mark,
                               uint32_t* map_w) {
    for (const ProductsItem& it : plan.items) {
        if (!it.wide) continue;
        const size_t lo = off[it.j0], nt = off[it.j1] - lo;
        uint32_t kf = 0;
        for (size_t t = 0; t < nt; ++t) {
            const uint32_t qi = qidx[lo + t];
            map_w[it.map_at + t] = qi == BN_QIDX_FRESH ? kf++ : mark | qi;
        }
    }
}

}  // namespace bn
#pragma GCC visibility pop
