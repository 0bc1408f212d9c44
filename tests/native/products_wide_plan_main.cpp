// products_wide_plan_main.cpp -- stand-alone checks of the wide path's part of
// csrc/products_plan.h: that the plan without the wide limits is the plan of
// the rules before it, the routing rule of both product calls on each side of each of its
// conditions, the cuts of the wide sets and the gather words.  Built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_products_wide_plan.py.  Prints
// "products wide plan ok" when every check holds.
#include "../../paritytech-bn_amd/csrc/products_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>

using namespace bn;

#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                \
        }                                                           \
    } while (0)

static const size_t kChunk = size_t(1) << 18, kLaneMax = 64;
static const uint32_t F = BN_QIDX_FRESH, B = 0x80000000u;
static const uint32_t kUnset = 0x7fffffffu;  // the value of no offset or map word

static std::vector<size_t> offsets_of(const std::vector<size_t>& sizes) {
    std::vector<size_t> off(1, 0);
    for (size_t s : sizes) off.push_back(off.back() + s);
    return off;
}
static std::vector<size_t> repeat(const std::vector<size_t>& v, size_t k) {
    std::vector<size_t> r;
    for (size_t i = 0; i < k; ++i) r.insert(r.end(), v.begin(), v.end());
    return r;
}

// ---- the rules before the wide path, written out again: short products (at most 64 terms)
// are packed when the form is the prepared one or there are at least products_min of them
// (and at least one); a packed set grows while it stays within `chunk` products and
// products_chunk terms; everything else is one product alone.  A set of the prepared form has
// three map words per term.
struct OldItem {
    size_t j0, j1;
    bool packed;
    size_t off_at, nf, np, f0, map_at;
};
struct OldPlan {
    std::vector<OldItem> items;
    size_t off_words = 0, map_words = 0;
};
static OldPlan old_plan(size_t products_min, size_t products_chunk, const std::vector<size_t>& off,
                        const uint32_t* qidx) {
    const size_t m = off.size() - 1;
    auto len = [&](size_t j) { return off[j + 1] - off[j]; };
    size_t nshort = 0;
    for (size_t j = 0; j < m; ++j) nshort += len(j) <= kLaneMax;
    const bool pack = qidx || (nshort > 0 && nshort >= products_min);
    OldPlan plan;
    size_t f0 = 0, j = 0;
    while (j < m) {
        if (!pack || len(j) > kLaneMax) {
            plan.items.push_back({j, j + 1, false, 0, 0, 0, 0, 0});
            ++j;
            continue;
        }
        size_t e = j + 1;
        for (; e < m; ++e)
            if (e - j >= kChunk || len(e) > kLaneMax || off[e + 1] - off[j] > products_chunk) break;
        size_t nf = 0;
        for (size_t i = off[j]; qidx && i < off[e]; ++i) nf += qidx[i] == F;
        plan.items.push_back({j, e, true, plan.off_words, nf, off[e] - off[j] - nf, f0, plan.map_words});
        f0 += nf;
        plan.off_words += e - j + 1;
        plan.map_words += qidx ? 3 * (off[e] - off[j]) : 0;
        j = e;
    }
    return plan;
}
static void check_same(const ProductsPlan& p, const OldPlan& o) {
    CHECK(p.items.size() == o.items.size() && p.off_words == o.off_words && p.map_words == o.map_words);
    for (size_t k = 0; k < o.items.size(); ++k) {
        const ProductsItem& a = p.items[k];
        const OldItem& b = o.items[k];
        CHECK(!a.wide && a.alone() == !b.packed);
        CHECK(a.j0 == b.j0 && a.j1 == b.j1 && a.packed == b.packed && a.off_at == b.off_at);
        CHECK(a.nf == b.nf && a.np == b.np && a.f0 == b.f0 && a.map_at == b.map_at);
    }
}
static std::vector<uint32_t> some_qidx(size_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<uint32_t> q(n);
    for (uint32_t& x : q) x = rng() % 3 ? (uint32_t)(rng() % 5) : F;
    return q;
}

// wide off: the limits left out (the four-field initialisation of the callers before the
// path), wide_max 0 with a latency limit, and a latency limit of 0 with a wide_max
static void test_off_is_unchanged() {
    std::vector<std::vector<size_t>> lists = {
        {4, 4, 65, 4}, std::vector<size_t>(7, 4), std::vector<size_t>(8, 4), {4, 4, 4, 9, 1}, {0},
        {0, 0, 0}, {5}, {64}, {65}, {2, 65, 1, 0, 4, 200, 3, 64, 0}, {30, 30, 10, 64, 0, 1, 2, 5, 56, 0, 3, 60, 4, 0, 33, 0},
        {4, 2}, repeat({0, 1, 2, 5, 0, 3, 1, 64, 1}, 5), std::vector<size_t>(kChunk + 2, 0)};
    std::mt19937 rng(20240911);
    for (int r = 0; r < 60; ++r) {
        std::vector<size_t> s(1 + rng() % 40);
        for (size_t& x : s) x = rng() % 71;
        lists.push_back(s);
    }
    const size_t mins[] = {0, 1, 8, 12}, chunks[] = {1, 4, 8, 64, 300, kChunk};
    for (const std::vector<size_t>& sizes : lists) {
        const std::vector<size_t> off = offsets_of(sizes);
        const size_t m = sizes.size();
        const bool shorts = *std::max_element(sizes.begin(), sizes.end()) <= kLaneMax;
        const std::vector<uint32_t> qidx = some_qidx(off[m], (uint32_t)m);
        for (size_t pmin : mins)
            for (size_t pchunk : chunks) {
                if (m > 1000 && pchunk != kChunk) continue;  // (the 2^18 empty products: once per products_min)
                for (int prepared = 0; prepared <= (shorts ? 1 : 0); ++prepared) {
                    const uint32_t* q = prepared ? qidx.data() : nullptr;
                    const OldPlan want = old_plan(pmin, pchunk, off, q);
                    check_same(products_plan({kChunk, kLaneMax, pmin, pchunk}, off.data(), m, q), want);
                    check_same(products_plan({kChunk, kLaneMax, pmin, pchunk, 0, 4096}, off.data(), m, q), want);
                    check_same(products_plan({kChunk, kLaneMax, pmin, pchunk, 1 << 20, 0}, off.data(), m, q), want);
                }
            }
    }
}

struct Want {
    size_t j0, j1;
    int kind;  // 0 wide, 1 packed, 2 alone
};
static void check_items(const ProductsPlan& p, const std::vector<Want>& want) {
    CHECK(p.items.size() == want.size());
    for (size_t k = 0; k < want.size(); ++k) {
        const ProductsItem& it = p.items[k];
        CHECK(it.j0 == want[k].j0 && it.j1 == want[k].j1);
        CHECK(!(it.wide && it.packed));
        CHECK((it.wide ? 0 : it.packed ? 1 : 2) == want[k].kind);
    }
}
static ProductsPlan plan_of(const std::vector<size_t>& sizes, size_t pmin, size_t pchunk, size_t wide_max,
                            size_t latency_max, const uint32_t* qidx = nullptr) {
    const std::vector<size_t> off = offsets_of(sizes);
    return products_plan({kChunk, kLaneMax, pmin, pchunk, wide_max, latency_max}, off.data(), sizes.size(), qidx);
}

static void test_fresh_routing() {
    const size_t L = 4096;
    // the path: seven products, below products_min, in one wide set
    check_items(plan_of(std::vector<size_t>(7, 4), 8, kChunk, 4096, L), {{0, 7, 0}});
    // ... and at or above products_min as well, while the terms are within wide_max
    check_items(plan_of(std::vector<size_t>(8, 4), 8, kChunk, 4096, L), {{0, 8, 0}});
    // products_min == 0: every short product packed, as documented
    check_items(plan_of(std::vector<size_t>(7, 4), 0, kChunk, 4096, L), {{0, 7, 1}});
    // one eligible product stays on the single-product path, two are a wide set
    check_items(plan_of({5}, 8, kChunk, 4096, L), {{0, 1, 2}});
    check_items(plan_of({5, 70}, 8, kChunk, 4096, L), {{0, 1, 2}, {1, 2, 2}});
    check_items(plan_of({5, 70}, 1, kChunk, 4096, L), {{0, 1, 1}, {1, 2, 2}});  // (products_min 1: packed, as before)
    check_items(plan_of({5, 0}, 8, kChunk, 4096, L), {{0, 2, 0}});
    check_items(plan_of({5, 70, 3}, 8, kChunk, 4096, L), {{0, 1, 0}, {1, 2, 2}, {2, 3, 0}});
    // the eligible products' terms at wide_max, and one above: the plan before the path
    check_items(plan_of(std::vector<size_t>(10, 4), 8, kChunk, 40, L), {{0, 10, 0}});
    check_items(plan_of(std::vector<size_t>(10, 4), 8, kChunk, 39, L), {{0, 10, 1}});
    check_items(plan_of(std::vector<size_t>(7, 4), 8, kChunk, 27, L), {{0, 1, 2}, {1, 2, 2}, {2, 3, 2}, {3, 4, 2},
                                                                       {4, 5, 2}, {5, 6, 2}, {6, 7, 2}});
    // (a long product's terms do not count: 8 + 200 terms, wide_max 8)
    check_items(plan_of({4, 200, 4}, 8, kChunk, 8, L), {{0, 1, 0}, {1, 2, 2}, {2, 3, 0}});
    // a 65-term product inside a wide call runs alone and ends a set
    const ProductsPlan mid = plan_of({2, 64, 65, 1, 0}, 8, kChunk, 4096, L);
    check_items(mid, {{0, 2, 0}, {2, 3, 2}, {3, 5, 0}});
    CHECK(mid.items[0].off_at == 0 && mid.items[2].off_at == 3 && mid.off_words == 6 && mid.map_words == 0);
    // W below 64: W = min(latency_max, products_chunk) terms at most are eligible
    check_items(plan_of({16, 17, 16, 3}, 8, kChunk, 4096, 16), {{0, 1, 0}, {1, 2, 2}, {2, 3, 0}, {3, 4, 0}});
    check_items(plan_of({16, 17, 16, 3}, 8, 16, 4096, L), {{0, 1, 0}, {1, 2, 2}, {2, 3, 0}, {3, 4, 0}});
    check_items(plan_of({17, 17, 3}, 8, kChunk, 4096, 16), {{0, 1, 2}, {1, 2, 2}, {2, 3, 2}});  // one eligible
    // W == 0: off, also for empty products
    check_items(plan_of({0, 0}, 8, kChunk, 4096, 0), {{0, 1, 2}, {1, 2, 2}});
}

static void test_prepared_routing() {
    const std::vector<size_t> sizes = {4, 4, 64, 0};
    const std::vector<uint32_t> q = some_qidx(72, 7);
    check_items(plan_of(sizes, 8, kChunk, 72, 4096, q.data()), {{0, 4, 0}});
    check_items(plan_of(sizes, 0, kChunk, 72, 4096, q.data()), {{0, 4, 0}});    // products_min does not apply
    check_items(plan_of(sizes, 8, kChunk, 71, 4096, q.data()), {{0, 4, 1}});    // n above wide_max
    check_items(plan_of(sizes, 8, kChunk, 0, 4096, q.data()), {{0, 4, 1}});     // off
    check_items(plan_of(sizes, 8, kChunk, 4096, 63, q.data()), {{0, 4, 1}});    // W below 64
    check_items(plan_of(sizes, 8, 63, 4096, 4096, q.data()), {{0, 2, 1}, {2, 3, 1}, {3, 4, 1}});
    check_items(plan_of(sizes, 8, 64, 4096, 4096, q.data()), {{0, 2, 0}, {2, 4, 0}});  // W == 64
    // one product, and one empty product
    check_items(plan_of({4}, 8, kChunk, 4096, 4096, q.data()), {{0, 1, 0}});
    check_items(plan_of({0}, 8, kChunk, 4096, 4096, q.data()), {{0, 1, 0}});
}

static void test_cuts() {
    // at W terms: a product that would straddle the cut starts the next set, one of exactly W
    // terms fills a set, empty products sit at the cuts (with the set in front of them)
    const std::vector<size_t> sizes = {3, 3, 2, 0, 8, 0, 0, 5, 4, 0};
    check_items(plan_of(sizes, 8, 8, 4096, 4096), {{0, 4, 0}, {4, 7, 0}, {7, 8, 0}, {8, 10, 0}});
    check_items(plan_of(sizes, 8, kChunk, 4096, 8), {{0, 4, 0}, {4, 7, 0}, {7, 8, 0}, {8, 10, 0}});
    const ProductsPlan p = plan_of(sizes, 8, 8, 4096, 4096);
    const std::vector<size_t> off = offsets_of(sizes);
    std::vector<uint32_t> ow(p.off_words, kUnset);
    products_fill(p, off.data(), nullptr, false, B, ow.data(), nullptr);
    CHECK((ow == std::vector<uint32_t>{0, 3, 6, 8, 8, 0, 8, 8, 8, 0, 5, 0, 4, 4}));
    // at kChunk products: 2^18 + 2 empty products, then one of a term
    std::vector<size_t> many(kChunk + 2, 0);
    many.push_back(1);
    const ProductsPlan big = plan_of(many, 8, kChunk, 4096, 4096);
    check_items(big, {{0, kChunk, 0}, {kChunk, kChunk + 3, 0}});
    CHECK(big.items[1].off_at == kChunk + 1 && big.off_words == kChunk + 5);
    // invariants over seeded random calls that take the path
    std::mt19937 rng(20240912);
    for (int round = 0; round < 200; ++round) {
        const size_t m = 2 + rng() % 40, W = 1 + rng() % 100, elig = std::min(W, kLaneMax);
        const bool prepared = round % 2 == 1 && W >= kLaneMax;
        std::vector<size_t> s(m);
        for (size_t& x : s) x = rng() % (prepared ? 65 : 71);
        s[0] = std::min(s[0], elig), s[1] = std::min(s[1], elig);  // two eligible products
        const std::vector<size_t> o = offsets_of(s);
        const std::vector<uint32_t> q = some_qidx(o[m], (uint32_t)round);
        const ProductsPlan pl = plan_of(s, 1 + rng() % 12, round % 3 ? kChunk : W, 1 << 20, round % 3 ? W : 4096,
                                        prepared ? q.data() : nullptr);
        std::vector<uint32_t> w(pl.off_words, kUnset), mw(pl.map_words, kUnset);
        products_fill(pl, o.data(), prepared ? q.data() : nullptr, false, B, w.data(), mw.data());
        if (prepared) products_wide_fill(pl, o.data(), q.data(), B, mw.data());
        size_t next = 0, off_words = 0, map_words = 0, f0 = 0;
        for (const ProductsItem& it : pl.items) {
            CHECK(it.j0 == next && it.j1 > it.j0 && it.j1 <= m && !it.packed);
            next = it.j1;
            const size_t nt = o[it.j1] - o[it.j0];
            if (!it.wide) {
                CHECK(it.j1 == it.j0 + 1 && nt > elig);
                continue;
            }
            CHECK(nt <= W && it.off_at == off_words && w[it.off_at] == 0 && w[it.off_at + it.j1 - it.j0] == nt);
            for (size_t j = it.j0; j < it.j1; ++j) CHECK(o[j + 1] - o[j] <= elig);
            // greedy: the next product, if eligible, did not fit
            if (it.j1 < m && o[it.j1 + 1] - o[it.j1] <= elig) CHECK(o[it.j1 + 1] - o[it.j0] > W);
            off_words += it.j1 - it.j0 + 1;
            if (prepared) {
                CHECK(it.nf + it.np == nt && it.f0 == f0 && it.map_at == map_words);
                f0 += it.nf;
                map_words += nt;
            }
        }
        CHECK(next == m && off_words == pl.off_words && map_words == pl.map_words);
        for (uint32_t x : w) CHECK(x != kUnset);
        for (uint32_t x : mw) CHECK(x != kUnset);
    }
}

static void test_gather_words() {
    // two sets (W = 64 cuts after the second product): fresh indices restart per set, f0 moves on
    const std::vector<size_t> sizes = {4, 60, 3};
    std::vector<uint32_t> q(67, 1);
    q[0] = F, q[1] = 2, q[2] = F, q[3] = 0;       // product 0: fresh, 2, fresh, 0
    q[4] = F, q[63] = F;                          // product 1: fresh first and last, point 1 between
    q[64] = 4, q[65] = F, q[66] = F;              // product 2, the second set
    const ProductsPlan p = plan_of(sizes, 8, 64, 4096, 4096, q.data());
    check_items(p, {{0, 2, 0}, {2, 3, 0}});
    CHECK(p.items[0].nf == 4 && p.items[0].np == 60 && p.items[0].f0 == 0 && p.items[0].map_at == 0);
    CHECK(p.items[1].nf == 2 && p.items[1].np == 1 && p.items[1].f0 == 4 && p.items[1].map_at == 64);
    CHECK(p.map_words == 67 && p.off_words == 5);
    const std::vector<size_t> off = offsets_of(sizes);
    std::vector<uint32_t> ow(p.off_words, kUnset), mw(p.map_words, kUnset);
    products_fill(p, off.data(), q.data(), false, B, ow.data(), mw.data());
    for (uint32_t x : mw) CHECK(x == kUnset);  // a wide set has no packed map words
    CHECK((ow == std::vector<uint32_t>{0, 4, 64, 0, 3}));
    products_wide_fill(p, off.data(), q.data(), B, mw.data());
    std::vector<uint32_t> want = {0, B | 2, 1, B | 0, 2};
    want.insert(want.end(), 58, B | 1);
    want.insert(want.end(), {3, B | 4, 0, 1});
    CHECK(mw == want);
    // a packed plan of the same call is left alone by products_wide_fill
    const ProductsPlan pk = plan_of(sizes, 8, 64, 0, 4096, q.data());
    std::vector<uint32_t> none(pk.map_words, kUnset);
    products_wide_fill(pk, off.data(), q.data(), B, none.data());
    for (uint32_t x : none) CHECK(x == kUnset);
}

int main() {
    test_off_is_unchanged();
    test_fresh_routing();
    test_prepared_routing();
    test_cuts();
    test_gather_words();
    printf("products wide plan ok\n");
    return 0;
}
