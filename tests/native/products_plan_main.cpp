// products_plan_main.cpp -- stand-alone checks of csrc/products_plan.h (the planner, the
// refusals and the offset / map words of bn_pairing_batch_many and
// bn_pairing_batch_prepared_many), built with AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_products_plan.py.  Prints "products plan ok" when every check holds.
#include "../../paritytech-bn_amd/csrc/products_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
static ProductsPlan plan_of(const std::vector<size_t>& off, size_t products_min, size_t products_chunk,
                            const uint32_t* qidx = nullptr) {
    return products_plan({kChunk, kLaneMax, products_min, products_chunk}, off.data(), off.size() - 1, qidx);
}
struct Want {
    size_t j0, j1;
    bool packed;
};
static void check_items(const ProductsPlan& p, const std::vector<Want>& want) {
    CHECK(p.items.size() == want.size());
    for (size_t k = 0; k < want.size(); ++k) {
        CHECK(p.items[k].j0 == want[k].j0 && p.items[k].j1 == want[k].j1);
        CHECK(p.items[k].packed == want[k].packed);
    }
}

static void test_plans() {
    check_items(plan_of(offsets_of({4, 4, 65, 4}), 1, kChunk), {{0, 2, true}, {2, 3, false}, {3, 4, true}});
    // products_min: seven short products each alone, eight in one packed item
    const ProductsPlan seven = plan_of(offsets_of(std::vector<size_t>(7, 4)), 8, kChunk);
    CHECK(seven.items.size() == 7 && seven.off_words == 0);
    for (size_t k = 0; k < 7; ++k) CHECK(seven.items[k].j0 == k && seven.items[k].j1 == k + 1 && !seven.items[k].packed);
    check_items(plan_of(offsets_of(std::vector<size_t>(8, 4)), 8, kChunk), {{0, 8, true}});
    // products_chunk: a single product may exceed the chunk
    check_items(plan_of(offsets_of({4, 4, 4, 9, 1}), 1, 8), {{0, 2, true}, {2, 3, true}, {3, 4, true}, {4, 5, true}});
    // empty products
    const ProductsPlan many = plan_of(std::vector<size_t>(kChunk + 2, 0), 1, kChunk);
    check_items(many, {{0, kChunk, true}, {kChunk, kChunk + 1, true}});
    CHECK(many.items[1].off_at == kChunk + 1 && many.off_words == kChunk + 3);
    const ProductsPlan one = plan_of({0, 0}, 1, kChunk);
    check_items(one, {{0, 1, true}});
    uint32_t w[2] = {7, 7};
    products_fill(one, std::vector<size_t>{0, 0}.data(), nullptr, false, B, w, nullptr);
    CHECK(one.off_words == 2 && w[0] == 0 && w[1] == 0);
}

static void test_map() {
    const std::vector<size_t> off = offsets_of({4, 2});
    const uint32_t qidx[6] = {F, 2, F, 0, 1, F};
    const ProductsPlan p = plan_of(off, 1, kChunk, qidx);
    check_items(p, {{0, 2, true}});
    const ProductsItem& it = p.items[0];
    CHECK(it.nf == 3 && it.np == 3 && it.f0 == 0 && it.off_at == 0 && it.map_at == 0);
    CHECK(p.off_words == 3 && p.map_words == 18);
    for (int compact = 0; compact < 2; ++compact) {
        std::vector<uint32_t> ow(p.off_words, kUnset), mw(p.map_words, kUnset);
        products_fill(p, off.data(), qidx, compact != 0, B, ow.data(), mw.data());
        CHECK((ow == std::vector<uint32_t>{0, 4, 6}));
        const std::vector<uint32_t> pterm = compact ? std::vector<uint32_t>{3, 4, 5} : std::vector<uint32_t>{1, 3, 4};
        std::vector<uint32_t> want = {0, B | 0, 1, B | 1, B | 2, 2};  // the map: nt words
        want.insert(want.end(), pterm.begin(), pterm.end());         // pterm: np
        want.insert(want.end(), {2, 0, 1});                          // pidx: np
        want.insert(want.end(), {0, 2, 5});                          // fterm: nf
        // (a set has room for 3 nt words, an upper bound of the nt + 2 np + nf it uses)
        CHECK(want.size() <= mw.size() && std::equal(want.begin(), want.end(), mw.begin()));
    }
    // a second set starts where the first one's words end, its fresh points behind the first's
    const uint32_t q2[6] = {F, 2, F, 0, 1, F};
    const ProductsPlan two = plan_of(off, 1, 4, q2);
    check_items(two, {{0, 1, true}, {1, 2, true}});
    CHECK(two.items[1].off_at == 2 && two.items[1].map_at == 12 && two.items[1].f0 == 2);
    CHECK(two.items[1].nf == 1 && two.items[1].np == 1 && two.off_words == 4 && two.map_words == 18);
}

static void test_refusals() {
    const size_t bad0[3] = {1, 2, 3}, dec[4] = {0, 3, 2, 4}, good[3] = {0, 2, 4};
    CHECK(!strcmp(products_offsets_refusal(nullptr, 2), "null offsets"));
    CHECK(!strcmp(products_offsets_refusal(bad0, 2), "offsets[0] must be 0"));
    CHECK(!strcmp(products_offsets_refusal(dec, 3), "offsets must not decrease"));
    CHECK(products_offsets_refusal(good, 2) == nullptr);
    size_t nf = 0;
    const std::vector<size_t> big = offsets_of({4, 65});
    const std::vector<uint32_t> qbig(69, 0);
    CHECK(!strcmp(products_terms_refusal(qbig.data(), big.data(), 2, kLaneMax, 3, &nf),
                  "a product of more than 64 terms; use bn_pairing_batch"));
    const uint32_t qi[4] = {0, F, 3, 2};
    CHECK(!strcmp(products_terms_refusal(qi, good, 2, kLaneMax, 3, &nf), "prepared-point index out of range"));
    CHECK(products_terms_refusal(qi, good, 2, kLaneMax, 4, &nf) == nullptr && nf == 1);
}

static void test_sweep() {
    std::mt19937 rng(20240607);
    auto upto = [&](size_t hi) { return (size_t)(rng() % (hi + 1)); };
    for (int round = 0; round < 200; ++round) {
        const size_t m = 1 + upto(39);
        const bool prepared = round % 2 == 1;  // every product packed: sizes within the lane maximum
        std::vector<size_t> sizes(m);
        for (size_t& s : sizes) s = upto(prepared ? kLaneMax : 70);
        const std::vector<size_t> off = offsets_of(sizes);
        const size_t pmin = upto(12), pchunk = 1 + upto(300);
        std::vector<uint32_t> qidx(prepared ? off[m] : 0);
        for (uint32_t& q : qidx) q = rng() % 3 ? (uint32_t)(rng() % 5) : F;
        const ProductsPlan p = plan_of(off, pmin, pchunk, prepared ? qidx.data() : nullptr);
        std::vector<uint32_t> ow(p.off_words, kUnset), mw(p.map_words, kUnset);
        products_fill(p, off.data(), prepared ? qidx.data() : nullptr, round % 4 == 1, B, ow.data(), mw.data());
        size_t next = 0, off_words = 0, map_words = 0, f0 = 0;
        for (const ProductsItem& it : p.items) {
            CHECK(it.j0 == next && it.j1 > it.j0 && it.j1 <= m);  // the items tile [0, m) in order
            next = it.j1;
            const size_t nt = off[it.j1] - off[it.j0];
            if (!it.packed) {
                CHECK(!prepared && it.j1 == it.j0 + 1);
                continue;
            }
            CHECK(it.j1 - it.j0 <= kChunk);
            for (size_t j = it.j0; j < it.j1; ++j) CHECK(off[j + 1] - off[j] <= kLaneMax);
            CHECK(nt <= pchunk || it.j1 == it.j0 + 1);
            CHECK(it.off_at == off_words);
            CHECK(ow[it.off_at] == 0 && ow[it.off_at + (it.j1 - it.j0)] == nt);
            off_words += it.j1 - it.j0 + 1;
            if (prepared) {
                CHECK(it.nf + it.np == nt && it.f0 == f0 && it.map_at == map_words);
                for (size_t t = 0; t < 2 * nt + it.np; ++t) CHECK(mw[it.map_at + t] != kUnset);  // its words written
                f0 += it.nf;
                map_words += 3 * nt;
            }
        }
        CHECK(next == m && off_words == p.off_words && map_words == p.map_words);
        for (uint32_t w : ow) CHECK(w != kUnset);  // every offset word written
    }
}

int main() {
    test_plans();
    test_map();
    test_refusals();
    test_sweep();
    printf("products plan ok\n");
    return 0;
}
