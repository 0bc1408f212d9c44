// ctx_mem_main.cpp -- stand-alone checks of the types that own a context's device and pinned
// memory (csrc/ctx_mem.h, through csrc/ctx.h), built by tests/test_ctx_mem.py with
// AddressSanitizer + UndefinedBehaviorSanitizer against tests/native/fakehip (allocations
// backed by malloc, counted; the k-th can be made to fail), so the failure paths that a GPU
// reaches only when starved of memory run here.  Prints "ctx mem ok" when every check holds.
#include "../../paritytech-bn_amd/csrc/ctx.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>

using namespace bn;
namespace fh = fakehip;

#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                \
        }                                                           \
    } while (0)

static size_t mark() { return fh::calls.size(); }
// a drain is the one stream synchronize of ws_drain (the context here has nothing pending)
static int drains(size_t from) { return fh::count("hipStreamSynchronize", from); }
static bool nothing_live() { return fh::dev.empty() && fh::pin.empty() && fh::events.empty() && fh::streams.empty(); }

static void test_grow() {
    bn_ctx c;
    DevBuf<uint32_t> b;
    // nothing to drain for a first buffer; the floor applies
    size_t t = mark();
    CHECK(b.grow(&c, 10, 64) == BN_OK && b.cap() == 64 && b.get() && fh::dev.size() == 1);
    CHECK(drains(t) == 0 && fh::count("hipMalloc", t) == 1 && fh::count("hipFree", t) == 0);
    // at or below the capacity: no HIP call at all
    t = mark();
    CHECK(b.grow(&c, 64, 4096) == BN_OK && b.grow(&c, 1) == BN_OK && b.grow(&c, 0, 0, true) == BN_OK);
    CHECK(mark() == t && b.cap() == 64);
    // past it: drained because there was a buffer, the old one freed before the new one is made
    uint32_t* old = b;
    t = mark();
    CHECK(b.grow(&c, 65) == BN_OK && b.cap() == 65 && fh::dev.size() == 1 && !fh::dev.count(old));
    CHECK(mark() == t + 3 && std::string(fh::calls[t]) == "hipStreamSynchronize" &&
          std::string(fh::calls[t + 1]) == "hipFree" && std::string(fh::calls[t + 2]) == "hipMalloc");
    for (size_t i = 0; i < 65; ++i) b[i] = (uint32_t)i;  // all of it is there
    // drain_always drains for a first buffer too
    DevBuf<bn_g1> p;
    t = mark();
    CHECK(p.grow(&c, 3, 4096, true) == BN_OK && p.cap() == 4096 && drains(t) == 1);
    // a pinned buffer never drains
    PinBuf<uint8_t> h;
    t = mark();
    CHECK(h.grow(&c, 8) == BN_OK && h.grow(&c, 9) == BN_OK && h.cap() == 9 && drains(t) == 0 && fh::pin.size() == 1);
    CHECK(fh::count("hipHostMalloc", t) == 2 && fh::count("hipHostFree", t) == 1 && fh::count("hipMalloc", t) == 0);
    // moving leaves the source empty: one owner, one free
    DevBuf<uint32_t> m(std::move(b));
    CHECK(!b.get() && b.cap() == 0 && m.cap() == 65 && fh::dev.size() == 2);
}

static void test_grow_failure() {
    bn_ctx c;
    DevBuf<uint32_t> b;
    CHECK(b.grow(&c, 8) == BN_OK);
    fh::fail_alloc_in = 1;
    size_t t = mark();
    CHECK(b.grow(&c, 16) == BN_ERR_HIP);
    CHECK(c.err.find("hipMalloc") != std::string::npos && c.err.find("out of memory") != std::string::npos);
    CHECK(!b.get() && b.cap() == 0 && fh::dev.empty() && fh::count("hipFree", t) == 1);
    // the next grow succeeds, with nothing old to drain or free
    t = mark();
    CHECK(b.grow(&c, 16) == BN_OK && b.cap() == 16 && fh::dev.size() == 1);
    CHECK(drains(t) == 0 && fh::count("hipFree", t) == 0);
    PinBuf<uint32_t> h;
    fh::fail_alloc_in = 1;
    CHECK(h.grow(&c, 4) == BN_ERR_HIP && c.err.find("hipHostMalloc") != std::string::npos && !h.get() && h.cap() == 0);
    CHECK(h.grow(&c, 4) == BN_OK && fh::pin.size() == 1);
}

// bn::reserve's rule (grow_together): each of its four allocations failing in turn
static void test_reserve_failure() {
    const size_t per[4] = {3, 5, 7, 2};
    for (int k = 1; k <= 4; ++k) {
        bn_ctx c;
        auto reserve = [&](size_t n) {
            return grow_together(&c, &c.cap, n, 1024, per, c.coeffs, c.paff, c.slots, c.flags);
        };
        size_t t = mark();
        CHECK(reserve(1) == BN_OK && c.cap == 1024 && fh::dev.size() == 4 && drains(t) == 0);  // the floor; no workspace yet
        CHECK(c.coeffs.cap() == 3 * 1024 && c.paff.cap() == 5 * 1024 && c.slots.cap() == 7 * 1024 && c.flags.cap() == 2 * 1024);
        t = mark();
        CHECK(reserve(1024) == BN_OK && mark() == t);
        fh::fail_alloc_in = k;
        t = mark();
        CHECK(reserve(2000) == BN_ERR_HIP && c.cap == 0 && c.err.find("hipMalloc") != std::string::npos);
        CHECK(drains(t) == 1 && fh::count("hipFree", t) == 4 && fh::count("hipMalloc", t) == k);
        // the k - 1 that succeeded are held by their members, and by nothing else
        const size_t held = (c.coeffs ? 1 : 0) + (c.paff ? 1 : 0) + (c.slots ? 1 : 0) + (c.flags ? 1 : 0);
        CHECK(held == (size_t)k - 1 && fh::dev.size() == held);
        t = mark();
        CHECK(reserve(1) == BN_OK && c.cap == 1024 && fh::dev.size() == 4);  // the next call: the floor again
        CHECK(fh::count("hipFree", t) == k - 1 && drains(t) == 0);  // (capacity 0: there was no workspace to drain)
        CHECK(reserve(2000) == BN_OK && c.cap == 2000 && c.slots.cap() == 7 * 2000 && fh::dev.size() == 4);
    }
    CHECK(nothing_live());
}

static void test_channel_and_fence() {
    bn_ctx c;
    UploadChannel a, b;  // two channels under one fence, as the products'
    Fence f;
    const int e0 = fh::events_created;
    size_t t = mark();
    CHECK(a.grow(&c, f, 0) == BN_OK && mark() == t && !a.cap);  // no words: nothing at all
    CHECK(a.grow(&c, f, 10) == BN_OK && a.cap == 4096 && a.h.cap() == 4096 && a.d.cap() == 4096);
    CHECK(b.grow(&c, f, 5000) == BN_OK && b.cap == 5000);
    CHECK(fh::count("hipEventSynchronize", t) == 0 && fh::events_created == e0 + 1 && !f.pending());
    for (size_t i = 0; i < 4096; ++i) a.h[i] = (uint32_t)i;
    CHECK(a.copy(&c, 4096, nullptr) == BN_OK && f.record(&c, nullptr) == BN_OK && f.pending());
    CHECK(a.d[4095] == 4095);
    // the next call: one wait while the copy is pending, none after it
    t = mark();
    CHECK(a.grow(&c, f, 10) == BN_OK && b.grow(&c, f, 10) == BN_OK && f.wait(&c) == BN_OK);
    CHECK(mark() == t + 1 && std::string(fh::calls[t]) == "hipEventSynchronize" && !f.pending());
    // growing a pending channel waits first, then drains, then replaces both buffers
    CHECK(f.record(&c, nullptr) == BN_OK);
    t = mark();
    CHECK(a.grow(&c, f, 4097) == BN_OK && a.cap == 4097 && a.h.cap() == 4097 && a.d.cap() == 4097);
    CHECK(std::string(fh::calls[t]) == "hipEventSynchronize" && std::string(fh::calls[t + 1]) == "hipStreamSynchronize" &&
          fh::count("hipEventSynchronize", t) == 1 && drains(t) == 1);
    CHECK(fh::events_created == e0 + 1 && fh::events.size() == 1);  // created once
    // either allocation failing leaves capacity 0, and the next call rebuilds both
    for (int k = 1; k <= 2; ++k) {
        fh::fail_alloc_in = k;
        CHECK(a.grow(&c, f, 9000) == BN_ERR_HIP && a.cap == 0);
        CHECK(a.grow(&c, f, 10) == BN_OK && a.cap == 4096 && a.h.cap() == 4096 && a.d.cap() == 4096);
        CHECK(fh::dev.size() == 2 && fh::pin.size() == 2);
    }
}

static void test_handles() {
    bn_ctx c;
    HandleList<bn_g1_basis>& list = c.g1_basis;
    bn_g1_basis foreign;
    bn_g1_basis* gone = nullptr;
    CHECK(!list.live(nullptr) && !list.live(&foreign));
    // a build that fails half way: the handle is dropped behind a stream synchronize, nothing stays
    {
        auto h = std::make_unique<bn_g1_basis>();
        CHECK(h->table.alloc(&c, 8) == BN_OK);
        fh::fail_alloc_in = 1;
        const int rc = h->zero.alloc(&c, 4);
        CHECK(rc == BN_ERR_HIP && fh::dev.size() == 1);
        bn_g1_basis* out = nullptr;
        const size_t t = mark();
        CHECK(list.settle(&c, std::move(h), rc, true, nullptr, &out) == BN_ERR_HIP && !out);
        CHECK(std::string(fh::calls[t]) == "hipStreamSynchronize" && std::string(fh::calls.back()) == "hipFree");
        CHECK(fh::dev.empty());
    }
    // a build that succeeds: the host form waits once, the _dev form not at all
    for (bool wait : {true, false}) {
        auto h = std::make_unique<bn_g1_basis>();
        CHECK(h->table.alloc(&c, 8) == BN_OK && h->zero.alloc(&c, 4) == BN_OK);
        bn_g1_basis* out = nullptr;
        const size_t t = mark();
        CHECK(list.settle(&c, std::move(h), BN_OK, wait, nullptr, &out) == BN_OK && out && list.live(out));
        CHECK(fh::count("hipStreamSynchronize", t) == (wait ? 1 : 0));
        gone = out;
    }
    CHECK(fh::dev.size() == 4);
    // destroy: refused with the caller's words when not live; drained before anything is freed
    CHECK(list.destroy(&c, &foreign, "not one of mine") == BN_ERR_INVALID_ARGUMENT && c.err == "not one of mine");
    CHECK(list.destroy(&c, nullptr, "null") == BN_ERR_INVALID_ARGUMENT);
    size_t t = mark();
    CHECK(list.destroy(&c, gone, "") == BN_OK && fh::dev.size() == 2);
    CHECK(std::string(fh::calls[t]) == "hipStreamSynchronize" && fh::count("hipFree", t) == 2);
    // the destroyed handle is looked up, not read (the sanitizer would report a read of it)
    t = mark();
    CHECK(!list.live(gone) && list.destroy(&c, gone, "destroyed") == BN_ERR_INVALID_ARGUMENT && mark() == t);
    // the one still alive goes with the context
}

// a context with every buffer grown to one element and a handle of each kind, destroyed the
// way capi.hip's ctx_teardown does it
static void test_full_context() {
    bn_ctx* c = new bn_ctx();
    for (hipStream_t* s : {&c->stream, &c->h2d, &c->d2h}) CHECK(hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess);
    for (hipEvent_t* e : {&c->ws_event, &c->ev_in[0], &c->ev_in[1], &c->ev_comp[0], &c->ev_comp[1], &c->ev_out[0], &c->ev_out[1]})
        CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess);
    hipEvent_t pooled = nullptr;
    CHECK(hipEventCreateWithFlags(&pooled, 0) == hipSuccess);
    c->ev_pool.push_back(pooled);
    const size_t per[4] = {1, 1, 1, 1};
    CHECK(grow_together(c, &c->cap, 1, 0, per, c->coeffs, c->paff, c->slots, c->flags) == BN_OK);
    CHECK(c->d_prog.alloc(c, 1) == BN_OK && c->d_err.alloc(c, 1) == BN_OK && c->tail_ws.alloc(c, 1) == BN_OK &&
          c->fe_ds_ws.alloc(c, 1) == BN_OK);
    CHECK(c->stage.grow(c, 1) == BN_OK && c->pin.grow(c, 1) == BN_OK);
    CHECK(c->msm_keys.grow(c, 1) == BN_OK && c->msm_sorted.grow(c, 1) == BN_OK);
    auto group = [&](auto& g) {
        return g.buckets.grow(c, 1) == BN_OK && g.parts.grow(c, 1) == BN_OK && g.tmp.grow(c, 1) == BN_OK &&
               g.run_a.grow(c, 1) == BN_OK && g.run_b.grow(c, 1) == BN_OK && g.fixed.grow(c, 1) == BN_OK;
    };
    CHECK(group(c->msm_g1) && group(c->msm_g2));
    CHECK(c->prod_off.grow(c, c->prod_fence, 1) == BN_OK && c->prod_map.grow(c, c->prod_fence, 1) == BN_OK);
    CHECK(c->prod_fresh.grow(c, 1) == BN_OK && c->prod_gq.grow(c, 1) == BN_OK);
    CHECK(c->many_digits.grow(c, 1) == BN_OK && c->many_table.grow(c, 1) == BN_OK && c->many_parts.grow(c, 1) == BN_OK);
    CHECK(c->many_words.grow(c, c->many_fence, 1) == BN_OK);
    CHECK(c->prod_fence.record(c, c->stream) == BN_OK && c->many_fence.record(c, c->stream) == BN_OK);
    auto g2 = std::make_unique<bn_g2_prepared>();
    CHECK(g2->table.alloc(c, 1) == BN_OK && g2->zero.alloc(c, 1) == BN_OK && g2->points.alloc(c, 1) == BN_OK);
    auto g1 = std::make_unique<bn_g1_prepared>();
    CHECK(g1->table.alloc(c, 1) == BN_OK && g1->zero.alloc(c, 1) == BN_OK);
    auto gb = std::make_unique<bn_g1_basis>();
    CHECK(gb->table.alloc(c, 1) == BN_OK && gb->zero.alloc(c, 1) == BN_OK);
    CHECK(c->prepared.adopt(std::move(g2)) && c->g1_prepared.adopt(std::move(g1)) && c->g1_basis.adopt(std::move(gb)));
    CHECK(fh::dev.size() == 4 + 4 + 1 + 2 + 12 + 2 + 2 + 3 + 1 + 7 && fh::pin.size() == 4 && fh::events.size() == 10);
    // ctx_teardown's ordered part, then delete
    for (hipStream_t s : {c->stream, c->h2d, c->d2h}) (void)hipStreamSynchronize(s);
    for (hipEvent_t e : {c->ws_event, c->ev_in[0], c->ev_in[1], c->ev_comp[0], c->ev_comp[1], c->ev_out[0], c->ev_out[1]})
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    for (hipStream_t s : {c->h2d, c->d2h, c->stream}) (void)hipStreamDestroy(s);
    delete c;
    CHECK(nothing_live());
}

int main() {
    test_grow();
    CHECK(nothing_live());
    test_grow_failure();
    CHECK(nothing_live());
    test_reserve_failure();
    test_channel_and_fence();
    CHECK(nothing_live());
    test_handles();
    CHECK(nothing_live());
    test_full_context();
    // a parent multi-device context owns no device memory: deleting it makes no HIP call
    const size_t t = mark();
    delete new bn_ctx();
    CHECK(mark() == t);
    printf("ctx mem ok\n");
    return 0;
}
