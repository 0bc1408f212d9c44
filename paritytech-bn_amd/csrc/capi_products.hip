// capi_products.hip -- host side of the C ABI's pairing products and prepared G2 points:
// bn_pairing_batch_many, the bn_g2_prepared handles with
// bn_pairing_prepared_many (§6b), bn_pairing_batch_prepared_many (§6c), and the wide path of
// both product calls for calls too small to fill the GPU (§6d).  The plain and
// the prepared products share one plan (products_plan.h), one upload of its words, one
// workspace rule, one launch tail and one host loop; they differ in the producers in front
// of the products' loop and in the loop's kernel.
#include <algorithm>
#include <vector>

#include "capi_internal.h"
#include "products_plan.h"

using namespace bn;

static ProductsLimits products_limits(const bn_ctx* c) {
    return {kChunk, (size_t)kProductLaneMax, c->products_min, c->products_chunk, c->products_wide_max, c->latency_max};
}
// a call's plan, its products counted by route for bn_get_products_routes
static ProductsPlan products_plan_counted(bn_ctx* c, const size_t* off, size_t m, const uint32_t* qidx) {
    ProductsPlan plan = products_plan(products_limits(c), off, m, qidx);
    for (const ProductsItem& it : plan.items) c->products_routes[it.wide ? 0 : it.packed ? 1 : 2] += it.j1 - it.j0;
    return plan;
}
static int offsets_check(bn_ctx* c, const size_t* off, size_t m) {
    if (const char* why = products_offsets_refusal(off, m)) return fail(c, BN_ERR_INVALID_ARGUMENT, why);
    return BN_OK;
}
// the workspace for every item of the call: the larger of a launch set's terms (coeffs,
// flags) and products (slots); a lone product's chunk
static int products_reserve(bn_ctx* c, const size_t* off, const ProductsPlan& plan) {
    size_t need = 1;
    for (const ProductsItem& it : plan.items) {
        const size_t nt = off[it.j1] - off[it.j0];
        need = std::max(need, it.alone() ? std::min(nt, kChunk) : std::max(nt, it.j1 - it.j0));
    }
    return reserve(c, need);
}
// The words of every launch set of the call (products_fill) -> prod_off.d and, with qidx,
// prod_map.d, in one copy each on s in front of the call's kernels.  The pinned sources are
// rewritten by the next call, which first waits for these copies (one fence for both; not
// for the kernels behind them).  The caller has ordered s after the workspace's previous user.
static int products_upload(bn_ctx* c, const ProductsPlan& plan, const size_t* off, const uint32_t* qidx,
                           bool compact_p, hipStream_t s) {
    if (!plan.off_words) return BN_OK;
    RET_IF(c->prod_off.grow(c, c->prod_fence, plan.off_words));
    RET_IF(c->prod_map.grow(c, c->prod_fence, plan.map_words));
    products_fill(plan, off, qidx, compact_p, kMapRegionB, c->prod_off.h, c->prod_map.h);
    if (qidx) products_wide_fill(plan, off, qidx, kMapRegionB, c->prod_map.h);
    RET_IF(c->prod_off.copy(c, plan.off_words, s));
    if (plan.map_words) RET_IF(c->prod_map.copy(c, plan.map_words, s));
    return c->prod_fence.record(c, s);
}
// the tail of a launch set: the products' loop over the workspace's coefficients
// (loop(grid, block) launches it, a lane pair per product), then the final exponentiation
// of its mc values -> d_out[0 .. mc)
template <class Loop>
static int products_loop_fe(bn_ctx* c, size_t mc, bn_gt* d_out, hipStream_t s, Loop&& loop) {
    const size_t lanes = kPathLanes * mc;
    const unsigned block = products_block(c, lanes);
    loop((unsigned)((lanes + block - 1) / block), block);
    HIPCHK(c, hipGetLastError());
    return run_fe(c, c->slots, mc, nullptr, d_out, nullptr, s);
}
// one launch set: the nt device pairs at d_p / d_q, mc products cut by d_off (mc + 1
// device words) -> d_out[0 .. mc)
static int products_set_dev(bn_ctx* c, const bn_g1* d_p, const bn_g2* d_q, size_t nt, const uint32_t* d_off, size_t mc,
                            bn_gt* d_out, hipStream_t s) {
    if (nt > c->cap || mc > c->cap) return fail(c, BN_ERR_INTERNAL, "launch set exceeds the workspace");
    // only Gt leaves: the producers on scaled inputs (no pair at all: nothing to prepare)
    if (nt) RET_IF(prepare(c, d_p, d_q, nt, 0, s, 1, true));
    return products_loop_fe(c, mc, d_out, s, [&](unsigned grid, unsigned block) {
        k_miller_products<<<grid, block, 0, s>>>(c->coeffs, c->flags, nt, d_off, mc, c->slots);
    });
}
// one launch set with prepared terms: the nf fresh pairs at d_pf / d_qf through the
// producers into region A of the workspace, the np prepared terms (G1 points
// d_pp[pterm[k]]) through k_prepared_expand into region B behind it, then the tail
static int prepared_set_dev(bn_ctx* c, const ProductsItem& st, const bn_g1* d_pf, const bn_g2* d_qf,
                            const bn_g1* d_pp, const bn_g2_prepared* h, bn_gt* d_out, hipStream_t s) {
    const size_t nf = st.nf, np = st.np, mc = st.j1 - st.j0;
    if (nf + np > c->cap || mc > c->cap) return fail(c, BN_ERR_INTERNAL, "launch set exceeds the workspace");
    const uint32_t* map = c->prod_map.d + st.map_at;
    if (nf) RET_IF(prepare(c, d_pf, d_qf, nf, 0, s, 1, true));
    if (np) {
        launch_prepared_expand(d_pp, map + nf + np, map + nf + 2 * np, h->table, h->zero, (uint32_t)h->nq, np,
                               c->coeffs + nf * (size_t)kCoeffFq * 9, c->flags + kPathLanes * nf, s);
        HIPCHK(c, hipGetLastError());
    }
    return products_loop_fe(c, mc, d_out, s, [&](unsigned grid, unsigned block) {
        k_miller_products_mapped<<<grid, block, 0, s>>>(c->coeffs, c->flags, nf, np, map, c->prod_off.d + st.off_at, mc,
                                                        c->slots);
    });
}
// one launch set of the wide path: the Miller values of the nt device pairs
// from one k_pairing_latency launch (a pair with a zero point comes out as one), a 16-lane
// group per product over them into slot 0, then the packed path's tail
static int wide_set_dev(bn_ctx* c, const bn_g1* d_p, const bn_g2* d_q, size_t nt, const uint32_t* d_off, size_t mc,
                        bn_gt* d_out, hipStream_t s) {
    if (nt > c->cap || mc > c->cap) return fail(c, BN_ERR_INTERNAL, "launch set exceeds the workspace");
    uint32_t* f = nullptr;
    RET_IF(latency_values(c, d_p, d_q, nt, s, &f));
    constexpr size_t kGroups = kBlock / 16;
    k_fq12_products_wide<<<(unsigned)((mc + kGroups - 1) / kGroups), kBlock, 0, s>>>(f, nt, nt, d_off, mc, c->slots);
    HIPCHK(c, hipGetLastError());
    return run_fe(c, c->slots, mc, nullptr, d_out, nullptr, s);
}
// the same with prepared terms: the set's G2 points gathered in term order into prod_gq (the
// caller has grown it) from its nf fresh points at d_qf and the handle's points; d_p in term order
static int wide_prepared_set_dev(bn_ctx* c, const ProductsItem& st, const bn_g1* d_p, const bn_g2* d_qf,
                                 const bn_g2_prepared* h, bn_gt* d_out, hipStream_t s) {
    const size_t nt = st.nf + st.np;
    if (nt > c->prod_gq.cap()) return fail(c, BN_ERR_INTERNAL, "launch set exceeds the gathered points");
    if (nt) {
        launch_g2_gather(d_qf, st.nf, h->points, (uint32_t)h->nq, c->prod_map.d + st.map_at, nt, c->prod_gq, s);
        HIPCHK(c, hipGetLastError());
    }
    return wide_set_dev(c, d_p, c->prod_gq, nt, c->prod_off.d + st.off_at, st.j1 - st.j0, d_out, s);
}
// prod_gq for the largest wide set of a plan of the prepared form
static int wide_gather_reserve(bn_ctx* c, const ProductsPlan& plan) {
    size_t ntmax = 0;
    for (const ProductsItem& st : plan.items)
        if (st.wide) ntmax = std::max(ntmax, st.nf + st.np);
    return c->prod_gq.grow(c, ntmax, 4096, true);
}
// The host forms: every item in turn through the context's stage.  run_set stages a packed
// (or wide) item's pairs and its products' Gt, copies the pairs in and runs the set, leaving the
// device rows in *d; an item alone (the plain form only: p and q are the caller's pairs)
// goes through batch_host, which clears the outcome word for its own product.  The device
// outcome is read after each item, BN_ERR_FE_ZERO reported at the end with every row written.
template <class RunSet>
static int products_host_loop(bn_ctx* c, const ProductsPlan& plan, const bn_g1* p, const bn_g2* q, const size_t* off,
                              bn_gt* out, RunSet&& run_set) {
    int zero = 0;
    for (const ProductsItem& it : plan.items) {
        if (it.alone()) {
            const size_t lo = off[it.j0], nt = off[it.j1] - lo;
            if (nt == 0) {  // mod.rs:922-924
                gt_one(out + it.j0);
                continue;
            }
            const int rc = batch_host(c, p + lo, q + lo, nt, 0, true, out + it.j0);
            if (rc == BN_ERR_FE_ZERO) zero = kBitFeZero;
            else if (rc) return rc;
            continue;
        }
        RET_IF(clear_err(c, c->stream));
        bn_gt* d = nullptr;
        RET_IF(run_set(it, &d));
        HIPCHK(c, hipMemcpyAsync(out + it.j0, d, (it.j1 - it.j0) * sizeof(bn_gt), hipMemcpyDeviceToHost, c->stream));
        int bits = 0;
        RET_IF(check_err(c, c->stream, &bits));  // synchronizes: the stage is reused
        zero |= bits;
    }
    return outcome(c, zero, kBitFeZero);
}

extern "C" {

// ---- many products in one call (bn_pairing_batch_many)
// offsets first; then the buffers (n = offsets[m])
static int products_check(bn_ctx* c, const void* p, const void* q, const size_t* off, size_t m, const void* out) {
    RET_IF(offsets_check(c, off, m));
    if (!out || (off[m] && (!p || !q))) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    return BN_OK;
}
int bn_pairing_batch_many_dev(bn_ctx* c, const bn_g1* d_p, const bn_g2* d_q, const size_t* offsets, size_t m,
                              bn_gt* d_out, void* stream) {
    CTX_GUARD(c);
    if (m == 0) return BN_OK;
    RET_IF(products_check(c, d_p, d_q, offsets, m, d_out));
    const hipStream_t s = pick(c, stream);
    const ProductsPlan plan = products_plan_counted(c, offsets, m, nullptr);
    RET_IF(products_reserve(c, offsets, plan));
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    RET_IF(products_upload(c, plan, offsets, nullptr, false, s));
    for (const ProductsItem& it : plan.items) {
        const size_t lo = offsets[it.j0], nt = offsets[it.j1] - lo;
        if (it.wide)
            RET_IF(wide_set_dev(c, d_p + lo, d_q + lo, nt, c->prod_off.d + it.off_at, it.j1 - it.j0, d_out + it.j0, s));
        else if (it.packed)
            RET_IF(products_set_dev(c, d_p + lo, d_q + lo, nt, c->prod_off.d + it.off_at, it.j1 - it.j0, d_out + it.j0, s));
        else if (nt == 0)  // mod.rs:922-924
            HIPCHK(c, hipMemcpyAsync(d_out + it.j0, &kGtOne, sizeof(bn_gt), hipMemcpyHostToDevice, s));
        else
            RET_IF(miller_product_dev(c, d_p + lo, d_q + lo, nt, 0, d_out + it.j0, s));
    }
    return BN_OK;
}
int bn_pairing_batch_many(bn_ctx* c, const bn_g1* p, const bn_g2* q, const size_t* offsets, size_t m, bn_gt* out) {
    if (is_multi(c)) return bn_multi_pairing_batch_many(c, p, q, offsets, m, out);
    CTX_GUARD_HOST(c);
    if (m == 0) return BN_OK;
    RET_IF(products_check(c, p, q, offsets, m, out));
    const ProductsPlan plan = products_plan_counted(c, offsets, m, nullptr);
    RET_IF(products_reserve(c, offsets, plan));
    RET_IF(products_upload(c, plan, offsets, nullptr, false, c->stream));
    return products_host_loop(c, plan, p, q, offsets, out, [&](const ProductsItem& it, bn_gt** d) -> int {
        const size_t lo = offsets[it.j0], nt = offsets[it.j1] - lo, mc = it.j1 - it.j0;
        void* at[3];
        RET_IF(stage_regions(c, {nt * sizeof(bn_g1), nt * sizeof(bn_g2), mc * sizeof(bn_gt)}, at));
        if (nt) {
            HIPCHK(c, hipMemcpyAsync(at[0], p + lo, nt * sizeof(bn_g1), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(at[1], q + lo, nt * sizeof(bn_g2), hipMemcpyHostToDevice, c->stream));
        }
        *d = (bn_gt*)at[2];
        return (it.wide ? wide_set_dev : products_set_dev)(c, (bn_g1*)at[0], (bn_g2*)at[1], nt,
                                                           c->prod_off.d + it.off_at, mc, *d, c->stream);
    });
}
int bn_set_products_min(bn_ctx* c, size_t m) {
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_products_min(d, m); });
    CTX_GUARD(c);
    c->products_min = m;
    return BN_OK;
}
int bn_set_products_wide_max(bn_ctx* c, size_t terms) {
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_products_wide_max(d, terms); });
    CTX_GUARD(c);
    c->products_wide_max = terms;
    return BN_OK;
}
int bn_get_products_routes(bn_ctx* c, size_t counts[3]) {
    if (!c || !counts) return BN_ERR_INVALID_ARGUMENT;
    if (is_multi(c)) {
        size_t sum[3] = {0, 0, 0};
        RET_IF(for_each_sub(c, [&](bn_ctx* d) -> int {
            size_t one[3];
            RET_IF(bn_get_products_routes(d, one));
            for (int k = 0; k < 3; ++k) sum[k] += one[k];
            return BN_OK;
        }));
        for (int k = 0; k < 3; ++k) counts[k] = sum[k];
        return BN_OK;
    }
    CTX_GUARD(c);
    for (int k = 0; k < 3; ++k) {
        counts[k] = c->products_routes[k];
        c->products_routes[k] = 0;
    }
    return BN_OK;
}
int bn_set_products_chunk(bn_ctx* c, size_t terms) {
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_products_chunk(d, terms); });
    CTX_GUARD(c);
    if (terms > kChunk) return fail(c, BN_ERR_INVALID_ARGUMENT, "at most kChunk terms per launch set");
    c->products_chunk = terms ? terms : kChunk;
    return BN_OK;
}

// ---------------------------------------------------------------- prepared G2 points
// Fills a new handle with the coefficients of the nq points at q (host memory, or device
// memory when q_dev) on stream s: per chunk, k_prepare(_wide) with G1::one() as the G1 side
// (mode 0: a zero q is flagged, not an error; scale 0: the reference's coefficients, as
// bn_g2_precompute_many) into the workspace, then k_prepared_repack into the table.  The
// caller holds the lock and has ordered s after the workspace's previous user.
static int g2_prepare_fill(bn_ctx* c, bn_g2_prepared* h, const bn_g2* q, bool q_dev, hipStream_t s) {
    const size_t nq = h->nq;
    RET_IF(h->table.alloc(c, nq * (size_t)kPreparedWords));
    RET_IF(h->zero.alloc(c, nq));
    RET_IF(h->points.alloc(c, nq));
    const size_t mmax = nq < kChunk ? nq : kChunk;
    RET_IF(reserve(c, mmax));
    void* at[2];
    RET_IF(stage_regions(c, {mmax * sizeof(bn_g1), q_dev ? 0 : mmax * sizeof(bn_g2)}, at));
    for (auto [off, m] : chunks(nq)) {
        bn_g1* dp = (bn_g1*)at[0];
        const bn_g2* dq = q + off;
        if (!q_dev) {
            HIPCHK(c, hipMemcpyAsync(at[1], q + off, m * sizeof(bn_g2), hipMemcpyHostToDevice, s));
            dq = (const bn_g2*)at[1];
        }
        HIPCHK(c, hipMemcpyAsync(h->points + off, dq, m * sizeof(bn_g2), hipMemcpyDeviceToDevice, s));
        k_g1_fill_one<<<grid_for(m), kBlock, 0, s>>>(dp, m);
        RET_IF(prepare(c, dp, dq, m, 0, s, 0));
        k_prepared_repack<<<grid_for(kPathLanes * m), kBlock, 0, s>>>(c->coeffs, c->flags, m,
                                                                     h->table + off * (size_t)kPreparedWords,
                                                                     h->zero + off);
        HIPCHK(c, hipGetLastError());
    }
    return BN_OK;
}
static int g2_prepare(bn_ctx* c, const bn_g2* q, bool q_dev, size_t nq, bn_g2_prepared** out, hipStream_t s) {
    auto h = std::make_unique<bn_g2_prepared>();
    h->nq = nq;
    const int rc = g2_prepare_fill(c, h.get(), q, q_dev, s);
    return c->prepared.settle(c, std::move(h), rc, !q_dev, s, out);
}
// refused before anything is read: a NULL q or out, nq outside 1 .. 2^16
static int g2_prepare_args(bn_ctx* c, const void* q, size_t nq, bn_g2_prepared** out) {
    if (!q || !out) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    if (nq < 1 || nq > kPreparedMax) return fail(c, BN_ERR_INVALID_ARGUMENT, "nq outside 1 .. 2^16");
    return BN_OK;
}

int bn_g2_prepare(bn_ctx* c, const bn_g2* q, size_t nq, bn_g2_prepared** out) {
    if (out) *out = nullptr;
    CTX_GUARD(c);
    RET_IF(g2_prepare_args(c, q, nq, out));
    RET_IF(ws_acquire(c, c->stream));
    WsUse use{c, c->stream};
    return g2_prepare(c, q, false, nq, out, c->stream);
}

int bn_g2_prepare_dev(bn_ctx* c, const bn_g2* d_q, size_t nq, bn_g2_prepared** out, void* stream) {
    if (out) *out = nullptr;
    CTX_GUARD(c);
    RET_IF(g2_prepare_args(c, d_q, nq, out));
    const hipStream_t s = pick(c, stream);
    // (the workspace may grow in the fill: reserve() drains the previous users itself)
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return g2_prepare(c, d_q, true, nq, out, s);
}

size_t bn_g2_prepared_count(const bn_g2_prepared* h) { return h ? h->nq : 0; }

int bn_g2_prepared_destroy(bn_ctx* c, bn_g2_prepared* h) {
    CTX_GUARD(c);
    return c->prepared.destroy(c, h, "not a live prepared handle of this context");
}

// n pairings (fe) or Miller values of device arrays against the handle on stream s, every n
// through k_pairing_prepared in launch sets of kChunk; the caller holds the lock
static int prepared_dev_impl(bn_ctx* c, const bn_g1* d_p, const bn_g2_prepared* h, const uint32_t* d_qidx, size_t n,
                             bn_gt* d_out, bool fe, hipStream_t s) {
    if (fe) {
        // the kernel returns the step program's last result as the Gt, as k_pairing_full
        if (!c->fe_last_out) return fail(c, BN_ERR_INTERNAL, "step program does not end in its output");
        RET_IF(reserve(c, n < kChunk ? n : kChunk));
    }
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    for (auto [off, m] : chunks(n)) {
        launch_pairing_prepared(fe, d_p + off, h->table, h->zero, (uint32_t)h->nq, d_qidx ? d_qidx + off : nullptr, m,
                                c->d_prog, c->fe_steps, c->slots, d_out + off, c->d_err, s);
        HIPCHK(c, hipGetLastError());
    }
    return BN_OK;
}
static int prepared_args(bn_ctx* c, const void* p, const bn_g2_prepared* h, const void* out) {
    if (!p || !out || !h) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    if (!c->prepared.live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, "not a live prepared handle of this context");
    return BN_OK;
}
// the host forms: indices checked first, then per chunk stage, copy, launch, read back,
// synchronize (the device bits read per chunk, as bn_pairing_many's pageable form); the
// trailing synchronize because an early error may leave copies queued
static int prepared_host(bn_ctx* c, const bn_g1* p, const bn_g2_prepared* h, const uint32_t* qidx, size_t n,
                         bn_gt* out, bool fe) {
    CTX_GUARD_HOST(c);
    if (n == 0) return BN_OK;
    RET_IF(prepared_args(c, p, h, out));
    const int rc = [&]() -> int {
        if (qidx)
            for (size_t i = 0; i < n; ++i)
                if (qidx[i] >= h->nq) return fail(c, BN_ERR_INVALID_ARGUMENT, "prepared-point index out of range");
        for (auto [off, m] : chunks(n)) {
            void* at[3];
            RET_IF(stage_regions(c, {m * sizeof(bn_g1), m * sizeof(uint32_t), m * sizeof(bn_gt)}, at));
            uint32_t* didx = qidx ? (uint32_t*)at[1] : nullptr;
            RET_IF(clear_err(c, c->stream));
            HIPCHK(c, hipMemcpyAsync(at[0], p + off, m * sizeof(bn_g1), hipMemcpyHostToDevice, c->stream));
            if (qidx) HIPCHK(c, hipMemcpyAsync(didx, qidx + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            RET_IF(prepared_dev_impl(c, (bn_g1*)at[0], h, didx, m, (bn_gt*)at[2], fe, c->stream));
            HIPCHK(c, hipMemcpyAsync(out + off, at[2], m * sizeof(bn_gt), hipMemcpyDeviceToHost, c->stream));
            int bits = 0;
            RET_IF(check_err(c, c->stream, &bits));
            RET_IF(outcome(c, bits, kBitFeZero));
        }
        return BN_OK;
    }();
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int bn_pairing_prepared_many(bn_ctx* c, const bn_g1* p, const bn_g2_prepared* h, const uint32_t* qidx, size_t n,
                             bn_gt* out) {
    return prepared_host(c, p, h, qidx, n, out, true);
}

int bn_miller_loop_prepared_many(bn_ctx* c, const bn_g1* p, const bn_g2_prepared* h, const uint32_t* qidx, size_t n,
                                 bn_gt* out) {
    return prepared_host(c, p, h, qidx, n, out, false);
}

int bn_pairing_prepared_many_dev(bn_ctx* c, const bn_g1* d_p, const bn_g2_prepared* h, const uint32_t* d_qidx,
                                 size_t n, bn_gt* d_out, void* stream) {
    CTX_GUARD(c);
    if (n == 0) return BN_OK;
    RET_IF(prepared_args(c, d_p, h, d_out));
    return prepared_dev_impl(c, d_p, h, d_qidx, n, d_out, true, pick(c, stream));
}

// ---- products with prepared terms (bn_pairing_batch_prepared_many)
// Refusals, before any point buffer is read (qidx and offsets are the host's control arrays)
static int prepared_products_check(bn_ctx* c, const void* p, const void* q, const bn_g2_prepared* h,
                                   const uint32_t* qidx, const size_t* off, size_t m, const void* out) {
    RET_IF(offsets_check(c, off, m));
    if (!qidx || !out || !h) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    if (!c->prepared.live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, "not a live prepared handle of this context");
    if (off[m] && !p) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    size_t nf = 0;
    if (const char* why = products_terms_refusal(qidx, off, m, kProductLaneMax, h->nq, &nf))
        return fail(c, BN_ERR_INVALID_ARGUMENT, why);
    if (nf && !q) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    return BN_OK;
}
// The _dev form gathers a set's fresh G1 points into prod_fresh (grown on first use) in
// front of the producers; the prepared terms read the caller's points in place.
// A wide set reads every G1 point in place and gathers its G2 points into prod_gq instead.
int bn_pairing_batch_prepared_many_dev(bn_ctx* c, const bn_g1* d_p, const bn_g2* d_q, const bn_g2_prepared* h,
                                       const uint32_t* qidx, const size_t* offsets, size_t m, bn_gt* d_out,
                                       void* stream) {
    CTX_GUARD(c);
    if (m == 0) return BN_OK;
    RET_IF(prepared_products_check(c, d_p, d_q, h, qidx, offsets, m, d_out));
    const hipStream_t s = pick(c, stream);
    const ProductsPlan plan = products_plan_counted(c, offsets, m, qidx);
    RET_IF(products_reserve(c, offsets, plan));
    size_t nfmax = 0;
    for (const ProductsItem& st : plan.items)
        if (st.packed) nfmax = std::max(nfmax, st.nf);
    RET_IF(c->prod_fresh.grow(c, nfmax, 4096, true));
    RET_IF(wide_gather_reserve(c, plan));
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    RET_IF(products_upload(c, plan, offsets, qidx, false, s));
    for (const ProductsItem& st : plan.items) {
        const size_t lo = offsets[st.j0];
        if (st.wide) {  // p is read in term order, in place
            RET_IF(wide_prepared_set_dev(c, st, d_p + lo, d_q + st.f0, h, d_out + st.j0, s));
            continue;
        }
        if (st.nf) {
            launch_g1_gather(d_p + lo, c->prod_map.d + st.map_at + st.nf + 3 * st.np, st.nf, c->prod_fresh, s);
            HIPCHK(c, hipGetLastError());
        }
        RET_IF(prepared_set_dev(c, st, c->prod_fresh, d_q + st.f0, d_p + lo, h, d_out + st.j0, s));
    }
    return BN_OK;
}
// The host form stages a set's G1 points compacted, fresh first, then its fresh G2 points
// (a wide set's G1 points in term order: its G2 points are gathered to match).
int bn_pairing_batch_prepared_many(bn_ctx* c, const bn_g1* p, const bn_g2* q, const bn_g2_prepared* h,
                                   const uint32_t* qidx, const size_t* offsets, size_t m, bn_gt* out) {
    CTX_GUARD_HOST(c);
    if (m == 0) return BN_OK;
    RET_IF(prepared_products_check(c, p, q, h, qidx, offsets, m, out));
    const ProductsPlan plan = products_plan_counted(c, offsets, m, qidx);
    std::vector<bn_g1> hp;
    int rc = products_reserve(c, offsets, plan);
    if (!rc) rc = wide_gather_reserve(c, plan);
    if (!rc) rc = products_upload(c, plan, offsets, qidx, true, c->stream);
    if (!rc) rc = products_host_loop(c, plan, p, q, offsets, out, [&](const ProductsItem& st, bn_gt** d) -> int {
        const size_t lo = offsets[st.j0], nt = st.nf + st.np, mc = st.j1 - st.j0;
        void* at[3];
        RET_IF(stage_regions(c, {nt * sizeof(bn_g1), st.nf * sizeof(bn_g2), mc * sizeof(bn_gt)}, at));
        bn_g1* dp = (bn_g1*)at[0];
        *d = (bn_gt*)at[2];
        if (st.wide) {  // p in term order, the compacted fresh q, the same gather as the _dev form
            if (nt) HIPCHK(c, hipMemcpyAsync(dp, p + lo, nt * sizeof(bn_g1), hipMemcpyHostToDevice, c->stream));
            if (st.nf)
                HIPCHK(c, hipMemcpyAsync(at[1], q + st.f0, st.nf * sizeof(bn_g2), hipMemcpyHostToDevice, c->stream));
            return wide_prepared_set_dev(c, st, dp, (bn_g2*)at[1], h, *d, c->stream);
        }
        hp.resize(nt);  // (the previous set's copy has completed: check_err synchronizes)
        size_t kf = 0, kp = st.nf;
        for (size_t t = 0; t < nt; ++t) hp[qidx[lo + t] == BN_QIDX_FRESH ? kf++ : kp++] = p[lo + t];
        if (nt) HIPCHK(c, hipMemcpyAsync(dp, hp.data(), nt * sizeof(bn_g1), hipMemcpyHostToDevice, c->stream));
        if (st.nf)
            HIPCHK(c, hipMemcpyAsync(at[1], q + st.f0, st.nf * sizeof(bn_g2), hipMemcpyHostToDevice, c->stream));
        return prepared_set_dev(c, st, dp, (bn_g2*)at[1], dp, h, *d, c->stream);
    });
    (void)hipStreamSynchronize(c->stream);  // an early error may leave copies queued
    return rc;
}

}  // extern "C"
