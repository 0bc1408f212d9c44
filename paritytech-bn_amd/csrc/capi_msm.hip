// capi_msm.hip -- host side of the C ABI's multi-scalar multiplication (bn_g1_msm,
// bn_g2_msm; kernels_msm.hip, kernels_msm_g2.hip).  The bucket path
// and the small path return the same image: the group law is exact and the result is
// normalized.  The host sequence is one template over the point type; MsmGroup<P>
// names the group's kernels, settings and buffers.  Behind it, the bn_g1_prepared handles
// and bn_g1_msm_prepared_many (kernels_msm_fixed.hip; §8c), bn_g1_msm_many
// (kernels_msm_many.hip, msm_many_plan.h; §8d), and the bn_g1_basis and bn_g2_basis handles
// with bn_g1_msm_basis and bn_g2_msm_basis (kernels_msm_basis.hip, kernels_msm_basis_g2.hip;
// §8e, §8f), one template over the point type, and bn_g1_msm_basis_many
// (kernels_msm_basis_many.hip, msm_basis_many.h; §8g).
#include <type_traits>

#include "capi_internal.h"
#include "msm_basis.h"
#include "msm_basis_many.h"
#include "msm_fixed.h"
#include "msm_many.h"
#include "msm_many_plan.h"

using namespace bn;

constexpr size_t kMsmMaxTerms = size_t(1) << 26;  // the entry index keeps bit 31 for the sign; keys and positions are 32-bit
// Lanes (partial sums of 96 bytes) per launch set of bn_g1_msm_prepared_many: a call of more
// runs its outputs in sets of this many lanes through the same buffer.
constexpr size_t kFixedSetLanes = size_t(1) << 20;
template <class P>
struct MsmGroup;
template <>
struct MsmGroup<bn_g1> {
    static constexpr size_t kLanes = 1;  // lanes per element of the group-law kernels
    static constexpr auto k_count = k_msm_count;
    static constexpr auto k_scatter = k_msm_scatter;
    static constexpr auto k_accumulate = k_msm_accumulate;
    static constexpr auto k_chunk = k_msm_chunk;
    static constexpr auto k_fold = k_msm_fold;
    static constexpr auto k_reduce = k_msm_reduce;
    static constexpr auto k_horner = k_msm_horner;
    static constexpr auto k_finish = k_msm_finish;
    static constexpr auto k_op = k_g1_op;
    static MsmGroupWs<bn_g1>& ws(bn_ctx* c) { return c->msm_g1; }
    static void mul(const bn_g1* d_p, const bn_fr* d_k, size_t n, bn_g1* d_out, hipStream_t s) {
        g1_mul_launch(d_p, d_k, n, d_out, s);
    }
    // The window width used when bn_set_msm_window is 0: the fastest width of the measured
    // sweep (profiles/msm_sweep.jsonl, tools/msm_bench.py) at the nearest
    // measured size, the steps at the geometric means between sizes whose best width
    // differs.  Below 2^13 terms every width from 8 to 12 is within the run-to-run spread.
    static int auto_window(size_t n) {
        if (n < 6144) return 10;
        if (n < 92682) return 12;    // 2^16.5
        if (n < 370728) return 14;   // 2^18.5
        if (n < 741455) return 15;   // 2^19.5
        return 16;
    }
};
template <>
struct MsmGroup<bn_g2> {
    static constexpr size_t kLanes = kPathLanes;
    static constexpr auto k_count = k_msm_count_g2;
    static constexpr auto k_scatter = k_msm_scatter_g2;
    static constexpr auto k_accumulate = k_msm_accumulate_g2;
    static constexpr auto k_chunk = k_msm_chunk_g2;
    static constexpr auto k_fold = k_msm_fold_g2;
    static constexpr auto k_reduce = k_msm_reduce_g2;
    static constexpr auto k_horner = k_msm_horner_g2;
    static constexpr auto k_finish = k_msm_finish_g2;
    static constexpr auto k_op = k_g2_op;
    static MsmGroupWs<bn_g2>& ws(bn_ctx* c) { return c->msm_g2; }
    static void mul(const bn_g2* d_p, const bn_fr* d_k, size_t n, bn_g2* d_out, hipStream_t s) {
        g2_mul_launch(d_p, d_k, n, d_out, s);
    }
    // G2's own table, read off its own sweep in the same way (profiles/msm_g2_sweep.jsonl,
    // tools/msm_bench.py --group g2): 11 is the fastest width in the
    // thousands of terms, 12 at 2^15 and 14 already at 2^16.  Below 2^15 terms the widths
    // from 8 to 13 differ by less than the run-to-run spread (0.5 ms on a 2.3 ms floor).
    static int auto_window(size_t n) {
        if (n < 1449) return 10;     // 2^10.5
        if (n < 23171) return 11;    // 2^14.5
        if (n < 46341) return 12;    // 2^15.5
        if (n < 370728) return 14;   // 2^18.5
        if (n < 741455) return 15;   // 2^19.5
        return 16;
    }
};
struct MsmPlan {
    bool small;
    int c;
    uint32_t nwin, nkeys, nseg;
    size_t nent;  // n * W(c): the most entries
    // the overlong runs (msm.h): the run cap (kMsmRunUnsplit when no key of n terms can be
    // long), the fold levels launched, and the slots of the even and the odd levels' arrays
    uint32_t L;
    int levels;
    size_t slots_a, slots_b;
};
// the bucket path's plan of n terms at width cw under the run-cap setting run_max
static MsmPlan msm_plan_at(size_t run_max, size_t n, int cw) {
    MsmPlan m{};
    m.c = cw;
    m.nwin = (uint32_t)msm_windows(m.c);
    m.nkeys = msm_num_keys(m.c);
    m.nseg = (msm_buckets(m.c) + kMsmSegment - 1) / kMsmSegment;
    m.nent = n * m.nwin;
    m.L = run_max == BN_MSM_RUN_UNSPLIT ? kMsmRunUnsplit
          : run_max                     ? (uint32_t)run_max
                                        : msm_run_cap_default((uint32_t)n, m.c);
    m.levels = msm_fold_levels((uint32_t)n, m.L);
    if (m.levels == 0) m.L = kMsmRunUnsplit;
    if (m.levels && m.nent <= (size_t)0x7fffffff) {
        m.slots_a = msm_level_slots((uint32_t)m.nent, m.nkeys, m.L, 0);
        if (m.levels > 1) m.slots_b = msm_level_slots((uint32_t)m.nent, m.nkeys, m.L, 1);
    }
    return m;
}
template <class P>
static MsmPlan msm_plan(bn_ctx* c, size_t n) {
    const MsmGroupWs<P>& g = MsmGroup<P>::ws(c);
    MsmPlan m = msm_plan_at(g.run_max, n, g.window ? g.window : MsmGroup<P>::auto_window(n));
    m.small = n < g.min;
    return m;
}
template <class P>
static int msm_reserve(bn_ctx* c, size_t n, const MsmPlan& m) {
    MsmGroupWs<P>& g = MsmGroup<P>::ws(c);
    if (m.small) return g.tmp.grow(c, n);
    // counts | cursors | offsets (nkeys + 1) | the count of long keys | the long keys
    RET_IF(c->msm_keys.grow(c, 4 * (size_t)m.nkeys + 2));
    RET_IF(c->msm_sorted.grow(c, m.nent));
    RET_IF(g.buckets.grow(c, (size_t)m.nkeys));
    RET_IF(g.run_a.grow(c, m.slots_a));
    RET_IF(g.run_b.grow(c, m.slots_b));
    return g.parts.grow(c, (size_t)m.nseg * m.nwin);
}
// buf[0 .. width) = sum of the m rows of `width` points at buf by a halving addition tree in
// place (odd tail carried)
template <class P>
static void msm_tree(P* buf, size_t m, size_t width, hipStream_t s) {
    while (m > 1) {
        const size_t h = (m + 1) / 2;
        MsmGroup<P>::k_op<<<grid_for((m - h) * width), kBlock, 0, s>>>(kGroupAdd, buf, buf + h * width, (m - h) * width, buf, nullptr);
        m = h;
    }
}
// the tree, then for width 1 *d_out = the sum's returned image (finish) or the Jacobian sum
// as it stands
template <class P>
static int msm_tree_out(bn_ctx* c, P* buf, size_t m, size_t width, int finish, P* d_out, hipStream_t s) {
    using G = MsmGroup<P>;
    msm_tree(buf, m, width, s);
    m = m ? 1 : 0;
    if (width != 1) return BN_OK;
    if (finish)
        G::k_finish<<<1, 64, 0, s>>>(m ? buf : nullptr, d_out);
    else if (m)
        HIPCHK(c, hipMemcpyAsync(d_out, buf, sizeof(P), hipMemcpyDeviceToDevice, s));
    else
        G::k_finish<<<1, 64, 0, s>>>(nullptr, d_out);  // zero is its own Jacobian image
    return BN_OK;
}
// The fold levels above the s0 chunk sums in run_a: one launch per level the largest run can
// have; every grid is the host's bound for its level.  Even levels write run_a, odd ones run_b.
template <class P>
static void msm_folds(bn_ctx* c, const MsmPlan& m, const uint32_t* offsets, const uint32_t* longinfo, uint32_t s0,
                      hipStream_t s) {
    using G = MsmGroup<P>;
    MsmGroupWs<P>& g = G::ws(c);
    const uint32_t nent = (uint32_t)m.nent;
    uint32_t nsrc = s0;
    for (int lv = 1; lv <= m.levels; ++lv) {
        P* src = lv & 1 ? g.run_a : g.run_b;
        P* dst = lv & 1 ? g.run_b : g.run_a;
        const size_t cap = lv == m.levels ? 0 : (lv & 1 ? g.run_b.cap() : g.run_a.cap());  // the last level writes buckets only
        const uint32_t slots = msm_level_slots(nent, m.nkeys, m.L, lv);
        const uint32_t ndst = (uint32_t)std::min<size_t>(slots, cap);
        G::k_fold<<<grid_for(G::kLanes * (size_t)slots), kBlock, 0, s>>>(src, nsrc, offsets, longinfo, m.nkeys, nent, m.L, lv, dst, ndst, slots, g.buckets);
        nsrc = ndst;
    }
}
// The bucket path's front half on s, shared by its two forms: msm_keys carved into counts |
// cursors | offsets | longinfo, then the entries of n terms counted, scanned and scattered
// into msm_sorted by key.  count and scatter are the form's kernels, src their first argument
// (the points, or a basis handle's zero flags).
struct MsmKeys {
    uint32_t *offsets, *longinfo;
    uint32_t nent;
};
template <class Count, class Scatter, class Src>
static int msm_sort(bn_ctx* c, const MsmPlan& m, Count count, Scatter scatter, Src src, const bn_fr* d_k, size_t n,
                    hipStream_t s, MsmKeys* k) {
    uint32_t* counts = c->msm_keys;
    uint32_t* cursors = counts + m.nkeys;
    k->offsets = cursors + m.nkeys;
    k->longinfo = k->offsets + m.nkeys + 1;
    k->nent = (uint32_t)m.nent;
    HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)m.nkeys * 4, s));
    count<<<grid_for(n), kBlock, 0, s>>>(src, d_k, n, m.c, m.nkeys, counts);
    k_msm_scan<<<1, kMsmScanBlock, 0, s>>>(counts, m.nkeys, k->offsets, cursors, m.L, k->longinfo);
    scatter<<<grid_for(n), kBlock, 0, s>>>(src, d_k, n, m.c, m.nkeys, cursors, k->offsets, c->msm_sorted, k->nent);
    return BN_OK;
}
// The runs above the cap, behind the form's accumulate: their chunks (chunk(grid, ...) launches
// the form's kernel behind its own leading arguments), then one fold launch per level the
// largest run n terms can have needs; every grid is the host's bound for its level, and a
// lane whose slot no long key holds returns.  Even levels write run_a, odd ones run_b.
template <class P, class Chunk>
static void msm_long_runs(bn_ctx* c, const MsmPlan& m, const MsmKeys& k, hipStream_t s, Chunk&& chunk) {
    if (!m.levels) return;
    MsmGroupWs<P>& g = MsmGroup<P>::ws(c);
    const uint32_t s0 = (uint32_t)std::min(m.slots_a, g.run_a.cap());
    chunk(grid_for(MsmGroup<P>::kLanes * (size_t)s0), c->msm_sorted.get(), k.offsets, k.longinfo, m.nkeys, k.nent, m.L,
          g.run_a.get(), s0);
    msm_folds<P>(c, m, k.offsets, k.longinfo, s0, s);
}
// the device sequence on stream s; the caller holds the lock and the workspace order.
// The group-law kernels take G::kLanes lanes per element (kBlock is even: whole pairs).
template <class P>
static int msm_dev_impl(bn_ctx* c, const P* d_p, const bn_fr* d_k, size_t n, P* d_out, hipStream_t s, int finish) {
    using G = MsmGroup<P>;
    if (n == 0) {
        G::k_finish<<<1, 64, 0, s>>>(nullptr, d_out);
        HIPCHK(c, hipGetLastError());
        return BN_OK;
    }
    const MsmPlan m = msm_plan<P>(c, n);
    if (!m.small && m.nent > (size_t)0x7fffffff)
        return fail(c, BN_ERR_INVALID_ARGUMENT, "n * windows exceeds the 32-bit entry positions at this window width");
    RET_IF(msm_reserve<P>(c, n, m));
    MsmGroupWs<P>& g = G::ws(c);
    if (m.small) {
        G::mul(d_p, d_k, n, g.tmp, s);
        RET_IF(msm_tree_out(c, g.tmp.get(), n, 1, finish, d_out, s));
        HIPCHK(c, hipGetLastError());
        return BN_OK;
    }
    const size_t nparts = (size_t)m.nseg * m.nwin;
    MsmKeys k;
    RET_IF(msm_sort(c, m, G::k_count, G::k_scatter, d_p, d_k, n, s, &k));
    G::k_accumulate<<<grid_for(G::kLanes * m.nkeys), kBlock, 0, s>>>(d_p, n, c->msm_sorted, k.offsets, m.nkeys, k.nent, m.L, g.buckets);
    msm_long_runs<P>(c, m, k, s, [&](auto grid, auto... a) { G::k_chunk<<<grid, kBlock, 0, s>>>(d_p, n, a...); });
    G::k_reduce<<<grid_for(G::kLanes * nparts), kBlock, 0, s>>>(g.buckets, m.c, m.nkeys, m.nseg, g.parts);
    RET_IF(msm_tree_out<P>(c, g.parts, m.nseg, m.nwin, 0, nullptr, s));
    G::k_horner<<<1, 64, 0, s>>>(g.parts, m.c, finish, d_out);
    HIPCHK(c, hipGetLastError());
    return BN_OK;
}
static int msm_check_args(bn_ctx* c, const void* p, const void* k, size_t n, const void* out) {
    if (n > kMsmMaxTerms) return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 terms");
    if (!out || (n && (!p || !k))) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    return BN_OK;
}
template <class P>
static int msm_host(bn_ctx* c, const P* p, const bn_fr* k, size_t n, P* out, int finish) {
    CTX_GUARD_HOST(c);
    RET_IF(msm_check_args(c, p, k, n, out));
    void* at[3];  // the sum, the points, the scalars
    RET_IF(stage_regions(c, {sizeof(P), n * sizeof(P), n * sizeof(bn_fr)}, at));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(at[1], p, n * sizeof(P), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(at[2], k, n * sizeof(bn_fr), hipMemcpyHostToDevice, c->stream));
    }
    RET_IF(msm_dev_impl(c, (const P*)at[1], (const bn_fr*)at[2], n, (P*)at[0], c->stream, finish));
    HIPCHK(c, hipMemcpyAsync(out, at[0], sizeof(P), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BN_OK;
}
// *out = the returned image of the sum of the m host points a[0 .. m) (the partials of
// a multi-device context, in device order)
template <class P>
static int msm_sum_host(bn_ctx* c, const P* a, size_t m, P* out) {
    CTX_GUARD_HOST(c);
    if (!out || (m && !a)) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    MsmGroupWs<P>& g = MsmGroup<P>::ws(c);
    RET_IF(g.tmp.grow(c, m + 1));
    P* dout = g.tmp + m;
    if (m) HIPCHK(c, hipMemcpyAsync(g.tmp, a, m * sizeof(P), hipMemcpyHostToDevice, c->stream));
    RET_IF(msm_tree_out(c, g.tmp.get(), m, 1, 1, dout, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, dout, sizeof(P), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BN_OK;
}
template <class P>
static int msm_dev(bn_ctx* c, const P* d_p, const bn_fr* d_k, size_t n, P* d_out, void* stream) {
    CTX_GUARD(c);
    RET_IF(msm_check_args(c, d_p, d_k, n, d_out));
    hipStream_t s = pick(c, stream);
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return msm_dev_impl(c, d_p, d_k, n, d_out, s, 1);
}
// bn_msm_reserve / bn_g2_msm_reserve on a single-device context
template <class P>
static int msm_reserve_terms(bn_ctx* c, size_t n) {
    CTX_GUARD(c);
    if (n > kMsmMaxTerms) return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 terms");
    if (n == 0) return BN_OK;
    const MsmPlan m = msm_plan<P>(c, n);
    if (!m.small && m.nent > (size_t)0x7fffffff)
        return fail(c, BN_ERR_INVALID_ARGUMENT, "n * windows exceeds the 32-bit entry positions at this window width");
    RET_IF(msm_reserve<P>(c, n, m));
    // and the partial sums of the prepared-bases MSM for calls of up to n lanes (G1 only)
    if constexpr (std::is_same<P, bn_g1>::value)
        return c->msm_g1.fixed.grow(c, std::min(n, kFixedSetLanes));
    return BN_OK;
}

// ---------------------------------------------------------------- prepared bases
// refused before anything is read: a NULL bases or out, a width outside 2 .. 16 (0: the
// default), a k that is 0 or whose table exceeds the 32-bit entry indices
static int g1_prepare_args(bn_ctx* c, const void* bases, size_t k, int cw, bn_g1_prepared** out) {
    if (!bases || !out) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    if (cw != 0 && !msm_window_ok(cw)) return fail(c, BN_ERR_INVALID_ARGUMENT, "window width outside 2 .. 16 (0: default)");
    if (!msm_fixed_entries(k, cw))
        return fail(c, BN_ERR_INVALID_ARGUMENT, "k is 0 or k * windows * 2^(c-1) exceeds the 32-bit entry indices");
    return BN_OK;
}
// Fills a new handle on stream s from the k bases (host memory, or device memory when dev).
// The caller holds the lock and has ordered s after the workspace's previous user (the host
// form stages the bases).
static int g1_prepare_fill(bn_ctx* c, bn_g1_prepared* h, const bn_g1* bases, bool dev, hipStream_t s) {
    RET_IF(h->table.alloc(c, (size_t)h->nent * 2));
    RET_IF(h->zero.alloc(c, h->k));
    const bn_g1* d = bases;
    if (!dev) {
        void* at[1];
        RET_IF(stage_regions(c, {h->k * sizeof(bn_g1)}, at));
        HIPCHK(c, hipMemcpyAsync(at[0], bases, h->k * sizeof(bn_g1), hipMemcpyHostToDevice, s));
        d = (const bn_g1*)at[0];
    }
    k_g1_table_build<<<grid_for(h->k * (size_t)msm_windows(h->c)), kBlock, 0, s>>>(d, (uint32_t)h->k, h->c, h->table,
                                                                                   h->zero, h->nent);
    HIPCHK(c, hipGetLastError());
    return BN_OK;
}
static int g1_prepare(bn_ctx* c, const bn_g1* bases, bool dev, size_t k, int cw, bn_g1_prepared** out, hipStream_t s) {
    auto h = std::make_unique<bn_g1_prepared>();
    h->k = k;
    h->c = cw ? cw : kMsmFixedWindow;
    h->nent = (uint32_t)msm_fixed_entries(k, h->c);
    const int rc = g1_prepare_fill(c, h.get(), bases, dev, s);
    return c->g1_prepared.settle(c, std::move(h), rc, !dev, s, out);
}
static int msm_prepared_args(bn_ctx* c, const bn_g1_prepared* h, const void* k, size_t m, const void* out,
                             size_t out_stride) {
    if (!c->g1_prepared.live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, "not a live prepared handle of this context");
    if (out_stride == 0) return fail(c, BN_ERR_INVALID_ARGUMENT, "out_stride is 0");
    if (m > kMsmMaxTerms) return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 outputs");
    if (m && (!k || !out)) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    return BN_OK;
}
// the device sequence on stream s, in sets of kFixedSetLanes lanes: the lookups, the tree
// over each output's lanes, the finish; the caller holds the lock and the workspace order
static int msm_prepared_dev_impl(bn_ctx* c, const bn_g1_prepared* h, const bn_fr* d_k, size_t m, bn_g1* d_out,
                                 size_t out_stride, hipStream_t s) {
    MsmGroupWs<bn_g1>& g = c->msm_g1;
    const uint32_t L = g.fixed_lanes ? (uint32_t)g.fixed_lanes : msm_fixed_auto_lanes(m, h->k, h->c);
    const size_t set = std::max<size_t>(1, kFixedSetLanes / L);
    RET_IF(g.fixed.grow(c, std::min(m, set) * L));
    for (size_t off = 0; off < m; off += set) {
        const size_t mc = std::min(m - off, set);
        k_g1_msm_fixed<<<grid_for(mc * L), kBlock, 0, s>>>(h->table, h->zero, h->nent, (uint32_t)h->k, h->c,
                                                           d_k + off * h->k, mc, L, g.fixed);
        msm_tree(g.fixed.get(), L, mc, s);
        k_g1_msm_fixed_finish<<<grid_for(mc), kBlock, 0, s>>>(g.fixed, mc, d_out + off * out_stride, out_stride);
    }
    HIPCHK(c, hipGetLastError());
    return BN_OK;
}

// ---------------------------------------------------------------- one large MSM over a fixed basis
// One host sequence over the point type; MsmBasis<P> names the group's handle type and list,
// its table element, its kernels and its default width (the grids take MsmGroup<P>::kLanes
// lanes per element; the workspace is MsmGroup<P>::ws).
template <class P>
struct MsmBasis;
template <>
struct MsmBasis<bn_g1> {
    using Handle = bn_g1_basis;
    using Elem = bn_fq;  // an entry is two of them: x, y
    static constexpr auto k_build = k_g1_basis_build;
    static constexpr auto k_accumulate = k_msm_basis_accumulate;
    static constexpr auto k_chunk = k_msm_basis_chunk;
    static constexpr auto k_reduce = k_msm_basis_reduce;
    // the batched form's kernels (bn_g1_msm_basis_many; G1 only so far)
    static constexpr auto k_many_count = k_msm_basis_many_count;
    static constexpr auto k_many_scan = k_msm_basis_many_scan;
    static constexpr auto k_many_scatter = k_msm_basis_many_scatter;
    static constexpr auto k_many_accumulate = k_msm_basis_many_accumulate;
    static constexpr auto k_many_chunk = k_msm_basis_many_chunk;
    static constexpr auto k_many_fold = k_msm_basis_many_fold;
    static constexpr auto k_many_reduce = k_msm_basis_many_reduce;
    static constexpr auto k_many_finish = k_g1_msm_fixed_finish;
    static constexpr auto k_many_zero = k_msm_basis_many_zero;
    static HandleList<Handle>& list(bn_ctx* c) { return c->g1_basis; }
    static int auto_window(size_t nbases) { return msm_basis_auto_window(nbases); }
};
template <>
struct MsmBasis<bn_g2> {
    using Handle = bn_g2_basis;
    using Elem = bn_fq2;  // an entry is two of them: the lane halves (x.c0, y.c0), (x.c1, y.c1)
    static constexpr auto k_build = k_g2_basis_build;
    static constexpr auto k_accumulate = k_msm_basis_accumulate_g2;
    static constexpr auto k_chunk = k_msm_basis_chunk_g2;
    static constexpr auto k_reduce = k_msm_basis_reduce_g2;
    static HandleList<Handle>& list(bn_ctx* c) { return c->g2_basis; }
    static int auto_window(size_t nbases) { return msm_basis_auto_window_g2(nbases); }
};
// entries of the table of nbases bases at width cw (0: the group's default); 0 for arguments
// that the prepare call refuses
template <class P>
static uint64_t basis_entries(size_t nbases, int cw) {
    return msm_basis_entries_at(nbases, cw ? cw : MsmBasis<P>::auto_window(nbases));
}
template <class P>
static size_t basis_table_bytes(size_t nbases, int cw) {
    const uint64_t nent = basis_entries<P>(nbases, cw);
    return nent ? (size_t)(nent * 2 * sizeof(typename MsmBasis<P>::Elem) + nbases) : 0;
}
// refused before anything is read: a NULL bases or out, a width outside 2 .. 16 (0: the
// default), an nbases that is 0, above 2^26 or whose nbases * W(c) exceeds the 32-bit positions
template <class P>
static int basis_args(bn_ctx* c, const void* bases, size_t nbases, int cw, typename MsmBasis<P>::Handle** out) {
    if (!bases || !out) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    if (cw != 0 && !msm_window_ok(cw)) return fail(c, BN_ERR_INVALID_ARGUMENT, "window width outside 2 .. 16 (0: default)");
    if (!basis_entries<P>(nbases, cw))
        return fail(c, BN_ERR_INVALID_ARGUMENT, "nbases is 0, above 2^26, or nbases * windows exceeds 2^31 - 1");
    return BN_OK;
}
// Fills a new handle on stream s from the bases (host memory, or device memory when dev).
// The caller holds the lock and has ordered s after the workspace's previous user (the host
// form stages the bases).
template <class P>
static int basis_fill(bn_ctx* c, typename MsmBasis<P>::Handle* h, const P* bases, bool dev, hipStream_t s) {
    using B = MsmBasis<P>;
    const size_t nbases = h->nbases;
    RET_IF(h->table.alloc(c, (size_t)msm_basis_entries_at(nbases, h->c) * 2));
    RET_IF(h->zero.alloc(c, nbases));
    const P* d = bases;
    if (!dev) {
        void* at[1];
        RET_IF(stage_regions(c, {nbases * sizeof(P)}, at));
        HIPCHK(c, hipMemcpyAsync(at[0], bases, nbases * sizeof(P), hipMemcpyHostToDevice, s));
        d = (const P*)at[0];
    }
    B::k_build<<<grid_for(MsmGroup<P>::kLanes * nbases), kBlock, 0, s>>>(d, (uint32_t)nbases, h->c, h->table, h->zero);
    HIPCHK(c, hipGetLastError());
    return BN_OK;
}
template <class P>
static int basis_make(bn_ctx* c, const P* bases, bool dev, size_t nbases, int cw, typename MsmBasis<P>::Handle** out,
                      hipStream_t s) {
    using B = MsmBasis<P>;
    auto h = std::make_unique<typename B::Handle>();
    h->nbases = nbases;
    h->c = cw ? cw : B::auto_window(nbases);
    const int rc = basis_fill<P>(c, h.get(), bases, dev, s);
    return B::list(c).settle(c, std::move(h), rc, !dev, s, out);
}
// bn_g1_basis_prepare / bn_g2_basis_prepare (stream: the context's) and their _dev forms
template <class P>
static int basis_prepare(bn_ctx* c, const P* bases, bool dev, size_t nbases, int cw, typename MsmBasis<P>::Handle** out,
                         void* stream) {
    CTX_GUARD(c);
    RET_IF(basis_args<P>(c, bases, nbases, cw, out));
    const hipStream_t s = dev ? pick(c, stream) : c->stream;
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return basis_make<P>(c, bases, dev, nbases, cw, out, s);
}
template <class P>
static int basis_destroy(bn_ctx* c, typename MsmBasis<P>::Handle* h) {
    CTX_GUARD(c);
    return MsmBasis<P>::list(c).destroy(c, h, "not a live basis handle of this context");
}
template <class P>
static int msm_basis_args(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const void* k, size_t n, const void* out) {
    if (!MsmBasis<P>::list(c).live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, "not a live basis handle of this context");
    if (!out) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    if (n > h->nbases) return fail(c, BN_ERR_INVALID_ARGUMENT, "more terms than the handle has bases");
    if (n && !k) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    return BN_OK;
}
// the plan of n terms over the handle: the bucket path's at the handle's width and the run
// cap in force (bn_set_msm_window and bn_set_msm_min do not apply)
template <class P>
static MsmPlan msm_basis_plan(bn_ctx* c, const typename MsmBasis<P>::Handle* h, size_t n) {
    return msm_plan_at(MsmGroup<P>::ws(c).run_max, n, h->c);
}
// The device sequence on stream s over the first n bases; the caller holds the lock and the
// workspace order.  n * W(c) <= nbases * W(c) <= 2^31 - 1 (the prepare call's check).
template <class P>
static int msm_basis_dev_impl(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const bn_fr* d_k, size_t n, P* d_out,
                              hipStream_t s) {
    using G = MsmGroup<P>;
    using B = MsmBasis<P>;
    if (n == 0) {
        G::k_finish<<<1, 64, 0, s>>>(nullptr, d_out);
        HIPCHK(c, hipGetLastError());
        return BN_OK;
    }
    const MsmPlan m = msm_basis_plan<P>(c, h, n);
    RET_IF(msm_reserve<P>(c, n, m));
    MsmGroupWs<P>& g = G::ws(c);
    const uint32_t nb = msm_buckets(m.c), nbases = (uint32_t)h->nbases;
    MsmKeys k;
    RET_IF(msm_sort(c, m, k_msm_count_basis, k_msm_scatter_basis, h->zero.get(), d_k, n, s, &k));
    B::k_accumulate<<<grid_for(G::kLanes * m.nkeys), kBlock, 0, s>>>(h->table, nbases, (uint32_t)n, m.c, c->msm_sorted,
                                                                     k.offsets, m.nkeys, k.nent, m.L, g.buckets);
    msm_long_runs<P>(c, m, k, s, [&](auto grid, auto... a) {
        B::k_chunk<<<grid, kBlock, 0, s>>>(h->table.get(), nbases, (uint32_t)n, m.c, a...);
    });
    // Every window's bucket j weighs j + 1 but the top one's, whose slots are replicas: the rows
    // of the windows below it are added into window 0's row, and two windows are reduced.
    msm_tree(g.buckets.get(), m.nwin - 1, nb, s);
    B::k_reduce<<<grid_for(G::kLanes * 2 * (size_t)m.nseg), kBlock, 0, s>>>(g.buckets, m.c, m.nkeys, m.nseg, g.parts);
    msm_tree(g.parts.get(), m.nseg, 2, s);
    msm_tree(g.parts.get(), 2, 1, s);  // the two window sums: no weight between them, nothing is doubled
    G::k_finish<<<1, 64, 0, s>>>(g.parts, d_out);
    HIPCHK(c, hipGetLastError());
    return BN_OK;
}
template <class P>
static int msm_basis_host(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const bn_fr* k, size_t n, P* out) {
    CTX_GUARD_HOST(c);
    RET_IF(msm_basis_args<P>(c, h, k, n, out));
    void* at[2];  // the sum, the scalars
    RET_IF(stage_regions(c, {sizeof(P), n * sizeof(bn_fr)}, at));
    if (n) HIPCHK(c, hipMemcpyAsync(at[1], k, n * sizeof(bn_fr), hipMemcpyHostToDevice, c->stream));
    RET_IF(msm_basis_dev_impl<P>(c, h, (const bn_fr*)at[1], n, (P*)at[0], c->stream));
    HIPCHK(c, hipMemcpyAsync(out, at[0], sizeof(P), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BN_OK;
}
template <class P>
static int msm_basis_dev(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const bn_fr* d_k, size_t n, P* d_out,
                         void* stream) {
    CTX_GUARD(c);
    RET_IF(msm_basis_args<P>(c, h, d_k, n, d_out));
    hipStream_t s = pick(c, stream);
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return msm_basis_dev_impl<P>(c, h, d_k, n, d_out, s);
}
template <class P>
static int msm_basis_reserve(bn_ctx* c, const typename MsmBasis<P>::Handle* h, size_t n) {
    CTX_GUARD(c);
    if (!MsmBasis<P>::list(c).live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, "not a live basis handle of this context");
    if (n > h->nbases) return fail(c, BN_ERR_INVALID_ARGUMENT, "more terms than the handle has bases");
    if (n == 0) return BN_OK;
    return msm_reserve<P>(c, n, msm_basis_plan<P>(c, h, n));
}

// ---------------------------------------------------------------- a batch of vectors over a fixed basis
// The m vectors run in launch sets of S (msm_basis_many.h msm_basis_many_set; bn_set_msm_basis_many_set
// forces S), one after another on the same stream through the shared workspace; a set costs the
// launches of one single call.  One host sequence over the point type: MsmBasis<P> names the
// kernels (G1 only so far).
template <class P>
static int msm_basis_many_args(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const void* k, size_t k_stride, size_t m,
                               size_t n, const void* out, size_t out_stride) {
    if (!MsmBasis<P>::list(c).live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, "not a live basis handle of this context");
    if (n > h->nbases) return fail(c, BN_ERR_INVALID_ARGUMENT, "more terms than the handle has bases");
    if (k_stride < n) return fail(c, BN_ERR_INVALID_ARGUMENT, "k_stride is below n");
    if (out_stride == 0) return fail(c, BN_ERR_INVALID_ARGUMENT, "out_stride is 0");
    if (m > kMsmBasisManyMaxVectors) return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 vectors");
    if (!out || (m && n && !k)) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    return BN_OK;
}
// one vector's plan and the vectors of a launch set of a call of m vectors of n terms
struct MsmBasisManyPlan {
    MsmPlan one;
    size_t S;
};
template <class P>
static MsmBasisManyPlan msm_basis_many_plan(bn_ctx* c, const typename MsmBasis<P>::Handle* h, size_t m, size_t n) {
    MsmBasisManyPlan p{msm_basis_plan<P>(c, h, n), 1};
    p.S = (size_t)msm_basis_many_set(m, n, p.one.c, 0, MsmGroup<P>::ws(c).basis_many_set);
    return p;
}
template <class P>
static int msm_basis_many_grow(bn_ctx* c, const MsmBasisManyPlan& p) {
    MsmGroupWs<P>& g = MsmGroup<P>::ws(c);
    const MsmPlan& m = p.one;
    RET_IF(c->msm_keys.grow(c, p.S * (size_t)msm_basis_many_words(m.nkeys)));
    RET_IF(c->msm_sorted.grow(c, p.S * m.nent));
    RET_IF(g.buckets.grow(c, p.S * m.nkeys));
    RET_IF(g.run_a.grow(c, p.S * m.slots_a));
    RET_IF(g.run_b.grow(c, p.S * m.slots_b));
    return g.parts.grow(c, (size_t)m.nseg * 2 * p.S);
}
// The device sequence on stream s; the caller holds the lock and the workspace order.  m > 0.
template <class P>
static int msm_basis_many_dev_impl(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const bn_fr* d_k, size_t k_stride,
                                   size_t m, size_t n, P* d_out, size_t out_stride, hipStream_t s) {
    using G = MsmGroup<P>;
    using B = MsmBasis<P>;
    if (n == 0) {
        B::k_many_zero<<<grid_for(m), kBlock, 0, s>>>(m, d_out, out_stride);
        HIPCHK(c, hipGetLastError());
        return BN_OK;
    }
    const MsmBasisManyPlan plan = msm_basis_many_plan<P>(c, h, m, n);
    RET_IF(msm_basis_many_grow<P>(c, plan));
    const MsmPlan& pl = plan.one;
    MsmGroupWs<P>& g = G::ws(c);
    const uint32_t nb = msm_buckets(pl.c), nbases = (uint32_t)h->nbases, nent = (uint32_t)pl.nent;
    const uint32_t sa = (uint32_t)pl.slots_a, sb = (uint32_t)pl.slots_b;
    const size_t words = (size_t)msm_basis_many_words(pl.nkeys);
    uint32_t* keys = c->msm_keys;
    for (size_t off = 0; off < m; off += plan.S) {
        const size_t sc = std::min(m - off, plan.S);
        const MsmBasisManyShape shape{(uint32_t)sc, (uint32_t)n, pl.nkeys, nent, pl.c};
        const bn_fr* k = d_k + off * k_stride;
        // every vector's counts (the head of its block)
        HIPCHK(c, hipMemset2DAsync(keys, words * 4, 0, (size_t)pl.nkeys * 4, sc, s));
        B::k_many_count<<<grid_for(sc * n), kBlock, 0, s>>>(h->zero, nbases, k, k_stride, shape, keys);
        B::k_many_scan<<<(unsigned)sc, kMsmScanBlock, 0, s>>>(keys, pl.nkeys, (uint32_t)sc, pl.L);
        B::k_many_scatter<<<grid_for(sc * n), kBlock, 0, s>>>(h->zero, nbases, k, k_stride, shape, keys, c->msm_sorted);
        B::k_many_accumulate<<<grid_for(G::kLanes * sc * pl.nkeys), kBlock, 0, s>>>(h->table, nbases, shape, keys,
                                                                                   c->msm_sorted, pl.L, g.buckets);
        if (pl.levels) {
            B::k_many_chunk<<<grid_for(G::kLanes * sc * sa), kBlock, 0, s>>>(h->table, nbases, shape, keys, c->msm_sorted,
                                                                             pl.L, g.run_a, sa);
            // even levels write run_a, odd ones run_b; the last level writes buckets only
            for (int lv = 1; lv <= pl.levels; ++lv) {
                const bool odd = lv & 1;
                const uint32_t slots = msm_level_slots(nent, pl.nkeys, pl.L, lv);
                B::k_many_fold<<<grid_for(G::kLanes * sc * slots), kBlock, 0, s>>>(
                    shape, keys, pl.L, lv, odd ? g.run_a.get() : g.run_b.get(), odd ? sa : sb,
                    odd ? g.run_b.get() : g.run_a.get(), lv == pl.levels ? 0u : (odd ? sb : sa), slots, g.buckets);
            }
        }
        // as the single call: the rows of the windows below the top one added into window 0's
        // (a row is every vector's slots), two windows reduced, the trees, the returned images
        msm_tree(g.buckets.get(), pl.nwin - 1, sc * nb, s);
        B::k_many_reduce<<<grid_for(G::kLanes * 2 * (size_t)pl.nseg * sc), kBlock, 0, s>>>(g.buckets, pl.c, pl.nkeys, pl.nseg,
                                                                                          (uint32_t)sc, g.parts);
        msm_tree(g.parts.get(), pl.nseg, 2 * sc, s);
        msm_tree(g.parts.get(), 2, sc, s);
        B::k_many_finish<<<grid_for(sc), kBlock, 0, s>>>(g.parts, sc, d_out + off * out_stride, out_stride);
        HIPCHK(c, hipGetLastError());
    }
    return BN_OK;
}
template <class P>
static int msm_basis_many_host(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const bn_fr* k, size_t k_stride, size_t m,
                               size_t n, P* out, size_t out_stride) {
    CTX_GUARD_HOST(c);
    RET_IF(msm_basis_many_args<P>(c, h, k, k_stride, m, n, out, out_stride));
    if (m == 0) return BN_OK;
    void* at[2];  // the sums, the rows' first n scalars (the padding of a wider row is not read)
    RET_IF(stage_regions(c, {m * sizeof(P), m * n * sizeof(bn_fr)}, at));
    if (n)
        HIPCHK(c, hipMemcpy2DAsync(at[1], n * sizeof(bn_fr), k, k_stride * sizeof(bn_fr), n * sizeof(bn_fr), m,
                                   hipMemcpyHostToDevice, c->stream));
    RET_IF(msm_basis_many_dev_impl<P>(c, h, (const bn_fr*)at[1], n, m, n, (P*)at[0], 1, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(out, out_stride * sizeof(P), at[0], sizeof(P), sizeof(P), m, hipMemcpyDeviceToHost,
                               c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BN_OK;
}
template <class P>
static int msm_basis_many_dev(bn_ctx* c, const typename MsmBasis<P>::Handle* h, const bn_fr* d_k, size_t k_stride, size_t m,
                              size_t n, P* d_out, size_t out_stride, void* stream) {
    CTX_GUARD(c);
    RET_IF(msm_basis_many_args<P>(c, h, d_k, k_stride, m, n, d_out, out_stride));
    if (m == 0) return BN_OK;
    hipStream_t s = pick(c, stream);
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return msm_basis_many_dev_impl<P>(c, h, d_k, k_stride, m, n, d_out, out_stride, s);
}
template <class P>
static int msm_basis_many_reserve(bn_ctx* c, const typename MsmBasis<P>::Handle* h, size_t m, size_t n) {
    CTX_GUARD(c);
    if (!MsmBasis<P>::list(c).live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, "not a live basis handle of this context");
    if (n > h->nbases) return fail(c, BN_ERR_INVALID_ARGUMENT, "more terms than the handle has bases");
    if (m > kMsmBasisManyMaxVectors) return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 vectors");
    if (m == 0 || n == 0) return BN_OK;
    return msm_basis_many_grow<P>(c, msm_basis_many_plan<P>(c, h, m, n));
}

// ---------------------------------------------------------------- many MSMs over fresh bases
// The settings a 0 stands for, read off profiles/msm_many_sweep.jsonl: width
// 4; the automatic T of a launch set is the smallest that keeps the set at 2^16 lanes (one
// wave on every SIMD: below that the card idles, above it a shorter chain gains less than the
// shared doublings), at most 16; a set takes at most 2^20 terms, and at most 1 GiB of digits
// and multiples, so windows above 4 shrink it (a forced chunk is taken as it is); segments
// above 1,024 terms run alone on bn_g1_msm's path (1.9 ms each) unless the call has 16 or more
// of them, which together fill the card on the packed path (a forced max always holds).
constexpr int kManyWindow = 4;
constexpr size_t kManyLanes = size_t(1) << 16;
constexpr uint32_t kManyUnitAutoMax = 16;
constexpr size_t kManySetTerms = size_t(1) << 20;
constexpr size_t kManySetBytes = size_t(1) << 30;
constexpr size_t kManyMaxDefault = 1024;
constexpr size_t kManyPackLongFrom = 16;

static int many_window(const bn_ctx* c) { return c->many_window ? c->many_window : kManyWindow; }
static MsmManyLimits many_limits(const bn_ctx* c) {
    const int cw = many_window(c);
    const size_t per_term = (sizeof(bn_g1) << (cw - 1)) + (size_t)msm_windows(cw);
    const size_t chunk = c->many_chunk ? c->many_chunk : std::min(kManySetTerms, kManySetBytes / per_term);
    return {(uint32_t)c->many_unit, c->many_max ? c->many_max : kManyMaxDefault, chunk, kManyLanes, kManyUnitAutoMax,
            c->many_max ? SIZE_MAX : kManyPackLongFrom};
}
// the buffers of a launch set of up to nt terms and nu units at the context's width, and
// the words of a call
static int many_grow(bn_ctx* c, size_t nt, size_t nu, size_t words) {
    const int cw = many_window(c);
    RET_IF(c->many_digits.grow(c, (size_t)msm_many_digits(nt, cw)));
    RET_IF(c->many_table.grow(c, (size_t)msm_many_entries(nt, cw)));
    RET_IF(c->many_parts.grow(c, nu));
    return c->many_words.grow(c, c->many_fence, words);
}
// Refusals, before any point buffer is read (offsets is the host's control array).  m is
// not 0.
static int many_args(bn_ctx* c, const void* p, const void* k, const size_t* off, size_t m, const void* out) {
    if (const char* why = msm_many_offsets_refusal(off, m)) return fail(c, BN_ERR_INVALID_ARGUMENT, why);
    if (!out || (off[m] && (!p || !k))) return fail(c, BN_ERR_INVALID_ARGUMENT, "null buffer");
    return BN_OK;
}
// The words of every launch set of the call -> many_words.d in one copy on s in front of the
// call's kernels.  The pinned source is rewritten by the next call, which first waits for
// this copy (not for the kernels behind it); many_grow has waited for the last call's.
static int many_upload(bn_ctx* c, const MsmManyPlan& plan, const size_t* off, hipStream_t s) {
    if (!plan.words) return BN_OK;
    msm_many_fill(plan, off, c->many_words.h);
    RET_IF(c->many_words.copy(c, plan.words, s));
    return c->many_fence.record(c, s);
}
// the device sequence on stream s: every packed item as one launch set through the shared
// buffers, every other segment through bn_g1_msm's path into its own output; the caller holds
// the lock and the workspace order
static int many_dev_impl(bn_ctx* c, const bn_g1* d_p, const bn_fr* d_k, const size_t* off, size_t m, bn_g1* d_out,
                         size_t out_stride, hipStream_t s) {
    const int cw = many_window(c);
    const MsmManyPlan plan = msm_many_plan(many_limits(c), off, m);
    if (plan.set_terms > 0xffffffffull || plan.set_units > 0xffffffffull)
        return fail(c, BN_ERR_INTERNAL, "launch set exceeds its 32-bit offsets");
    RET_IF(many_grow(c, plan.set_terms, plan.set_units, plan.words));
    RET_IF(many_upload(c, plan, off, s));
    for (const MsmManyItem& it : plan.items) {
        const size_t lo = off[it.j0], nt = off[it.j1] - lo, mc = it.j1 - it.j0;
        if (!it.packed) {
            RET_IF(msm_dev_impl(c, d_p + lo, d_k + lo, nt, d_out + it.j0 * out_stride, s, 1));
            continue;
        }
        if (nt > c->many_table.cap() >> (cw - 1) || it.units > c->many_parts.cap())
            return fail(c, BN_ERR_INTERNAL, "launch set exceeds the workspace");
        const uint32_t* unit_off = c->many_words.d + it.words_at;
        if (nt) {
            k_g1_msm_many_table<<<grid_for(nt), kBlock, 0, s>>>(d_p + lo, d_k + lo, (uint32_t)nt, cw, c->many_digits,
                                                                c->many_table);
            k_g1_msm_many_unit<<<grid_for(it.units), kBlock, 0, s>>>(c->many_digits, c->many_table, (uint32_t)nt, cw,
                                                                     unit_off, (uint32_t)it.units, c->many_parts);
        }
        k_g1_msm_many_finish<<<grid_for(mc), kBlock, 0, s>>>(c->many_parts, (uint32_t)it.units, unit_off + it.units + 1,
                                                             mc, d_out + it.j0 * out_stride, out_stride);
        HIPCHK(c, hipGetLastError());
    }
    return BN_OK;
}

extern "C" {

size_t bn_g1_prepared_table_bytes(size_t k, int cw) {
    const uint64_t nent = (cw == 0 || msm_window_ok(cw)) ? msm_fixed_entries(k, cw) : 0;
    return nent ? (size_t)(nent * 2 * sizeof(bn_fq) + k) : 0;
}
int bn_g1_bases_prepare(bn_ctx* c, const bn_g1* bases, size_t k, int cw, bn_g1_prepared** out) {
    CTX_GUARD(c);
    RET_IF(g1_prepare_args(c, bases, k, cw, out));
    RET_IF(ws_acquire(c, c->stream));
    WsUse use{c, c->stream};
    return g1_prepare(c, bases, false, k, cw, out, c->stream);
}
int bn_g1_bases_prepare_dev(bn_ctx* c, const bn_g1* d_bases, size_t k, int cw, bn_g1_prepared** out, void* stream) {
    CTX_GUARD(c);
    RET_IF(g1_prepare_args(c, d_bases, k, cw, out));
    const hipStream_t s = pick(c, stream);
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return g1_prepare(c, d_bases, true, k, cw, out, s);
}
size_t bn_g1_prepared_count(const bn_g1_prepared* h) { return h ? h->k : 0; }
int bn_g1_prepared_window(const bn_g1_prepared* h) { return h ? h->c : 0; }
int bn_g1_prepared_destroy(bn_ctx* c, bn_g1_prepared* h) {
    CTX_GUARD(c);
    return c->g1_prepared.destroy(c, h, "not a live prepared handle of this context");
}
int bn_g1_msm_prepared_many(bn_ctx* c, const bn_g1_prepared* h, const bn_fr* k, size_t m, bn_g1* out, size_t out_stride) {
    CTX_GUARD_HOST(c);
    RET_IF(msm_prepared_args(c, h, k, m, out, out_stride));
    if (m == 0) return BN_OK;
    void* at[2];  // the sums, the scalars
    RET_IF(stage_regions(c, {m * sizeof(bn_g1), m * h->k * sizeof(bn_fr)}, at));
    HIPCHK(c, hipMemcpyAsync(at[1], k, m * h->k * sizeof(bn_fr), hipMemcpyHostToDevice, c->stream));
    RET_IF(msm_prepared_dev_impl(c, h, (const bn_fr*)at[1], m, (bn_g1*)at[0], 1, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(out, out_stride * sizeof(bn_g1), at[0], sizeof(bn_g1), sizeof(bn_g1), m,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BN_OK;
}
int bn_g1_msm_prepared_many_dev(bn_ctx* c, const bn_g1_prepared* h, const bn_fr* d_k, size_t m, bn_g1* d_out,
                                size_t out_stride, void* stream) {
    CTX_GUARD(c);
    RET_IF(msm_prepared_args(c, h, d_k, m, d_out, out_stride));
    if (m == 0) return BN_OK;
    hipStream_t s = pick(c, stream);
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return msm_prepared_dev_impl(c, h, d_k, m, d_out, out_stride, s);
}
size_t bn_g1_basis_table_bytes(size_t nbases, int cw) { return basis_table_bytes<bn_g1>(nbases, cw); }
int bn_g1_basis_prepare(bn_ctx* c, const bn_g1* bases, size_t nbases, int cw, bn_g1_basis** out) {
    return basis_prepare(c, bases, false, nbases, cw, out, nullptr);
}
int bn_g1_basis_prepare_dev(bn_ctx* c, const bn_g1* d_bases, size_t nbases, int cw, bn_g1_basis** out, void* stream) {
    return basis_prepare(c, d_bases, true, nbases, cw, out, stream);
}
size_t bn_g1_basis_count(const bn_g1_basis* h) { return h ? h->nbases : 0; }
int bn_g1_basis_window(const bn_g1_basis* h) { return h ? h->c : 0; }
int bn_g1_basis_destroy(bn_ctx* c, bn_g1_basis* h) { return basis_destroy<bn_g1>(c, h); }
int bn_g1_msm_basis(bn_ctx* c, const bn_g1_basis* h, const bn_fr* k, size_t n, bn_g1* out) {
    return msm_basis_host(c, h, k, n, out);
}
int bn_g1_msm_basis_dev(bn_ctx* c, const bn_g1_basis* h, const bn_fr* d_k, size_t n, bn_g1* d_out, void* stream) {
    return msm_basis_dev(c, h, d_k, n, d_out, stream);
}
int bn_g1_msm_basis_reserve(bn_ctx* c, const bn_g1_basis* h, size_t n) { return msm_basis_reserve<bn_g1>(c, h, n); }
int bn_g1_msm_basis_many(bn_ctx* c, const bn_g1_basis* h, const bn_fr* k, size_t k_stride, size_t m, size_t n, bn_g1* out,
                         size_t out_stride) {
    return msm_basis_many_host(c, h, k, k_stride, m, n, out, out_stride);
}
int bn_g1_msm_basis_many_dev(bn_ctx* c, const bn_g1_basis* h, const bn_fr* d_k, size_t k_stride, size_t m, size_t n,
                             bn_g1* d_out, size_t out_stride, void* stream) {
    return msm_basis_many_dev(c, h, d_k, k_stride, m, n, d_out, out_stride, stream);
}
int bn_g1_msm_basis_many_reserve(bn_ctx* c, const bn_g1_basis* h, size_t m, size_t n) {
    return msm_basis_many_reserve<bn_g1>(c, h, m, n);
}
int bn_set_msm_basis_many_set(bn_ctx* c, size_t vectors) {
    if (c && vectors > kMsmBasisManyMaxVectors)
        return fail(c, BN_ERR_INVALID_ARGUMENT, "at most 2^26 vectors per launch set (0: default)");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_basis_many_set(d, vectors); });
    CTX_GUARD(c);
    c->msm_g1.basis_many_set = vectors;
    return BN_OK;
}
size_t bn_g2_basis_table_bytes(size_t nbases, int cw) { return basis_table_bytes<bn_g2>(nbases, cw); }
int bn_g2_basis_prepare(bn_ctx* c, const bn_g2* bases, size_t nbases, int cw, bn_g2_basis** out) {
    return basis_prepare(c, bases, false, nbases, cw, out, nullptr);
}
int bn_g2_basis_prepare_dev(bn_ctx* c, const bn_g2* d_bases, size_t nbases, int cw, bn_g2_basis** out, void* stream) {
    return basis_prepare(c, d_bases, true, nbases, cw, out, stream);
}
size_t bn_g2_basis_count(const bn_g2_basis* h) { return h ? h->nbases : 0; }
int bn_g2_basis_window(const bn_g2_basis* h) { return h ? h->c : 0; }
int bn_g2_basis_destroy(bn_ctx* c, bn_g2_basis* h) { return basis_destroy<bn_g2>(c, h); }
int bn_g2_msm_basis(bn_ctx* c, const bn_g2_basis* h, const bn_fr* k, size_t n, bn_g2* out) {
    return msm_basis_host(c, h, k, n, out);
}
int bn_g2_msm_basis_dev(bn_ctx* c, const bn_g2_basis* h, const bn_fr* d_k, size_t n, bn_g2* d_out, void* stream) {
    return msm_basis_dev(c, h, d_k, n, d_out, stream);
}
int bn_g2_msm_basis_reserve(bn_ctx* c, const bn_g2_basis* h, size_t n) { return msm_basis_reserve<bn_g2>(c, h, n); }
int bn_g1_msm_many(bn_ctx* c, const bn_g1* p, const bn_fr* k, const size_t* offsets, size_t m, bn_g1* out,
                   size_t out_stride) {
    CTX_GUARD_HOST(c);
    if (out_stride == 0) return fail(c, BN_ERR_INVALID_ARGUMENT, "out_stride is 0");
    if (m == 0) return BN_OK;
    RET_IF(many_args(c, p, k, offsets, m, out));
    const size_t n = offsets[m];
    void* at[3];  // the sums, the points, the scalars
    RET_IF(stage_regions(c, {m * sizeof(bn_g1), n * sizeof(bn_g1), n * sizeof(bn_fr)}, at));
    int rc = [&]() -> int {
        if (n) {
            HIPCHK(c, hipMemcpyAsync(at[1], p, n * sizeof(bn_g1), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(at[2], k, n * sizeof(bn_fr), hipMemcpyHostToDevice, c->stream));
        }
        RET_IF(many_dev_impl(c, (const bn_g1*)at[1], (const bn_fr*)at[2], offsets, m, (bn_g1*)at[0], 1, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(out, out_stride * sizeof(bn_g1), at[0], sizeof(bn_g1), sizeof(bn_g1), m,
                                   hipMemcpyDeviceToHost, c->stream));
        return BN_OK;
    }();
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == BN_OK) rc = fail(c, BN_ERR_HIP, "hipStreamSynchronize");
    return rc;
}
int bn_g1_msm_many_dev(bn_ctx* c, const bn_g1* d_p, const bn_fr* d_k, const size_t* offsets, size_t m, bn_g1* d_out,
                       size_t out_stride, void* stream) {
    CTX_GUARD(c);
    if (out_stride == 0) return fail(c, BN_ERR_INVALID_ARGUMENT, "out_stride is 0");
    if (m == 0) return BN_OK;
    RET_IF(many_args(c, d_p, d_k, offsets, m, d_out));
    hipStream_t s = pick(c, stream);
    RET_IF(ws_acquire(c, s));
    WsUse use{c, s};
    return many_dev_impl(c, d_p, d_k, offsets, m, d_out, out_stride, s);
}
int bn_set_msm_many_window(bn_ctx* c, int bits) {
    if (c && bits != 0 && !msm_many_window_ok(bits))
        return fail(c, BN_ERR_INVALID_ARGUMENT, "window width outside 2 .. 8 (0: default)");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_many_window(d, bits); });
    CTX_GUARD(c);
    c->many_window = bits;
    return BN_OK;
}
int bn_set_msm_many_unit(bn_ctx* c, int terms) {
    if (c && (terms < 0 || terms > (int)kMsmManyMaxUnitTerms))
        return fail(c, BN_ERR_INVALID_ARGUMENT, "terms per unit outside 1 .. 64 (0: automatic)");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_many_unit(d, terms); });
    CTX_GUARD(c);
    c->many_unit = terms;
    return BN_OK;
}
int bn_set_msm_many_max(bn_ctx* c, size_t terms) {
    if (c && terms > kMsmManyMaxSegment)
        return fail(c, BN_ERR_INVALID_ARGUMENT, "at most 4096 terms per packed segment (0: default)");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_many_max(d, terms); });
    CTX_GUARD(c);
    c->many_max = terms;
    return BN_OK;
}
int bn_set_msm_many_chunk(bn_ctx* c, size_t terms) {
    if (c && terms > kMsmManyMaxTerms)
        return fail(c, BN_ERR_INVALID_ARGUMENT, "at most 2^26 terms per launch set (0: default)");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_many_chunk(d, terms); });
    CTX_GUARD(c);
    c->many_chunk = terms;
    return BN_OK;
}
int bn_g1_msm_many_reserve(bn_ctx* c, size_t terms, size_t segments) {
    CTX_GUARD(c);
    if (terms > kMsmManyMaxTerms || segments > kMsmManyMaxTerms)
        return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 terms or segments");
    // a set holds at most the chunk's terms, or one segment of at most `max`; a unit has at
    // least one term; a call's words are its units, its segments and two per set
    const MsmManyLimits lim = many_limits(c);
    const size_t st = std::min(terms, std::max(lim.chunk, kMsmManyMaxSegment));
    return many_grow(c, st, st, terms + 3 * segments + 2);
}
int bn_set_msm_prepared_lanes(bn_ctx* c, int lanes) {
    if (c && lanes != 0 && !msm_fixed_lanes_ok(lanes))
        return fail(c, BN_ERR_INVALID_ARGUMENT, "lanes per output must be 0 (automatic) or a power of two from 1 to 64");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_prepared_lanes(d, lanes); });
    CTX_GUARD(c);
    c->msm_g1.fixed_lanes = lanes;
    return BN_OK;
}

int bn_internal_g1_msm_partial(bn_ctx* c, const bn_g1* p, const bn_fr* k, size_t n, bn_g1* out) {
    return msm_host(c, p, k, n, out, 0);
}
int bn_internal_g1_sum(bn_ctx* c, const bn_g1* a, size_t m, bn_g1* out) { return msm_sum_host(c, a, m, out); }
int bn_internal_g2_msm_partial(bn_ctx* c, const bn_g2* p, const bn_fr* k, size_t n, bn_g2* out) {
    return msm_host(c, p, k, n, out, 0);
}
int bn_internal_g2_sum(bn_ctx* c, const bn_g2* a, size_t m, bn_g2* out) { return msm_sum_host(c, a, m, out); }
int bn_g1_msm(bn_ctx* c, const bn_g1* p, const bn_fr* k, size_t n, bn_g1* out) {
    if (is_multi(c)) return bn_multi_g1_msm(c, p, k, n, out);
    return msm_host(c, p, k, n, out, 1);
}
int bn_g1_msm_dev(bn_ctx* c, const bn_g1* d_p, const bn_fr* d_k, size_t n, bn_g1* d_out, void* stream) {
    return msm_dev(c, d_p, d_k, n, d_out, stream);
}
int bn_g2_msm(bn_ctx* c, const bn_g2* p, const bn_fr* k, size_t n, bn_g2* out) {
    if (is_multi(c)) {
        // the cap is on the whole sum, not on a shard
        if (n > kMsmMaxTerms) return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 terms");
        return bn_multi_g2_msm(c, p, k, n, out);
    }
    return msm_host(c, p, k, n, out, 1);
}
int bn_g2_msm_dev(bn_ctx* c, const bn_g2* d_p, const bn_fr* d_k, size_t n, bn_g2* d_out, void* stream) {
    return msm_dev(c, d_p, d_k, n, d_out, stream);
}
int bn_set_msm_window(bn_ctx* c, int bits) {
    if (c && bits != 0 && !msm_window_ok(bits))
        return fail(c, BN_ERR_INVALID_ARGUMENT, "window width outside 2 .. 16 (0: automatic)");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_window(d, bits); });
    CTX_GUARD(c);
    c->msm_g1.window = bits;
    c->msm_g2.window = bits;
    return BN_OK;
}
int bn_set_msm_min(bn_ctx* c, size_t n) {
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_min(d, n); });
    CTX_GUARD(c);
    c->msm_g1.min = n;
    c->msm_g2.min = n;
    return BN_OK;
}
int bn_set_msm_run_max(bn_ctx* c, size_t entries) {
    if (c && entries != BN_MSM_RUN_UNSPLIT && entries > kMsmRunMax)
        return fail(c, BN_ERR_INVALID_ARGUMENT, "run cap outside 1 .. 65536 (0: default, BN_MSM_RUN_UNSPLIT: never split)");
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_set_msm_run_max(d, entries); });
    CTX_GUARD(c);
    c->msm_g1.run_max = entries;
    c->msm_g2.run_max = entries;
    return BN_OK;
}
int bn_msm_reserve(bn_ctx* c, size_t n) {
    if (is_multi(c)) return for_each_sub(c, [&](bn_ctx* d) { return bn_msm_reserve(d, n / c->subs.size() + 1); });
    return msm_reserve_terms<bn_g1>(c, n);
}
int bn_g2_msm_reserve(bn_ctx* c, size_t n) {
    if (is_multi(c)) {
        if (n > kMsmMaxTerms) return fail(c, BN_ERR_INVALID_ARGUMENT, "more than 2^26 terms");
        return for_each_sub(c, [&](bn_ctx* d) { return bn_g2_msm_reserve(d, n / c->subs.size() + 1); });
    }
    return msm_reserve_terms<bn_g2>(c, n);
}

}  // extern "C"
