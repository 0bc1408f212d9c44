// capi_internal.h -- what the host units of the C ABI share (capi.hip, capi_products.hip,
// capi_msm.hip): the workspace's ordering, staging of host buffers, the device outcome
// word.  Error plumbing and the owning types of the context's memory: ctx_mem.h.  Not a
// public header.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "kernels.h"
#include "ctx.h"

#pragma GCC visibility push(hidden)  // nothing here is part of the library's interface
namespace bn {

// (fail, HIPCHK, RET_IF and ws_drain: ctx_mem.h and ctx.h)
// order this call's device work after the workspace's previous user (see bn_ctx)
inline int ws_acquire(bn_ctx* c, hipStream_t s) {
    if (c->ws_pending) HIPCHK(c, hipStreamWaitEvent(s, c->ws_event, 0));
    return BN_OK;
}
// ... and mark this call's work as the workspace's latest user (scope exit)
struct WsUse {
    bn_ctx* c;
    hipStream_t s;
    ~WsUse() {
        if (hipEventRecord(c->ws_event, s) == hipSuccess) c->ws_pending = true;
    }
};

#define CTX_GUARD(ctx)                                 \
    if (!(ctx)) return BN_ERR_INVALID_ARGUMENT;        \
    if (!(ctx)->subs.empty())                          \
        return fail((ctx), BN_ERR_INVALID_ARGUMENT,    \
                    "not available on a multi-device context; use bn_ctx_device()"); \
    std::lock_guard<std::mutex> lock_((ctx)->mu);      \
    HIPCHK(ctx, hipSetDevice((ctx)->device))
// host-buffer entry points: the lock for the whole call, and the context stream
// ordered after the workspace's previous user
#define CTX_GUARD_HOST(ctx)                \
    CTX_GUARD(ctx);                        \
    RET_IF(ws_acquire((ctx), (ctx)->stream)); \
    WsUse ws_use_{(ctx), (ctx)->stream}

// a setting of a multi-device context goes to every sub-context
inline bool is_multi(const bn_ctx* c) { return c && !c->subs.empty(); }
template <class F>
int for_each_sub(bn_ctx* c, F&& set) {
    for (bn_ctx* d : c->subs) RET_IF(set(d));
    return BN_OK;
}

// for (auto [off, m] : chunks(n)): the launch sets of n elements, kChunk at a time
// (the range is its own iterator: it stands at `off` and ends at n)
struct Chunk {
    size_t off, m;
};
struct Chunks {
    size_t off, n;
    Chunk operator*() const { return {off, std::min(n - off, kChunk)}; }
    void operator++() { off += kChunk; }
    bool operator!=(const Chunks&) const { return off < n; }
    Chunks begin() const { return *this; }
    Chunks end() const { return *this; }
};
inline Chunks chunks(size_t n) { return {0, n}; }

inline hipStream_t pick(bn_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }
inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- defined in capi.hip
// the workspace for n pairings / the stage for `bytes` (grown, never shrunk; growing drains)
BN_HIDDEN int reserve(bn_ctx* c, size_t n);
BN_HIDDEN int stage(bn_ctx* c, size_t bytes);
BN_HIDDEN int prepare(bn_ctx* c, const bn_g1* d_p, const bn_g2* d_q, size_t m, int mode, hipStream_t s, int scale = 1,
                      bool scaled_inputs = false);
BN_HIDDEN int run_fe(bn_ctx* c, const uint32_t* f, size_t n, const uint8_t* flags, bn_gt* out, uint8_t* ok,
                     hipStream_t s);
// the Miller values of n <= c->cap device pairs from one k_pairing_latency launch (mode 0:
// a pair with a zero point gives one; no launch when n == 0) -> *f, split layout, stride n,
// in a region of the workspace's slots that slot 0's n values do not reach
BN_HIDDEN int latency_values(bn_ctx* c, const bn_g1* d_p, const bn_g2* d_q, size_t n, hipStream_t s, uint32_t** f);
BN_HIDDEN int miller_product_dev(bn_ctx* c, const bn_g1* d_p, const bn_g2* d_q, size_t n, int mode, bn_gt* d_out,
                                 hipStream_t s);
BN_HIDDEN int batch_host(bn_ctx* c, const bn_g1* p, const bn_g2* q, size_t n, int mode, bool do_fe, bn_gt* out);
BN_HIDDEN void g1_mul_launch(const bn_g1* d_p, const bn_fr* d_k, size_t n, bn_g1* d_out, hipStream_t s);
BN_HIDDEN void g2_mul_launch(const bn_g2* d_p, const bn_fr* d_k, size_t n, bn_g2* d_out, hipStream_t s);

// One stage() for regions of the given byte sizes, laid out in order: at[i] is region
// i's device pointer, 256-aligned.  The pointers hold until the next stage().
inline int stage_regions(bn_ctx* c, const size_t* bytes, size_t n, void** at) {
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) total += round256(bytes[i]);
    RET_IF(stage(c, total));
    uint8_t* p = c->stage;
    for (size_t i = 0; i < n; ++i) {
        at[i] = p;
        p += round256(bytes[i]);
    }
    return BN_OK;
}
template <size_t N>
int stage_regions(bn_ctx* c, const size_t (&bytes)[N], void* (&at)[N]) {
    return stage_regions(c, bytes, N, at);
}

// The device outcome word is two: d_err[0], which the kernels set, and d_err[1], where
// bn_*_batch_dev (which report d_err[0] alone through their own status word) put aside
// what the calls before them left (k_err_hold).  check_err reads both, clear_err clears both.
constexpr size_t kErrWords = 2;
// the device outcome bits of the calls since the last clear; a wave hand-off that
// ran out of its wait cap (BN_ERR_INTERNAL) fails the call here, whatever else is set
inline int check_err(bn_ctx* c, hipStream_t s, int* out_bits) {
    int h[kErrWords] = {};
    HIPCHK(c, hipMemcpyAsync(h, c->d_err, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *out_bits = h[0] | h[1];
    if (*out_bits & (1 << BN_ERR_INTERNAL))
        return fail(c, BN_ERR_INTERNAL, "device wave hand-off timed out; result discarded");
    return BN_OK;
}
inline int clear_err(bn_ctx* c, hipStream_t s) {
    HIPCHK(c, hipMemsetAsync(c->d_err, 0, kErrWords * sizeof(int), s));
    return BN_OK;
}
// the outcome bits a call reports (`mask`: those it can set) as its return code
constexpr int kBitBadIndex = 1 << BN_ERR_INVALID_ARGUMENT;
constexpr int kBitToAffine = 1 << BN_ERR_TO_AFFINE;
constexpr int kBitFeZero = 1 << BN_ERR_FE_ZERO;
inline int outcome(bn_ctx* c, int bits, int mask) {
    bits &= mask;
    if (bits & kBitBadIndex)  // bn_pairing_prepared_many_dev: an index past the handle's points
        return fail(c, BN_ERR_INVALID_ARGUMENT, "a prepared-point index was out of range; that row is zero");
    if (bits & kBitToAffine) return fail(c, BN_ERR_TO_AFFINE, "ToAffineConversion");
    if (bits & kBitFeZero) return fail(c, BN_ERR_FE_ZERO, "miller loop cannot produce zero");
    return BN_OK;
}

// Fq::one() (R mod p), and with it Fq12::one(): c0.c0.c0 = one.  Read-only images: no
// thread ever writes them, so an asynchronous copy may read them after the call.
constexpr bn_fq kFqOne = {{0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full}};
inline constexpr bn_gt kGtOne = {{kFqOne}};
inline void gt_one(bn_gt* out) { *out = kGtOne; }

// Threads per block of k_miller_products(_mapped).  A launch set of fewer lane pairs than
// fill the GPU with kPairBlock-thread blocks leaves whole CUs idle while the busy ones run
// two waves per SIMD, each at about half the lone-wave rate: smaller blocks spread the same
// waves over more SIMDs.  $BN254MI_PRODUCTS_BLOCK (128, 256 or 512) forces one size (A/B).
inline unsigned products_block(const bn_ctx* c, size_t lanes) {
    if (c->products_block) return c->products_block;
    const size_t cus = c->lat_w1_max / kLatPairs;  // the device's CU count (bn_ctx_create)
    if (lanes >= cus * kPairBlock) return kPairBlock;
    return lanes >= cus * 256 ? 256 : 128;
}

}  // namespace bn
#pragma GCC visibility pop
