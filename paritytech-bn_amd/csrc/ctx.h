// ctx.h -- the bn_ctx behind the C ABI (host side, shared by capi.hip, capi_products.hip,
// capi_msm.hip and capi_multi.hip).  Not a public header.  Everything a context holds on
// the device or in pinned memory is a member of an owning type (ctx_mem.h): `delete c` frees
// it, and so does deleting a handle; only the streams and the events named in capi.hip's
// ctx_teardown are released by hand, in their order.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bn254mi.h"
#include "ctx_mem.h"
#include "tail_epoch.h"

#pragma GCC visibility push(hidden)  // the owning members' destructors are not part of the library's interface

// One group's settings and point buffers of the multi-scalar multiplication (P = bn_g1
// or bn_g2): buckets the bucket sums, parts the segment and window partial sums, tmp
// the small path's n products; fixed the lanes' partial sums of the prepared-bases MSM
// (bn_g1_msm_prepared_many, G1 only so far).
template <class P>
struct MsmGroupWs {
    int window = 0;  // bits; 0: chosen from n (capi_msm.hip MsmGroup<P>::auto_window)
    size_t min = 0;  // batches below this many terms take the small path
    bn::DevBuf<P> buckets, parts, tmp;
    // the run cap (msm.h): 0 the default rule, (size_t)-1 never split; run_a / run_b the partial
    // sums of the overlong runs, the even and the odd levels of the chunk and fold tree
    size_t run_max = 0;
    bn::DevBuf<P> run_a, run_b;
    int fixed_lanes = 0;  // lanes per output of the lookup kernel; 0: chosen from m and k (msm_fixed.h)
    bn::DevBuf<P> fixed;
    // vectors per launch set of the batched fixed-basis MSM (bn_g1_msm_basis_many); 0: from the
    // bound on bucket memory (msm_basis_many.h)
    size_t basis_many_set = 0;
};

// bn_g2_prepare's handle: the 87 line coefficients of each of nq affine G2 points
// (kernels.h kPreparedWords words per point), a zero flag per point and the points as they
// were given (for the products' wide path, whose kernel takes points), device-resident and
// freed with the handle, which the single-device context owns whose `prepared` list holds it
// (bn::HandleList: it deletes the handles still alive when the context is destroyed).
struct bn_g2_prepared {
    size_t nq = 0;
    bn::DevBuf<uint32_t> table;
    bn::DevBuf<uint8_t> zero;  // zero[j] != 0: q[j] was G2::zero(), its table row is never used
    bn::DevBuf<bn_g2> points;  // q[0 .. nq)
};

// bn_g1_bases_prepare's handle: the window table of k G1 bases at width c (msm_fixed.h:
// nent affine entries of two bn_fq each) and a zero flag per base, device-resident, owned
// like a bn_g2_prepared by the single-device context whose `g1_prepared` list holds it.
struct bn_g1_prepared {
    size_t k = 0;
    int c = 0;
    uint32_t nent = 0;
    bn::DevBuf<bn_fq> table;
    bn::DevBuf<uint8_t> zero;  // zero[b] != 0: bases[b] had z == 0, its entries are never added
};

// bn_g1_basis_prepare's handle: for each of nbases G1 bases the W(c) affine points
// 2^(c w) * base (msm_basis.h: window major, two bn_fq each) and a zero flag per base,
// device-resident, owned like a bn_g1_prepared by the single-device context whose `g1_basis`
// list holds it.
struct bn_g1_basis {
    size_t nbases = 0;
    int c = 0;
    bn::DevBuf<bn_fq> table;
    bn::DevBuf<uint8_t> zero;  // zero[b] != 0: bases[b] had z == 0, its entries are never added
};

// bn_g2_basis_prepare's handle: the same for nbases G2 bases (two bn_fq2 per entry, stored as
// the two lane halves [x.c0, y.c0 | x.c1, y.c1]: kernels_msm_basis_g2.hip), owned by the
// single-device context whose `g2_basis` list holds it.
struct bn_g2_basis {
    size_t nbases = 0;
    int c = 0;
    bn::DevBuf<bn_fq2> table;
    bn::DevBuf<uint8_t> zero;  // zero[b] != 0: bases[b] had z == 0, its entries are never added
};

#pragma GCC visibility pop

struct bn_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // last error message; a multi-device context's host-buffer calls write it
    // without holding `mu` (their sub-contexts do the locking), so writes there
    // take err_mu
    std::mutex err_mu;
    std::string err;
    // workspace (device): four buffers under one capacity (bn::reserve)
    size_t cap = 0;  // pairings
    bn::DevBuf<uint32_t> coeffs, paff;
    bn::DevBuf<uint32_t> slots;  // Fq12 slots of the step machine; slot 0 = Miller values
    bn::DevBuf<uint8_t> flags;
    bn::DevBuf<uint32_t> d_prog;  // final-exponentiation step program
    // optional per-phase timing of bn_pairing_many_dev (HIP events on the launch stream)
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::array<hipEvent_t, 5>> ev_marks;
    int fe_steps = 0;
    int fe_out = 0;
    bool fe_last_out = false;  // the program's last step writes fe_out (k_pairing_full)
    // batches of at most this many elements run the final exponentiation on the
    // wide layout (kernels_wide.hip, 16 lanes per element: latency) instead of
    // the step machine (k_fq12_vm, 2 lanes per element: throughput)
    size_t fe_wide_max = 0;
    // bn_fq12_op_many's step machine: 0 = k_fq12_vm (kernels_fe.hip), 1 = k_fq12_vm_pairing
    // (kernels_pairing.hip: the build of the operations that k_pairing_full runs)
    int fq12_op_unit = 0;
    // A/B switch ($BN254MI_MILLER_FORM) for bn_pairing_many_dev batches above the
    // wide threshold: 1 (default, measured fastest) = to_affine,
    // line steps and Miller loop fused in one kernel (k_pairing_fused, no
    // coefficient traffic); 0 = k_prepare (line coefficients to HBM) + k_miller;
    // 2 = k_prepare + k_miller_seg with one segment
    int miller_form = 3;  // 3: k_pairing_full; 1: k_pairing_fused + k_fq12_vm + k_fe_out; 0/2: k_prepare + k_miller(_seg) + ...
    // bn_pairing_many_dev batches of at most this many pairs run k_pairing_latency
    size_t latency_max = 0;
    bool latency_w2 = true;  // above lat_w1_max pairs the one-launch path runs the two-wave build
    size_t lat_w1_max = 2048;  // CU count x kLatPairs (bn_ctx_create): one round of one-wave blocks
    // batches of at most this many pairs take k_prepare_wide (8 lanes per pair)
    size_t prepare_wide_max = 0;
    bn::DevBuf<int> d_err;  // two words: the kernels' outcome bits, and those put aside by k_err_hold (capi_internal.h)
    // pairing_batch's one-launch tail (kernels_tail.hip k_seg_tail): its own words
    // (kTailWsWords, zeroed at creation), every word it polls stamped with the
    // launch's epoch, so no clearing between products.  tail_epoch serves k_fe_ds too; it
    // runs 1 .. tail_epoch_wrap and then returns to 1, and the launch that gets 1 again
    // zeroes tail_ws and fe_ds_ws first (tail_epoch.h; $BN254MI_TAIL_EPOCH_WRAP, for tests)
    bn::DevBuf<uint32_t> tail_ws;
    uint32_t tail_epoch = 0;
    uint32_t tail_epoch_wrap = bn::kTailEpochWrapDefault;
    // pairing_many of at most fe_ds_max pairs: k_pairing_latency's Miller values, then
    // k_fe_ds (three digit-sliced blocks per pair); its words (kFeDsMax pairs, zeroed)
    bn::DevBuf<uint32_t> fe_ds_ws;
    size_t fe_ds_max = 0;
    // staging for host-buffer calls (device), in bytes
    bn::DevBuf<uint8_t> stage;
    // bn_pairing_many's host pipeline (capi.hip): two pinned bounce buffers, the
    // copy streams and the per-buffer events (created with the context, released by hand);
    // $BN254MI_HOST_PIPELINE: 1 (default) pipeline above one piece, 0 never
    // (pageable A/B form), 2 always
    int host_pipeline = 1;
    size_t host_piece = 0;  // pairs per piece (kHostPiece; $BN254MI_HOST_PIECE, at most kChunk)
    bn::PinBuf<uint8_t> pin;
    hipStream_t h2d = nullptr, d2h = nullptr;
    hipEvent_t ev_in[2] = {}, ev_comp[2] = {}, ev_out[2] = {};
    // The workspace (coeffs, paff, slots, flags, d_err, stage) is shared by every
    // call on this context.  Host-side, the mutex serializes the calls; device-side,
    // every workspace user records ws_event on its stream when it has enqueued its
    // work, and the next user's stream waits on that event first (WsUse), so _dev
    // calls on different caller streams run in call order instead of racing on the
    // same buffers.  No caller stream is remembered past its call.
    hipEvent_t ws_event = nullptr;
    bool ws_pending = false;
    // Multi-scalar multiplication (bn_g1_msm, bn_g2_msm; kernels_msm.hip,
    // kernels_msm_g2.hip).  Its workspace is its own (not part of bn_workspace_bytes),
    // grown by bn_msm_reserve / bn_g2_msm_reserve or on first use, ordered like the
    // shared one (ws_event) and freed with the context.  Both groups share the integer
    // buffers: msm_keys = counts | cursors | offsets | long keys of the (window, bucket) keys,
    // msm_sorted the entries sorted by key.  Each group has its own settings and point
    // buffers (MsmGroupWs).
    bn::DevBuf<uint32_t> msm_keys, msm_sorted;
    MsmGroupWs<bn_g1> msm_g1;
    MsmGroupWs<bn_g2> msm_g2;
    // bn_pairing_batch_many (capi_products.hip): calls with fewer than products_min products of at
    // most kProductLaneMax terms run each on the single-product path; the packed path
    // takes at most products_chunk terms per launch set.  Its chunk-relative 32-bit
    // offsets go up through the channel prod_off (pinned h into d), one upload per call in
    // front of its kernels; prod_fence marks that upload done, and the next call waits
    // for it before it rewrites prod_off.h.
    size_t products_min = 0;
    size_t products_chunk = 0;
    unsigned products_block = 0;  // threads per block of k_miller_products; 0: by the launch set's size
    bn::UploadChannel prod_off;
    bn::Fence prod_fence;
    // bn_pairing_batch_prepared_many: the per-term words of every launch set of a call (per
    // set the term map, then the prepared slots' terms and table indices, then the fresh
    // slots' terms), uploaded with the offsets under the same fence; and the _dev form's
    // gathered G1 points of a set's fresh terms.  Both grow on first use, like prod_off.
    bn::UploadChannel prod_map;
    bn::DevBuf<bn_g1> prod_fresh;
    // The wide path of both product calls: calls of at most products_wide_max
    // terms run k_pairing_latency's Miller values and a 16-lane group per product (0: never).
    // prod_gq: the G2 points of a wide set of the prepared form in term order (k_g2_gather),
    // grown on first use.  products_routes: the products planned as {wide, packed, alone}
    // since bn_get_products_routes last read them (host counters).
    size_t products_wide_max = 0;
    bn::DevBuf<bn_g2> prod_gq;
    size_t products_routes[3] = {0, 0, 0};
    // the bn_g2_prepared handles this context made and has not destroyed yet (capi_products.hip).
    // Their tables are their own memory, not part of the workspace; the calls that read
    // them order themselves through ws_event like every workspace user, which is what
    // bn_g2_prepared_destroy waits for.
    bn::HandleList<bn_g2_prepared> prepared;
    // the same for the bn_g1_prepared handles (capi_msm.hip)
    bn::HandleList<bn_g1_prepared> g1_prepared;
    // and for the bn_g1_basis handles (capi_msm.hip)
    bn::HandleList<bn_g1_basis> g1_basis;
    // and for the bn_g2_basis handles (capi_msm.hip)
    bn::HandleList<bn_g2_basis> g2_basis;
    // bn_g1_msm_many (capi_msm.hip, kernels_msm_many.hip).  Settings: 0 takes
    // the default (capi_msm.hip).  Its workspace is its own, like the MSM's: the digit bytes,
    // the multiples and the units' partial sums of one launch set, grown on first use or by
    // bn_g1_msm_many_reserve and ordered by ws_event; and the plan's words of every set of a
    // call (msm_many_plan.h), which go up through the channel many_words in one upload in front
    // of the call's kernels -- many_fence marks that upload done, and the next call
    // waits for it before it rewrites many_words.h.
    int many_window = 0, many_unit = 0;
    size_t many_max = 0, many_chunk = 0;
    bn::DevBuf<uint8_t> many_digits;
    bn::DevBuf<bn_g1> many_table, many_parts;
    bn::UploadChannel many_words;
    bn::Fence many_fence;
    // multi-device context (bn_ctx_create_multi): one single-device sub-context
    // per listed device; `device` is -1 and the fields above are unused
    std::vector<bn_ctx*> subs;
    std::vector<int> devices;
    void* comms = nullptr;  // RCCL communicators (capi_multi.hip), created on first use
};

#pragma GCC visibility push(hidden)
namespace bn {
inline int fail(bn_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
inline int ws_drain(bn_ctx* c) {
    if (c->ws_pending) HIPCHK(c, hipEventSynchronize(c->ws_event));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BN_OK;
}
}  // namespace bn
#pragma GCC visibility pop

// capi_multi.hip: the multi-device forms of the host-buffer entry points
#include "../../include/bn254mi.h"
#define BN_HIDDEN __attribute__((visibility("hidden")))
extern "C" {  // internal (not in bn254mi.h); C linkage matches their definitions' scope
BN_HIDDEN int bn_multi_pairing_many(bn_ctx* c, const bn_g1* p, const bn_g2* q, size_t n, bn_gt* out);
BN_HIDDEN int bn_multi_pairing_batch(bn_ctx* c, const bn_g1* p, const bn_g2* q, size_t n, bn_gt* out);
BN_HIDDEN int bn_multi_miller_loop_batch(bn_ctx* c, const bn_g2* q, const bn_g1* p, size_t n, bn_gt* out);
BN_HIDDEN int bn_multi_final_exponentiation_many(bn_ctx* c, const bn_gt* f, size_t n, bn_gt* out, uint8_t* ok);
BN_HIDDEN int bn_multi_miller_loop_many(bn_ctx* c, const bn_g1* p, const bn_g2* q, size_t n, bn_gt* out);
BN_HIDDEN int bn_multi_g1_mul_many(bn_ctx* c, const bn_g1* p, const bn_fr* k, size_t n, bn_g1* out);
BN_HIDDEN int bn_multi_g2_mul_many(bn_ctx* c, const bn_g2* p, const bn_fr* k, size_t n, bn_g2* out);
BN_HIDDEN int bn_multi_g1_msm(bn_ctx* c, const bn_g1* p, const bn_fr* k, size_t n, bn_g1* out);
BN_HIDDEN int bn_multi_g2_msm(bn_ctx* c, const bn_g2* p, const bn_fr* k, size_t n, bn_g2* out);
BN_HIDDEN int bn_multi_pairing_batch_many(bn_ctx* c, const bn_g1* p, const bn_g2* q, const size_t* offsets, size_t m,
                                          bn_gt* out);
BN_HIDDEN int bn_multi_destroy(bn_ctx* c);
// capi.hip / capi_msm.hip internals used by capi_multi.hip
BN_HIDDEN int bn_internal_miller_product(bn_ctx* c, const bn_g1* p, const bn_g2* q, size_t n, int mode, bn_gt* result);
BN_HIDDEN void bn_internal_gt_one(bn_gt* out);
// *out = the Jacobian (un-normalized) sum of p[i] * k[i], i < n
BN_HIDDEN int bn_internal_g1_msm_partial(bn_ctx* c, const bn_g1* p, const bn_fr* k, size_t n, bn_g1* out);
// *out = the returned image (normalized; zero as G1::zero()) of the sum of a[0 .. m)
BN_HIDDEN int bn_internal_g1_sum(bn_ctx* c, const bn_g1* a, size_t m, bn_g1* out);
// the same over G2
BN_HIDDEN int bn_internal_g2_msm_partial(bn_ctx* c, const bn_g2* p, const bn_fr* k, size_t n, bn_g2* out);
BN_HIDDEN int bn_internal_g2_sum(bn_ctx* c, const bn_g2* a, size_t m, bn_g2* out);
}
