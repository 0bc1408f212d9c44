/*
 * bn254mi.h -- C ABI of the MI355X BN254 pairing engine (libbn254mi.so).
 *
 * Drop-in boundary for the batched hot path of risc0/paritytech-bn
 * (crate substrate-bn 0.6.0).  The reference has no FFI; its boundary is the
 * public Rust API in src/lib.rs.  Each entry point below names the reference
 * function it replaces (file:line under /root/reference).  INTEGRATION.md shows
 * the Rust-side `extern "C"` binding a maintainer adds to keep
 * `pairing()/pairing_batch()/miller_loop_batch()/G1 * Fr` source-compatible.
 *
 * Value types are byte-identical to the reference's #[repr(C)] memory images,
 * so Rust slices pass zero-copy:
 *   bn_fq  == fields::Fq  == U256([u128;2]) : canonical x*2^256 mod p, little endian
 *   bn_fr  == fields::Fr  (Montgomery mod r, same layout)
 *   bn_g1  == groups::G1  == G<G1Params>{x,y,z}  (Jacobian; zero is z == 0)
 *   bn_g2  == groups::G2  (Jacobian over Fq2 {c0,c1})
 *   bn_gt  == Gt(Fq12)    12 Fq in order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1
 *
 * Every call returns BN_OK (0) or a bn_status code.  Host-buffer calls block
 * until the result is in the caller's buffer (the Rust API is synchronous).
 * *_dev calls take device pointers and enqueue on `stream` (a hipStream_t, or
 * NULL for the context's own stream) without synchronizing.
 */
#ifndef BN254MI_H
#define BN254MI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } bn_fq;
typedef struct { bn_fq c0, c1; } bn_fq2;
typedef struct { uint64_t l[4]; } bn_fr;
typedef struct { bn_fq x, y, z; } bn_g1;
typedef struct { bn_fq2 x, y, z; } bn_g2;
typedef struct { bn_fq c[12]; } bn_gt;

typedef enum {
    BN_OK = 0,
    BN_ERR_INVALID_ARGUMENT = 1,
    BN_ERR_TO_AFFINE = 2,     /* CurveError::ToAffineConversion (lib.rs:629-630) */
    BN_ERR_FE_ZERO = 3,       /* final exponentiation of zero: fq12.rs:63-72 None; pairing panics (mod.rs:900) */
    BN_ERR_HIP = 4,           /* a HIP runtime error; see bn_last_error() */
    BN_ERR_NO_DEVICE = 5,
    BN_ERR_INTERNAL = 6       /* a device-side hand-off between waves ran out of its wait cap; the result is
                                 not trusted and the call fails (never seen in normal operation) */
} bn_status;

typedef struct bn_ctx bn_ctx;

/* One context per device.  A context may be shared by host threads: each call holds
 * it for its whole duration (staging, kernels, readback).
 * Ordering across streams.  The *_dev calls that use a workspace of the context or read a
 * handle run on the device in call order, whatever streams they are enqueued on (the
 * workspaces are shared; each such call's stream first waits for the work of the one
 * before it).  They are: bn_pairing_many_dev, bn_pairing_batch_dev, bn_miller_loop_batch_dev,
 * bn_pairing_batch_many_dev, bn_g2_prepare_dev, bn_pairing_prepared_many_dev,
 * bn_pairing_batch_prepared_many_dev, bn_g1_msm_dev, bn_g2_msm_dev, bn_g1_bases_prepare_dev,
 * bn_g1_msm_prepared_many_dev, bn_g1_basis_prepare_dev, bn_g1_msm_basis_dev, bn_g1_msm_basis_many_dev,
 * bn_g2_basis_prepare_dev, bn_g2_msm_basis_dev, bn_g1_msm_many_dev and bn_gt_pow_many_dev (bn_pairing_many_allgather_dev is
 * bn_pairing_many_dev on every device's context); bn_dev_status and the host-buffer calls,
 * which run on the context's own stream, take their place in that order too.  A caller may
 * therefore hand one such call's output to the next on another stream without an event of
 * its own.
 * The other *_dev calls use no workspace and are ordered by their own stream ONLY:
 * bn_g1_mul_many_dev and bn_g2_mul_many_dev, the ten group-law calls
 * (bn_g1/g2_{add,sub,neg,normalize,eq}_many_dev) and the three codec calls
 * (bn_g2_affine_new_many_dev, bn_g1/g2_from_compressed_many_dev).  They neither wait for the
 * calls above nor make them wait: a caller who chains one of them with any other call across
 * two streams must order the two itself (an event, or one stream).
 * The reference is reentrant from any thread (lib.rs:303-305, Group: Send + Sync). */
int bn_ctx_create(int device, bn_ctx** out);
int bn_ctx_destroy(bn_ctx* ctx);
const char* bn_last_error(const bn_ctx* ctx);
/* the stream *_dev calls use when given NULL */
void* bn_ctx_stream(bn_ctx* ctx);
/* The sticky device outcome of the *_dev calls without a status word (bn_pairing_many_dev,
 * bn_pairing_many_allgather_dev): synchronizes `stream` (NULL: the context's stream), returns
 * BN_ERR_INTERNAL or BN_ERR_FE_ZERO (a Miller value was zero: the reference panics, mod.rs:900)
 * if any such call since the last bn_dev_status (or host-buffer call, which starts from a clear
 * word) set it, else BN_OK, and clears it.  A call with a status word of its own in between
 * (bn_pairing_batch_dev, bn_miller_loop_batch_dev) reports only itself there and leaves the
 * sticky outcome of the calls before it in place.  bn_pairing_prepared_many_dev adds BN_ERR_INVALID_ARGUMENT
 * (an index past the handle's points), reported after BN_ERR_INTERNAL and before BN_ERR_FE_ZERO.  On a multi-device context it checks every device,
 * each on its own context stream, and `stream` must be NULL (else BN_ERR_INVALID_ARGUMENT). */
int bn_dev_status(bn_ctx* ctx, void* stream);

/* ---- several devices of the node in one process ----
 * A multi-device context shards the host-buffer calls bn_pairing_many,
 * bn_final_exponentiation_many, bn_miller_loop_many, bn_g1_mul_many, bn_g2_mul_many
 * bn_g1_msm and bn_g2_msm contiguously (device k takes bn_shard_range(n, D, k)), runs the
 * shards concurrently and writes each into the caller's output: the same bytes
 * as one device.  bn_pairing_batch / bn_miller_loop_batch reduce each shard to
 * one Miller value, multiply the partials on the first device in device order
 * (pairing_batch then runs one final exponentiation): the reference's shared
 * loop value exactly (mod.rs:609-640).  bn_g1_msm / bn_g2_msm reduce each shard to its
 * Jacobian partial sum, adds the partials on the first device in device order and
 * normalizes there.  bn_pairing_batch_many is sharded by whole products, balanced by
 * terms: device k takes the products from the first whose offset is >= k * n / D up to
 * device k + 1's first, and writes its own rows of out.  Other calls need a single-device
 * context: bn_ctx_device(ctx, k) returns device k's (owned by ctx). */
int bn_ctx_create_multi(const int* devices, int ndev, bn_ctx** out);
int bn_ctx_num_devices(const bn_ctx* ctx);
bn_ctx* bn_ctx_device(bn_ctx* ctx, int k);
/* [*lo, *hi) = shard k of n elements over ndev devices: [k*n/ndev, (k+1)*n/ndev) */
void bn_shard_range(size_t n, int ndev, int k, size_t* lo, size_t* hi);
/* BASELINE config 4 in one process: device k computes out = pairing(d_p[k][i], d_q[k][i])
 * for its n_per_dev HBM-resident pairs, then one RCCL all-gather over xGMI leaves
 * every d_out[k] (ndev * n_per_dev Gt on device k) holding all results in device
 * order.  streams[k] (or NULL / a NULL array: the device context's stream) orders
 * the work on device k.  RCCL (librccl.so.1) is loaded on first use. */
int bn_pairing_many_allgather_dev(bn_ctx* ctx, const bn_g1* const* d_p, const bn_g2* const* d_q, size_t n_per_dev,
                                  bn_gt* const* d_out, void* const* streams);

/* ---- pairing path (src/groups/mod.rs:894-926, src/lib.rs:611-633) ---- */

/* out[i] = pairing(p[i], q[i]) for i < n                     (lib.rs:611-613, mod.rs:894-902)
 * Zero input point -> Gt::one().  BN_ERR_FE_ZERO if a Miller value is 0 (the reference panics). */
int bn_pairing_many(bn_ctx* ctx, const bn_g1* p, const bn_g2* q, size_t n, bn_gt* out);
int bn_pairing_many_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_g2* d_q, size_t n, bn_gt* d_out, void* stream);

/* *out = pairing_batch(&[(p[i], q[i])])                       (lib.rs:615-623, mod.rs:904-926)
 * Pairs with a zero point are skipped; n == 0 or all skipped -> Gt::one(). */
int bn_pairing_batch(bn_ctx* ctx, const bn_g1* p, const bn_g2* q, size_t n, bn_gt* out);

/* out[j] = pairing_batch(&[(p[i], q[i]) for offsets[j] <= i < offsets[j+1]])  for j < m
 * (lib.rs:615-623, mod.rs:904-926 per product): many independent products in one call, the
 * shape of a batch of Groth16 / PLONK verifications or of ecPairing calls.
 * offsets is HOST memory in both forms: m + 1 entries, non-decreasing, offsets[0] == 0, and
 * n = offsets[m] pairs in p and q.  Anything else is refused with BN_ERR_INVALID_ARGUMENT
 * before any buffer is read; so is a NULL out, and a NULL p or q when n > 0.  m == 0 returns
 * BN_OK and touches nothing.
 * Each product follows pairing_batch: a pair with a zero point is skipped, an empty or
 * all-skipped product gives Gt::one(), and every out[j] is bit-identical to bn_pairing_batch
 * on the same slice.  A zero Miller product (no input is known to give one) makes that out[j]
 * the zero image and the call return BN_ERR_FE_ZERO, with every other row written.
 * Three paths, chosen per call from its offsets; results are identical on
 * every one.
 * Wide: a call whose products of at most 64 terms are at least two and hold together at most
 * bn_set_products_wide_max terms sends those products through the one-launch latency kernel
 * (k_pairing_latency: every term's Miller value, 16 lanes per term), then one 16-lane group
 * per product multiplies its terms' values (k_fq12_products_wide), then one final
 * exponentiation per product: the path for calls too small to fill the GPU with lane pairs.
 * Its launch sets hold at most min(bn_set_latency_max, bn_set_products_chunk) terms, and a
 * product above that (when the minimum is below 64) is not eligible.
 * Packed: otherwise, products of at most 64 terms run one per lane pair of one kernel
 * (k_miller_products, the shared-squaring loop per product) in launch sets of at most
 * bn_set_products_chunk terms, followed by one final exponentiation per product.
 * Alone: a product of more than 64 terms, and, off the wide path, every product of a call
 * with fewer than bn_set_products_min of the short ones, runs as bn_pairing_batch_dev does.
 * bn_set_products_min(0) keeps the wide path off as well: every short product is packed.
 * The _dev form enqueues on `stream` without synchronizing and reports the data-dependent
 * outcome through bn_dev_status, as bn_pairing_many_dev does; it reads offsets before it
 * returns, may wait for the previous call's upload of its offsets (not for its kernels),
 * and may allocate (and then waits for earlier work) on first use at a larger size.  It is
 * refused on a multi-device context.
 * Workspace: a launch set needs room for the larger of its terms and its products.
 * bn_reserve(n) guarantees that a call whose launch sets each hold at most n terms and at
 * most n products allocates no workspace (n up to 2^18, the most a launch set takes of
 * either); the 32-bit offsets buffer (m + 1 words per launch set) is separate, grows on
 * first use and is not counted by bn_workspace_bytes. */
int bn_pairing_batch_many(bn_ctx* ctx, const bn_g1* p, const bn_g2* q, const size_t* offsets, size_t m, bn_gt* out);
int bn_pairing_batch_many_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_g2* d_q, const size_t* offsets, size_t m,
                              bn_gt* d_out, void* stream);
/* bn_pairing_batch_many calls with fewer than m products of at most 64 terms run every
 * product alone; 0 sends every such product down the packed path.  Default: the measured
 * crossover or $BN254MI_PRODUCTS_MIN.  On a multi-device context it applies
 * to every device (and to each device's shard). */
int bn_set_products_min(bn_ctx* ctx, size_t m);
/* terms per launch set of the packed path (a single product may exceed it) and of the wide
 * path; 0 = the default, 2^18, and more than that is refused with BN_ERR_INVALID_ARGUMENT */
int bn_set_products_chunk(bn_ctx* ctx, size_t terms);
/* bn_pairing_batch_many and bn_pairing_batch_prepared_many calls of at most this many terms
 * (the plain form: the terms of its products of at most 64 terms) take the wide path; 0 turns
 * it off, any other value is accepted.  bn_set_latency_max(0) turns it off too: the path is
 * built on that kernel.  Default: the measured crossover or
 * $BN254MI_PRODUCTS_WIDE_MAX.  On a multi-device context it applies to every device. */
int bn_set_products_wide_max(bn_ctx* ctx, size_t terms);

/* *out = miller_loop_batch(&[(q[i], p[i])]) -- note the (G2, G1) order (lib.rs:625-633,
 * mod.rs:609-640).  No final exponentiation.  BN_ERR_TO_AFFINE if any point is zero. */
int bn_miller_loop_batch(bn_ctx* ctx, const bn_g2* q, const bn_g1* p, size_t n, bn_gt* out);

/* Device-pointer forms (BASELINE config 5 with HBM-resident inputs): *d_out (one Gt
 * on the device) = pairing_batch / miller_loop_batch of the n pairs, enqueued on
 * `stream` without synchronizing.  The per-pair Miller values are reduced on the
 * device (kernels_wide.hip) and pairing_batch's one final exponentiation runs on
 * a 16-lane group.  Outcomes that depend on the data are written to *d_status
 * (a device int, may be NULL) when the work completes: BN_OK, BN_ERR_TO_AFFINE
 * (miller_loop_batch: a zero point, lib.rs:629-630; *d_out is then unspecified)
 * or BN_ERR_FE_ZERO (pairing_batch: the reference panics; *d_out is zero). */
int bn_pairing_batch_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_g2* d_q, size_t n, bn_gt* d_out, int* d_status,
                         void* stream);
int bn_miller_loop_batch_dev(bn_ctx* ctx, const bn_g2* d_q, const bn_g1* d_p, size_t n, bn_gt* d_out,
                             int* d_status, void* stream);

/* out[i] = Gt::final_exponentiation(f[i]) (lib.rs:598-600, fq12.rs:107-110);
 * ok[i] = 0 where f[i] == 0 (the reference returns None), out[i] then zero. */
int bn_final_exponentiation_many(bn_ctx* ctx, const bn_gt* f, size_t n, bn_gt* out, uint8_t* ok);

/* per-pair Miller values G2Precomp::miller_loop (mod.rs:579-607) after to_affine +
 * precompute; a pair with a zero point gives Fq12::one() */
int bn_miller_loop_many(bn_ctx* ctx, const bn_g1* p, const bn_g2* q, size_t n, bn_gt* out);

/* the line coefficients of AffineG2::precompute (mod.rs:701-727) of q[i] after
 * to_affine: out[(i * 87 + k) * 3 + j] = coefficient k's (ell_0, ell_vw, ell_vv)[j]
 * (G2Precomp / EllCoeffs, mod.rs:566-577).  BN_ERR_TO_AFFINE if a q is zero. */
int bn_g2_precompute_many(bn_ctx* ctx, const bn_g2* q, size_t n, bn_fq2* out);

/* ---- pairings against prepared G2 points (G2Precomp, mod.rs:566-607, 701-727) ----
 * Verifiers pair many G1 points against a few fixed G2 points (a verifying key, an SRS element, a
 * public key).  A bn_g2_prepared handle holds, on the device, the reference's coefficients of
 * q[j].to_affine().precompute() for j < nq -- the 87 (ell_0, ell_vw, ell_vv) that
 * bn_g2_precompute_many exports, 18,792 bytes per point -- so the calls below skip the line steps.
 *   1 <= nq <= 2^16; a NULL q or out, an nq outside that range and a multi-device context are
 *   refused with BN_ERR_INVALID_ARGUMENT before anything is read (a device context from
 *   bn_ctx_device works).  A zero q[j] (z == 0) is legal: pairs against it give what pairing(p, zero)
 *   gives, Gt::one().
 *   The handle belongs to the context that made it: any other context refuses it with
 *   BN_ERR_INVALID_ARGUMENT.  bn_g2_prepared_destroy waits for the work that uses the handle, then
 *   frees it; bn_ctx_destroy frees the handles still alive (they must not be used afterwards).
 *   The table is the handle's own memory: it is separate from the pairing workspace and not counted
 *   by bn_workspace_bytes.  Beside the table the handle keeps the nq points themselves (192 bytes
 *   each; the products' wide path reads points, not lines): 18,985 bytes per point in all with the
 *   zero flag.  Filling it uses the pairing workspace (bn_reserve(nq) pre-sizes that).
 * The _dev form takes device q and enqueues on `stream` without synchronizing (it allocates the
 * table, and may grow the workspace and then wait for earlier work, before it enqueues). */
typedef struct bn_g2_prepared bn_g2_prepared;
int bn_g2_prepare(bn_ctx* ctx, const bn_g2* q, size_t nq, bn_g2_prepared** out);
int bn_g2_prepare_dev(bn_ctx* ctx, const bn_g2* d_q, size_t nq, bn_g2_prepared** out, void* stream);
size_t bn_g2_prepared_count(const bn_g2_prepared* prepared);
int bn_g2_prepared_destroy(bn_ctx* ctx, bn_g2_prepared* prepared);

/* out[i] = pairing(p[i], Q[qidx[i]]) for i < n, Q the handle's points: bit-identical to
 * bn_pairing_many with q[i] = Q[qidx[i]].  qidx == NULL means index 0 for every i.  A zero p[i] or a
 * zero Q[qidx[i]] gives Gt::one(); a zero Miller value the zero image and BN_ERR_FE_ZERO.
 * n == 0 returns BN_OK and touches nothing.  A NULL p, out or handle with n > 0, a handle of another
 * context and a multi-device context are refused with BN_ERR_INVALID_ARGUMENT.
 * Host forms: every qidx[i] < nq is checked before any copy or launch; a bad index is
 * BN_ERR_INVALID_ARGUMENT with out untouched.
 * _dev form: d_qidx is device memory and cannot be checked on the host.  The kernel clamps a bad
 * index (nothing outside the table is read), writes that row as the zero image and sets the sticky
 * outcome that bn_dev_status reports as BN_ERR_INVALID_ARGUMENT (after BN_ERR_INTERNAL, before
 * BN_ERR_FE_ZERO); every other row is correct.
 * Every n takes one throughput kernel (k_pairing_prepared: two lanes per pairing, the lines read
 * from the table as the loop needs them, then the final exponentiation's step machine) in launch
 * sets of 2^18 pairs, on the workspace bn_reserve sizes.  There is no latency path: a small batch
 * costs one throughput launch, the time of a lone lane pair's chain; callers who need small-batch
 * latency keep bn_pairing_many. */
int bn_pairing_prepared_many(bn_ctx* ctx, const bn_g1* p, const bn_g2_prepared* prepared, const uint32_t* qidx,
                             size_t n, bn_gt* out);
int bn_pairing_prepared_many_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_g2_prepared* prepared,
                                 const uint32_t* d_qidx, size_t n, bn_gt* d_out, void* stream);
/* out[i] = G2Precomp::miller_loop (mod.rs:579-607) of Q[qidx[i]] at p[i].to_affine(): bit-identical
 * to bn_miller_loop_many on the same pairs; a zero p[i] or Q[qidx[i]] gives Fq12::one().  Arguments
 * as for bn_pairing_prepared_many. */
int bn_miller_loop_prepared_many(bn_ctx* ctx, const bn_g1* p, const bn_g2_prepared* prepared, const uint32_t* qidx,
                                 size_t n, bn_gt* out);

/* out[j] = pairing_batch over terms offsets[j] <= i < offsets[j+1], for j < m, where the G2 side
 * of term i is the handle's point Q[qidx[i]], or, when qidx[i] == BN_QIDX_FRESH, the next unused
 * entry of q: bn_pairing_batch_many with the fixed G2 points (a Groth16 verifying key's beta,
 * gamma, delta) taken from a bn_g2_prepared handle, so that their line steps are not recomputed
 * and their points are not uploaded.  Every out[j] is bit-identical to bn_pairing_batch over the
 * same terms with the G2 points written out.
 *   p: n = offsets[m] G1 points in term order.  q: only the fresh terms' G2 points, compacted, in
 *   term order (nf entries, nf = the number of BN_QIDX_FRESH in qidx).  qidx (n entries) and
 *   offsets (m + 1 entries, non-decreasing from 0) are HOST memory in both forms.
 *   A term with a zero p[i], a zero fresh q or a zero table point is skipped; an empty or
 *   all-skipped product gives Gt::one().  A zero Miller product makes that out[j] the zero image
 *   and the call return BN_ERR_FE_ZERO with every other row written (the _dev form reports it
 *   through bn_dev_status).
 *   Refused with BN_ERR_INVALID_ARGUMENT before any buffer is read, out untouched: malformed
 *   offsets; a NULL qidx, out or handle; a NULL p with n > 0; a NULL q with nf > 0; an index that
 *   is neither BN_QIDX_FRESH nor below the handle's count; a handle of another context or a
 *   destroyed one; a multi-device context (its device contexts work); any product of more than 64
 *   terms.  m == 0 returns BN_OK and touches nothing.
 * Two paths; bn_set_products_min does not apply and there is no alone path.
 * Wide: a call of at most bn_set_products_wide_max terms, one product included (and
 * min(bn_set_latency_max, bn_set_products_chunk) at least 64, so that every product fits a launch
 * set), gathers each set's G2 points in term order -- the next fresh point, or the handle's own
 * copy of point qidx[i] -- and runs bn_pairing_batch_many's wide path over them: the latency
 * kernel's Miller value per term, a 16-lane group per product, one final exponentiation per
 * product.  It recomputes the fixed points' line steps, on 16 lanes per term, which at these sizes
 * is far below the time of a lone lane pair's chain.  The gathered points (192 bytes per term of a
 * set) grow on first use and are not counted by bn_workspace_bytes.
 * Packed: every larger call runs one product per lane pair of the packed kernel
 * (k_miller_products_mapped) and costs at least the time of one lane pair's chain.  Products of
 * more than 64 terms keep bn_pairing_batch.
 * Per packed launch set (cut at product boundaries, at most bn_set_products_chunk terms and 2^18
 * products): the line producers over the fresh terms only, k_prepared_expand over the prepared
 * ones (the table's lines scaled by the term's Jacobian P; no inversion), the products' loop, one
 * final exponentiation per product.  bn_reserve(n) guarantees that sets of at most n terms and n
 * products allocate no workspace.  Two buffers grow on first use and are not counted by
 * bn_workspace_bytes: the per-term map (up to 3 words per term, uploaded with the offsets) and,
 * in the _dev form, the gathered G1 points of a set's fresh terms (96 bytes each).
 * The _dev form enqueues on `stream` without synchronizing, reads qidx and offsets before it
 * returns, and may wait for the previous call's upload of its offsets (not for its kernels). */
#define BN_QIDX_FRESH 0xffffffffu
int bn_pairing_batch_prepared_many(bn_ctx* ctx, const bn_g1* p, const bn_g2* q, const bn_g2_prepared* prepared,
                                   const uint32_t* qidx, const size_t* offsets, size_t m, bn_gt* out);
int bn_pairing_batch_prepared_many_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_g2* d_q,
                                       const bn_g2_prepared* prepared, const uint32_t* qidx, const size_t* offsets,
                                       size_t m, bn_gt* d_out, void* stream);

/* ---- group path (src/groups/mod.rs:250-334, lib.rs:425-431) ---- */

/* out[i] = p[i] * k[i]: the reference's double-and-add chain (mod.rs:272-292), so the
 * Jacobian output is bit-identical, not merely an equal point -- also where the chain meets
 * res == zero, res == p or res == -p on its way, and for a zero image p (z == 0 under any x, y;
 * see the group law section below). */
int bn_g1_mul_many(bn_ctx* ctx, const bn_g1* p, const bn_fr* k, size_t n, bn_g1* out);
int bn_g1_mul_many_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_fr* d_k, size_t n, bn_g1* d_out, void* stream);
int bn_g2_mul_many(bn_ctx* ctx, const bn_g2* p, const bn_fr* k, size_t n, bn_g2* out);
int bn_g2_mul_many_dev(bn_ctx* ctx, const bn_g2* d_p, const bn_fr* d_k, size_t n, bn_g2* d_out, void* stream);

/* ---- G1 multi-scalar multiplication (bucket method) ---- */

/* *out = (sum over i < n of p[i] * k[i]).normalize()  -- groups/mod.rs:272-334 for the terms and the
 * sum, lib.rs:391-398 for normalize.  The reference has no multi-scalar multiplication, so there is
 * no Jacobian image to reproduce; the normalized image (x, y, one) is the unique one and is what is
 * returned.  A zero sum, and n == 0, give G1::zero() = (0, one, 0) (mod.rs:230-236).  p[i] may be any
 * Jacobian image (z != one, z == 0); k[i] are Fr images as for bn_g1_mul_many.
 * n above 2^26 terms is refused with BN_ERR_INVALID_ARGUMENT (no chunking: entry indices and
 * positions are 32-bit), and so is an n whose n * windows exceeds 2^31 - 1 at a forced narrow window.
 * The _dev form enqueues on `stream` without synchronizing; it may allocate (and then waits for
 * earlier work) on first use at a larger n, as bn_pairing_many_dev does. */
int bn_g1_msm(bn_ctx* ctx, const bn_g1* p, const bn_fr* k, size_t n, bn_g1* out);
int bn_g1_msm_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_fr* d_k, size_t n, bn_g1* d_out, void* stream);
/* window width in bits for the bucket path of both groups, 2 .. 16; 0 (default) = chosen from n by
 * the group's own measured table.  Any other value is refused with BN_ERR_INVALID_ARGUMENT.  Results
 * are identical at every width. */
int bn_set_msm_window(bn_ctx* ctx, int c);
/* batches of either group below n terms take the small path (bn_g1_mul_many's / bn_g2_mul_many's
 * kernels + an addition tree); 0 sends every n >= 1 down the bucket path.  Default: each group's own
 * measured crossover, or $BN254MI_MSM_MIN for both.  Results are identical on either path. */
int bn_set_msm_min(bn_ctx* ctx, size_t n);
/* The run cap L of the bucket path of both groups.  A (window, bucket) key that more than L terms
 * fall into -- many equal scalars, a witness of zeros and ones -- is not summed by one lane as one
 * chain of dependent additions: its run is cut into chunks of at most L entries, one lane each, and
 * the chunk sums are folded by a tree of fan-in 32, so no bucket costs more than
 * L + 32 * ceil(log32(ceil(n / L))) dependent additions.  All of it is enqueued from n, the window
 * and this setting alone: no readback, no synchronization, the _dev forms still only enqueue.
 *   0 (default)         L = max(128, 2 * ceil(n / 2^(c-1))): twice the mean run of uniform scalars at
 *                       window c, so uniform scalars essentially never split
 *   1 .. 65536          exactly this cap
 *   BN_MSM_RUN_UNSPLIT  never split: one lane per key whatever its run (all-equal scalars at 2^18
 *                       terms then take seconds; kept for measurements)
 * Anything else is refused with BN_ERR_INVALID_ARGUMENT.  With the default, skewed batches of 2^18 terms
 * (all scalars equal; half of them 1; 1 % equal to r - 1) take 4 - 9 ms and beat the small path; only a
 * batch whose scalars are ALL 0 or 1 is still faster there (bn_set_msm_min above n), since G * 1 is no
 * chain at all.  No value changes a result: the pieces are
 * the same points added in another order, the group law is exact and the image normalized.  On a
 * multi-device context it applies to every device.
 * Workspace: the partial sums live beside the bucket sums (one point each: 96 bytes for G1, 192 for
 * G2), sized by bn_msm_reserve / bn_g2_msm_reserve for the setting current then, else grown on first
 * use, and not counted by bn_workspace_bytes.  With E = n * windows entries and K = min(buckets *
 * windows, E / (L + 1)) the most keys that can be long, the chunk sums take at most E / L + K points
 * (at most 2 E / L) and the first fold level 1/32 of that plus K; further levels reuse the two.
 * Nothing is allocated when n <= L.  A forced tiny L at a huge n may fail to allocate, and the call
 * then returns BN_ERR_HIP like any other allocation failure. */
#define BN_MSM_RUN_UNSPLIT ((size_t)-1)
int bn_set_msm_run_max(bn_ctx* ctx, size_t entries);
/* pre-size the G1 MSM workspace for up to n terms (else allocated on first use, as bn_reserve);
 * it is separate from the pairing workspace and not counted by bn_workspace_bytes */
int bn_msm_reserve(bn_ctx* ctx, size_t n);

/* ---- G1 MSMs over prepared bases (window tables, no doubling) ----
 * Many small MSMs over the SAME few G1 bases: a Groth16 verifier's vk_x = IC[0] + sum input_i IC[i]
 * per proof, many commitments over one basis, batched fixed-base G1 * Fr (k = 1).  A bn_g1_prepared
 * handle holds, on the device, for every base b and every window w of the signed c-bit recoding
 * (W(c) = 254 / c + 1 windows, as bn_g1_msm), the affine points (j + 1) 2^(c w) bases[b] for
 * j < 2^(c-1): 64 bytes each, and one zero flag per base.  An MSM is then k W(c) table lookups added
 * up, with no doubling.
 *   c: the window width, 2 .. 16; 0 takes the default, 10 (832 KiB per base;
 *   bn_g1_prepared_window reports the width used).  Wider is faster and costs twice the memory
 *   and the prepare time per bit.  k >= 1, and k W(c) 2^(c-1) entries must not exceed 2^31 - 1 (indices are 32-bit).
 *   bn_g1_prepared_table_bytes(k, c) is host arithmetic (no device needed): the device bytes of that
 *   table, 0 for arguments bn_g1_bases_prepare refuses.
 *   Refused with BN_ERR_INVALID_ARGUMENT before anything is read, *out untouched: a NULL bases or
 *   out, a k or c outside those limits, a multi-device context (a device context from bn_ctx_device
 *   works).
 *   bases[b] may be any Jacobian image (z != one; z == 0 with arbitrary x, y: such a base
 *   contributes nothing); points are assumed to be on the curve, as everywhere in the group API.
 *   The handle belongs to the context that made it, exactly as a bn_g2_prepared: any other context
 *   refuses it; bn_g1_prepared_destroy waits for the work that reads it, then frees it;
 *   bn_ctx_destroy frees the handles still alive.  The table is the handle's own memory, not
 *   counted by bn_workspace_bytes.
 * The _dev form takes device bases and enqueues on `stream` without synchronizing (it allocates
 * the table first). */
typedef struct bn_g1_prepared bn_g1_prepared;
size_t bn_g1_prepared_table_bytes(size_t k, int c);
int bn_g1_bases_prepare(bn_ctx* ctx, const bn_g1* bases, size_t k, int c, bn_g1_prepared** out);
int bn_g1_bases_prepare_dev(bn_ctx* ctx, const bn_g1* d_bases, size_t k, int c, bn_g1_prepared** out, void* stream);
size_t bn_g1_prepared_count(const bn_g1_prepared* prepared);
int bn_g1_prepared_window(const bn_g1_prepared* prepared);
int bn_g1_prepared_destroy(bn_ctx* ctx, bn_g1_prepared* prepared);
/* out[j * out_stride] = (sum over b < k of bases[b] * k[j * k + b]).normalize() for j < m: `k` is an
 * m x k row-major matrix of Fr images (k = the handle's count), and every output is the image
 * bn_g1_msm(bases, row j) returns, bit for bit: (x, y, one), and (0, one, 0) for a zero sum.
 *   out_stride counts points and must be >= 1; the points between the strided outputs are not
 *   written (stride 4 writes vk_x straight into the interleaved p array of
 *   bn_pairing_batch_prepared_many_dev for Groth16).
 *   m == 0 returns BN_OK and touches nothing.  Refused with BN_ERR_INVALID_ARGUMENT: a NULL k or out
 *   with m > 0; a NULL handle, one of another context or a destroyed one; out_stride == 0; a
 *   multi-device context; m above 2^26.  No outcome depends on the data: the _dev form has no
 *   status to report.
 * L lanes per output each add their share of the lookups; the partial sums (96 bytes per lane,
 * at most 2^20 lanes at a time: more outputs run in sets) live in the G1 MSM workspace, grown on
 * first use or by bn_msm_reserve(n) for calls of up to n = m L lanes.  The _dev form enqueues on
 * `stream` without synchronizing; it may allocate (and then waits for earlier work) on first use at
 * a larger size. */
int bn_g1_msm_prepared_many(bn_ctx* ctx, const bn_g1_prepared* prepared, const bn_fr* k, size_t m, bn_g1* out,
                            size_t out_stride);
int bn_g1_msm_prepared_many_dev(bn_ctx* ctx, const bn_g1_prepared* prepared, const bn_fr* d_k, size_t m,
                                bn_g1* d_out, size_t out_stride, void* stream);
/* lanes per output of the lookup kernel: a power of two from 1 to 64, or 0 (default) = chosen from
 * m and k.  Anything else is refused with BN_ERR_INVALID_ARGUMENT.  Results are identical for every
 * value. */
int bn_set_msm_prepared_lanes(bn_ctx* ctx, int lanes);

/* ---- many small G1 MSMs over FRESH bases in one call (shared doublings) ----
 * The front half of a batch of PLONK / KZG verifications: one or two MSMs of 2 to about 30 terms
 * per proof over the proof's own commitments, which differ in every proof, so no table can be
 * prepared ahead.  One call computes m of them:
 *   out[j * out_stride] = (sum over offsets[j] <= i < offsets[j+1] of p[i] * k[i]).normalize(), j < m,
 * every output bit for bit the 96 bytes the single MSM returns on the same slice: (x, y, one), and
 * (0, one, 0) for a zero sum or an empty segment.  The group law is exact and the normalized image
 * unique: every setting below, and both paths, give the same bytes.
 *   p[i] may be any Jacobian image (z != one; z == 0 with arbitrary x, y: such a term contributes
 *   nothing), k[i] any Fr image, as for the single MSM.  offsets is HOST memory in both forms:
 *   m + 1 entries, non-decreasing, offsets[0] == 0, n = offsets[m].  out_stride counts points and
 *   must be >= 1; the points between the strided outputs are not written (stride 1 or 2 writes the
 *   sums straight into the p array of bn_pairing_batch_prepared_many_dev).
 *   Refused with BN_ERR_INVALID_ARGUMENT before any buffer is read, out untouched: malformed
 *   offsets; a NULL offsets or out with m > 0; a NULL p or k with n > 0; out_stride == 0; n or m
 *   above 2^26; a multi-device context (a device context from bn_ctx_device works).  m == 0 returns
 *   BN_OK and touches nothing.  No outcome depends on the data: the _dev form has no status to report.
 * Packed path (Straus): per launch set, one lane per term writes the term's signed c-bit digits (one
 * byte each: c <= 8) and its 2^(c-1) Jacobian multiples; one lane per UNIT -- a contiguous run of at
 * most T terms of one segment -- walks the windows from the top, doubling c times per window and adding
 * one signed multiple per term, so the terms of a unit share the 254 doublings; one lane per segment
 * adds its units' partial sums (at most 64) and normalizes.  A segment of more than 64 T terms takes
 * units of ceil(len / 64) terms.  A segment longer than the max setting is not packed: it runs alone
 * on the single MSM's path into its own output, on the same stream.
 * The digits, multiples and partial sums of one launch set live in a workspace of their own, grown on
 * first use or by bn_g1_msm_many_reserve, ordered like the shared one and not counted by
 * bn_workspace_bytes.  The _dev form enqueues on `stream` without synchronizing; it reads offsets
 * before it returns, may wait for the previous call's upload of its plan words (not for its
 * kernels), and may allocate (and then waits for earlier work) on first use at a larger size. */
int bn_g1_msm_many(bn_ctx* ctx, const bn_g1* p, const bn_fr* k, const size_t* offsets, size_t m, bn_g1* out,
                   size_t out_stride);
int bn_g1_msm_many_dev(bn_ctx* ctx, const bn_g1* d_p, const bn_fr* d_k, const size_t* offsets, size_t m,
                       bn_g1* d_out, size_t out_stride, void* stream);
/* the packed path's settings; each refuses a value outside its range with BN_ERR_INVALID_ARGUMENT and
 * none changes a result.  window: c, 2 .. 8, 0 = default (4).  unit: T, 1 .. 64, 0 = chosen per launch
 * set (the smallest that keeps the set at 2^16 lanes, at most 16: T = 1 up to 2^16 terms).  max:
 * segments of more terms run alone; at most 4096, 0 = default (1024, except that a call with 16 or more
 * such segments packs those of up to 4096 terms too: together they fill the card, while a few of them
 * run faster alone).  chunk: the most terms of a launch
 * set (sets are cut at segment boundaries; a single segment may exceed it), at most 2^26; 0 = default
 * (2^20, and at most 1 GiB of digits and multiples, so windows above 4 shrink the set; a set of 2^20
 * terms at c = 4 holds 832 MiB of them, allocated only by calls of that size). */
int bn_set_msm_many_window(bn_ctx* ctx, int c);
int bn_set_msm_many_unit(bn_ctx* ctx, int terms);
int bn_set_msm_many_max(bn_ctx* ctx, size_t terms);
int bn_set_msm_many_chunk(bn_ctx* ctx, size_t terms);
/* pre-size that workspace for calls of up to `terms` terms in up to `segments` segments at the current
 * settings (else grown on first use) */
int bn_g1_msm_many_reserve(bn_ctx* ctx, size_t terms, size_t segments);

/* ---- one large G1 MSM over a FIXED basis (shifted-base table, mixed additions) ----
 * The caller who runs 2^16 - 2^20-term MSMs over the same bases in every call: a KZG / PLONK
 * commitment over an SRS, a Groth16 prover's queries over its proving key.  A bn_g1_basis handle holds,
 * on the device, for every base b and every window w of the signed c-bit recoding (W(c) = 254 / c + 1
 * windows, as the single MSM), the ONE affine point 2^(c w) bases[b]: 64 bytes each, and one zero flag
 * per base -- W(c) points per base (1 KiB at c = 16, 1 GiB for 2^20 bases), where a bn_g1_prepared holds
 * 2^(c-1) W(c).  An MSM is then the bucket method with every digit a lookup of a point that already
 * carries its window's weight: mixed additions into the buckets, the windows' buckets added together,
 * one reduction, and no doubling chain.
 *   c: the window width, 2 .. 16, fixed at prepare time; 0 takes the default from nbases (the basis
 *   form's own measured table; the handle's window call reports the width used).  bn_set_msm_window and
 *   bn_set_msm_min do not apply to these calls; bn_set_msm_run_max does, with the same default rule.
 *   1 <= nbases <= 2^26, and nbases W(c) must not exceed 2^31 - 1.  The table-bytes call is host
 *   arithmetic (no device needed): the device bytes of that table, 0 for arguments the prepare call
 *   refuses.
 *   Refused with BN_ERR_INVALID_ARGUMENT before anything is read, *out untouched: a NULL bases or out,
 *   an nbases or c outside those limits, a multi-device context (a device context from bn_ctx_device
 *   works).
 *   bases[b] may be any Jacobian image (z != one; z == 0 with arbitrary x, y: such a base contributes
 *   nothing); points are assumed to be on the curve, as everywhere in the group API.
 *   The handle belongs to the context that made it, exactly as a bn_g1_prepared: any other context
 *   refuses it; the destroy call waits for the work that reads it, then frees it; bn_ctx_destroy frees
 *   the handles still alive.  The table is the handle's own memory, not counted by bn_workspace_bytes.
 *   Preparing costs about c W(c) doublings and W(c) inversions per base, once: 6.3 ms for 2^18 bases,
 *   20.5 ms for 2^20.
 * The _dev form takes device bases and enqueues on `stream` without synchronizing (it allocates the
 * table first). */
typedef struct bn_g1_basis bn_g1_basis;
size_t bn_g1_basis_table_bytes(size_t nbases, int c);
int bn_g1_basis_prepare(bn_ctx* ctx, const bn_g1* bases, size_t nbases, int c, bn_g1_basis** out);
int bn_g1_basis_prepare_dev(bn_ctx* ctx, const bn_g1* d_bases, size_t nbases, int c, bn_g1_basis** out, void* stream);
size_t bn_g1_basis_count(const bn_g1_basis* basis);
int bn_g1_basis_window(const bn_g1_basis* basis);
int bn_g1_basis_destroy(bn_ctx* ctx, bn_g1_basis* basis);
/* *out = (sum over i < n of bases[i] * k[i]).normalize() over the FIRST n <= nbases bases of the handle
 * (a commitment to a polynomial shorter than the SRS): bit for bit the 96 bytes the single MSM returns
 * on the same bases and scalars, (x, y, one), and (0, one, 0) for a zero sum or n == 0.  The group law
 * is exact and the normalized image unique: no width and no run cap changes a result.
 *   Refused with BN_ERR_INVALID_ARGUMENT: a NULL out; a NULL k with n > 0; n above the handle's count;
 *   a NULL handle, one of another context or a destroyed one; a multi-device context.  No outcome
 *   depends on the data: the _dev form has no status to report.
 * The integer buffers and bucket arrays are the G1 MSM workspace, shared with the single MSM and
 * ordered like it; the reserve call sizes them for n terms at the handle's width and the run cap in
 * force (else grown on first use).  The _dev form enqueues on `stream` without synchronizing; it may
 * allocate (and then waits for earlier work) on first use at a larger size.
 * Which form: with the bases fixed, this one.  Measured against the single MSM on the same terms it is
 * faster at every size from 1 to 2^20 terms (2.5 against 3.9 ms at 2^18, 6.2 against 8.0 at 2^20) and on
 * the skewed scalar patterns, each time by more than the run-to-run spread. */
int bn_g1_msm_basis(bn_ctx* ctx, const bn_g1_basis* basis, const bn_fr* k, size_t n, bn_g1* out);
int bn_g1_msm_basis_dev(bn_ctx* ctx, const bn_g1_basis* basis, const bn_fr* d_k, size_t n, bn_g1* d_out, void* stream);
int bn_g1_msm_basis_reserve(bn_ctx* ctx, const bn_g1_basis* basis, size_t n);

/* ---- a batch of scalar vectors over one FIXED basis in one pass ----
 * out[j * out_stride] = (sum over i < n of bases[i] * k[j * k_stride + i]).normalize() for j < m, over the
 * first n <= nbases bases of the handle: the nine or more polynomials a PLONK prover commits to over one
 * SRS, one polynomial per KZG opening, a Groth16 prover's queries once per proof.  Every output is bit for
 * bit the 96 bytes bn_g1_msm_basis returns for that row: (x, y, one), and (0, one, 0) for a zero sum or
 * n == 0.
 *   k_stride counts scalars and is at least n (rows of a wider coefficient matrix; a shorter polynomial is
 *   a row padded with zero scalars; the scalars of a row past its first n are not read).  out_stride
 *   counts points and is at least 1; the points between outputs are not written.
 *   m == 0 returns BN_OK and touches nothing.  Refused with BN_ERR_INVALID_ARGUMENT before anything is
 *   read, out untouched: a NULL out; a NULL k when m * n > 0; n above the handle's count; k_stride < n;
 *   out_stride == 0; m above 2^26; a NULL handle, one of another context or a destroyed one; a
 *   multi-device context (its device contexts work).  No outcome depends on the data: the _dev form has no
 *   status to report.
 * The m vectors run in launch sets of S vectors, one set after another on the same stream; a set runs
 * every phase of the single call once for all its vectors (one lane per (vector, term), (vector, key), ...),
 * so it costs the launches of ONE single call whatever S is.  S is the largest count with S W(c) 2^(c-1) <=
 * 2^23 (768 MiB of bucket sums) and S n W(c) <= 2^31 - 1, at least 1; bn_set_msm_basis_many_set forces it
 * (1 .. 2^26; 0: that default; still held to the 32-bit positions; a multi-device context sets it on every
 * device).  bn_set_msm_run_max applies per vector with the single call's default rule;
 * bn_set_msm_window and bn_set_msm_min do not apply.
 * The buffers are the G1 MSM workspace, shared with the single MSM, ordered like it and not counted by
 * bn_workspace_bytes; the reserve call sizes them for calls of m vectors of n terms at the handle's width
 * and the settings in force (else grown on first use).  The _dev form only enqueues on `stream`; it may
 * allocate (and then waits for earlier work) on first use at a larger size.
 * Which form: with two or more vectors over one handle, this one.  Measured against a loop of m
 * bn_g1_msm_basis_dev calls on the same handle and scalars (m in {2, 8, 32, 128} x n in {2^10 .. 2^18}, and 9 x
 * 2^16) it is faster at every shape by more than the run-to-run spread: 2 vectors cost one call's time up to 2^12
 * terms; 9 x 2^16 takes 4.0 against 12.3 ms, 128 x 2^10 2.1 against 100, 128 x 2^14 14.4 against 130; the gain is
 * smallest at large n with small m (2 x 2^18: 3.6 against 5.0 ms).  No measured shape is slower. */
int bn_g1_msm_basis_many(bn_ctx* ctx, const bn_g1_basis* basis, const bn_fr* k, size_t k_stride, size_t m, size_t n,
                         bn_g1* out, size_t out_stride);
int bn_g1_msm_basis_many_dev(bn_ctx* ctx, const bn_g1_basis* basis, const bn_fr* d_k, size_t k_stride, size_t m, size_t n,
                             bn_g1* d_out, size_t out_stride, void* stream);
int bn_g1_msm_basis_many_reserve(bn_ctx* ctx, const bn_g1_basis* basis, size_t m, size_t n);
int bn_set_msm_basis_many_set(bn_ctx* ctx, size_t vectors); /* vectors per launch set; 0 = default */

/* ---- G2 multi-scalar multiplication (bucket method on the two-lane layout) ---- */

/* The same contract over G2: *out = (sum over i < n of p[i] * k[i]).normalize(), the image (x, y, one)
 * with one the Fq2 one; a zero sum, and n == 0, give G2::zero() = (0, one, 0).  p[i] may be any
 * Jacobian image (z != one, and z == 0 with arbitrary x, y).  The same limits on n, refused before
 * any buffer is read; NULL pointers are refused; the _dev form is refused on a multi-device context.
 * A multi-device context shards bn_g2_msm as bn_g1_msm (bn_shard_range, Jacobian partials added on
 * the first device in device order, normalized there): the single-device bytes. */
int bn_g2_msm(bn_ctx* ctx, const bn_g2* p, const bn_fr* k, size_t n, bn_g2* out);
int bn_g2_msm_dev(bn_ctx* ctx, const bn_g2* d_p, const bn_fr* d_k, size_t n, bn_g2* d_out, void* stream);
/* pre-size the G2 MSM workspace for up to n terms.  The integer buffers (keys, sorted entries) are
 * shared with G1; the bucket sums, partial sums and small-path products are G2's own (a bn_g2 is
 * 192 bytes: 96 MiB of bucket sums at c = 16).  Not counted by bn_workspace_bytes. */
int bn_g2_msm_reserve(bn_ctx* ctx, size_t n);

/* ---- one large G2 MSM over a FIXED basis (shifted-base table, mixed additions) ----
 * The caller who runs 2^16 - 2^20-term MSMs over the same G2 bases in every call: a Groth16 prover's B
 * query over its proving key, the G2 powers of tau of a KZG or aggregation scheme.  A bn_g2_basis handle
 * holds, on the device, for every base b and every window w of the signed c-bit recoding (W(c) = 254 / c + 1
 * windows, as the single MSM), the ONE affine point 2^(c w) bases[b]: 128 bytes each, and one zero flag
 * per base -- W(c) points per base (2 KiB at c = 16, 2 GiB for 2^20 bases).  An MSM is then the bucket
 * method with every digit a lookup of a point that already carries its window's weight: mixed additions
 * into the buckets, the windows' buckets added together, one reduction, and no doubling chain.
 *   c: the window width, 2 .. 16, fixed at prepare time; 0 takes the default from nbases (the G2 basis
 *   form's own table; the handle's window call reports the width used).  bn_set_msm_window and
 *   bn_set_msm_min do not apply to these calls; bn_set_msm_run_max does, with the same default rule.
 *   1 <= nbases <= 2^26, and nbases W(c) must not exceed 2^31 - 1.  The table-bytes call is host
 *   arithmetic (no device needed): the device bytes of that table, nbases (128 W(c) + 1), and 0 for
 *   arguments the prepare call refuses.
 *   Refused with BN_ERR_INVALID_ARGUMENT before anything is read, *out untouched: a NULL bases or out,
 *   an nbases or c outside those limits, a multi-device context (a device context from bn_ctx_device
 *   works).
 *   bases[b] may be any Jacobian image (z != one; z == 0 with arbitrary x, y: such a base contributes
 *   nothing); points are assumed to be on the twist, as everywhere in the group API, and need not lie
 *   in the order-r subgroup (the twist's group order is odd: no doubling of the build reaches zero).
 *   The handle belongs to the context that made it, exactly as a bn_g1_basis: any other context
 *   refuses it; the destroy call waits for the work that reads it, then frees it; bn_ctx_destroy frees
 *   the handles still alive.  The table is the handle's own memory, not counted by bn_workspace_bytes.
 *   Preparing costs about c W(c) doublings and W(c) inversions per base, once: 14.1 ms for 2^18 bases,
 *   51.4 ms for 2^20.
 * The _dev form takes device bases and enqueues on `stream` without synchronizing (it allocates the
 * table first). */
typedef struct bn_g2_basis bn_g2_basis;
size_t bn_g2_basis_table_bytes(size_t nbases, int c);
int bn_g2_basis_prepare(bn_ctx* ctx, const bn_g2* bases, size_t nbases, int c, bn_g2_basis** out);
int bn_g2_basis_prepare_dev(bn_ctx* ctx, const bn_g2* d_bases, size_t nbases, int c, bn_g2_basis** out, void* stream);
size_t bn_g2_basis_count(const bn_g2_basis* basis);
int bn_g2_basis_window(const bn_g2_basis* basis);
int bn_g2_basis_destroy(bn_ctx* ctx, bn_g2_basis* basis);
/* *out = (sum over i < n of bases[i] * k[i]).normalize() over the FIRST n <= nbases bases of the handle:
 * bit for bit the 192 bytes bn_g2_msm returns on the same bases and scalars, (x, y, one) with one the
 * Fq2 one, and (0, one, 0) for a zero sum or n == 0.  The group law is exact and the normalized image
 * unique: no width and no run cap changes a result.
 *   Refused with BN_ERR_INVALID_ARGUMENT: a NULL out; a NULL k with n > 0; n above the handle's count;
 *   a NULL handle, one of another context or a destroyed one; a multi-device context.  No outcome
 *   depends on the data: the _dev form has no status to report.
 * The integer buffers and bucket arrays are the G2 MSM workspace, shared with bn_g2_msm and ordered
 * like it; the reserve call sizes them for n terms at the handle's width and the run cap in force
 * (else grown on first use).  The _dev form enqueues on `stream` without synchronizing; it may
 * allocate (and then waits for earlier work) on first use at a larger size.
 * Which form: with the bases fixed, this one.  Measured against bn_g2_msm on the same terms it is faster at
 * every size from 1 to 2^20 terms (2.3 against 3.9 ms at 2^16, 4.2 against 6.2 at 2^18, 10.2 against 13.8 at
 * 2^20) and on the skewed scalar patterns, each time by more than the run-to-run spread. */
int bn_g2_msm_basis(bn_ctx* ctx, const bn_g2_basis* basis, const bn_fr* k, size_t n, bn_g2* out);
int bn_g2_msm_basis_dev(bn_ctx* ctx, const bn_g2_basis* basis, const bn_fr* d_k, size_t n, bn_g2* d_out, void* stream);
int bn_g2_msm_basis_reserve(bn_ctx* ctx, const bn_g2_basis* basis, size_t n);

/* ---- group law (lib.rs:388-423, 539-574; src/groups/mod.rs:169-216, 294-358) ----
 * Batched forms of the G1 / G2 operators, each lane running the reference's own
 * Jacobian formulas, so the output images are bit-identical (not merely equal points):
 *   add        out = a + b      (mod.rs:294-334: both zero shortcuts, the doubling when a == b)
 *   sub        out = a - b      (mod.rs:352-358: a + (-b))
 *   neg        out = -a         (mod.rs:336-350: zero unchanged, else (x, -y, z))
 *   normalize  out = a.normalize() (lib.rs:391-398: to_affine then to_jacobian, z = one,
 *              mod.rs:199-226; zero unchanged)
 *   eq         eq[i] = (a == b) (PartialEq, mod.rs:169-195: projective equality) as 0 / 1
 * A zero point is any image with z == 0, whatever its x, y (mod.rs:246-248; G::new takes any x, y, z):
 * every entry point of this header accepts such an image, and every returned image is the
 * reference's.  zero + b is b's own image, a + zero is a's, and zero + zero the second operand's;
 * neg and normalize leave a zero image as it is; eq looks only at z when either side is zero.
 * double() has no zero check, so a zero image keeps its z == 0 while its x, y go on through the
 * doubling formulas: p * k for a zero image p is p doubled once per trailing zero bit of k (and
 * (0, one, 0) for k == 0).  The pairing entry points skip a pair with a zero image on either side,
 * or return BN_ERR_TO_AFFINE where the reference fails (bn_miller_loop_batch,
 * bn_g2_precompute_many); a prepared zero q[j] sets that point's zero flag.  The chains take the
 * doubling branch and the h == 0 branch (z3 == 0) wherever the data leads them, also mid-chain:
 * on-curve G2 images outside the order-r subgroup (small-order twist points) are multiplied and
 * summed exactly as the reference does. */
int bn_g1_add_many(bn_ctx* ctx, const bn_g1* a, const bn_g1* b, size_t n, bn_g1* out);
int bn_g1_sub_many(bn_ctx* ctx, const bn_g1* a, const bn_g1* b, size_t n, bn_g1* out);
int bn_g1_neg_many(bn_ctx* ctx, const bn_g1* a, size_t n, bn_g1* out);
int bn_g1_normalize_many(bn_ctx* ctx, const bn_g1* a, size_t n, bn_g1* out);
int bn_g1_eq_many(bn_ctx* ctx, const bn_g1* a, const bn_g1* b, size_t n, uint8_t* eq);
int bn_g2_add_many(bn_ctx* ctx, const bn_g2* a, const bn_g2* b, size_t n, bn_g2* out);
int bn_g2_sub_many(bn_ctx* ctx, const bn_g2* a, const bn_g2* b, size_t n, bn_g2* out);
int bn_g2_neg_many(bn_ctx* ctx, const bn_g2* a, size_t n, bn_g2* out);
int bn_g2_normalize_many(bn_ctx* ctx, const bn_g2* a, size_t n, bn_g2* out);
int bn_g2_eq_many(bn_ctx* ctx, const bn_g2* a, const bn_g2* b, size_t n, uint8_t* eq);
int bn_g1_add_many_dev(bn_ctx* ctx, const bn_g1* d_a, const bn_g1* d_b, size_t n, bn_g1* d_out, void* stream);
int bn_g1_sub_many_dev(bn_ctx* ctx, const bn_g1* d_a, const bn_g1* d_b, size_t n, bn_g1* d_out, void* stream);
int bn_g1_neg_many_dev(bn_ctx* ctx, const bn_g1* d_a, size_t n, bn_g1* d_out, void* stream);
int bn_g1_normalize_many_dev(bn_ctx* ctx, const bn_g1* d_a, size_t n, bn_g1* d_out, void* stream);
int bn_g1_eq_many_dev(bn_ctx* ctx, const bn_g1* d_a, const bn_g1* d_b, size_t n, uint8_t* d_eq, void* stream);
int bn_g2_add_many_dev(bn_ctx* ctx, const bn_g2* d_a, const bn_g2* d_b, size_t n, bn_g2* d_out, void* stream);
int bn_g2_sub_many_dev(bn_ctx* ctx, const bn_g2* d_a, const bn_g2* d_b, size_t n, bn_g2* d_out, void* stream);
int bn_g2_neg_many_dev(bn_ctx* ctx, const bn_g2* d_a, size_t n, bn_g2* d_out, void* stream);
int bn_g2_normalize_many_dev(bn_ctx* ctx, const bn_g2* d_a, size_t n, bn_g2* d_out, void* stream);
int bn_g2_eq_many_dev(bn_ctx* ctx, const bn_g2* d_a, const bn_g2* d_b, size_t n, uint8_t* d_eq, void* stream);

/* ---- Gt / Fq12 element operations (src/fields/fq12.rs) for batched callers and tests ---- */
typedef enum {
    BN_FQ12_MUL = 0,          /* a * b          fq12.rs:319-327 (Gt * Gt, lib.rs:603-609) */
    BN_FQ12_SQR = 1,          /* a^2            fq12.rs:295-303 */
    BN_FQ12_INV = 2,          /* a^-1 (0 -> 0)  fq12.rs:305-313 */
    BN_FQ12_CYC_SQR = 3,      /* cyclotomic_squared fq12.rs:198-247 */
    BN_FQ12_EXP_BY_NEG_Z = 4, /* fq12.rs:121-124 */
    BN_FQ12_FROB1 = 5, BN_FQ12_FROB2 = 6, BN_FQ12_FROB3 = 7 /* fq12.rs:112-119 */
} bn_fq12_op;
int bn_fq12_op_many(bn_ctx* ctx, int op, const bn_gt* a, const bn_gt* b, size_t n, bn_gt* out);

/* ---- encodings, validation, square roots, decompression, Gt::pow ----
 * Batched forms of the reference's per-element API.  Each element gets a status
 * (bn_elem_status) where the reference returns a Result/Option; an element that
 * fails has an all-zero output image.  Byte records are the reference's slices:
 * 32-byte big-endian Fq/Fr, 64-byte big-endian Fq2 (a U512 = c1 * p + c0),
 * 33-byte compressed G1, 65-byte compressed G2, packed back to back.  The host
 * forms copy through the context; the _dev forms take device pointers and
 * enqueue on `stream` (NULL: the context's stream) without synchronizing. */
typedef enum {
    BN_ST_OK = 0,
    BN_ST_FIELD_INVALID_SLICE_LENGTH = 1, /* FieldError::InvalidSliceLength (lib.rs:99-104) */
    BN_ST_FIELD_INVALID_U512 = 2,         /* FieldError::InvalidU512Encoding */
    BN_ST_FIELD_NOT_MEMBER = 3,           /* FieldError::NotMember */
    BN_ST_CURVE_INVALID_ENCODING = 4,     /* CurveError::InvalidEncoding (lib.rs:106-112) */
    BN_ST_CURVE_NOT_MEMBER = 5,           /* CurveError::NotMember */
    BN_ST_GROUP_NOT_ON_CURVE = 6,         /* groups::Error::NotOnCurve (mod.rs:89-92) */
    BN_ST_GROUP_NOT_IN_SUBGROUP = 7       /* groups::Error::NotInSubgroup */
} bn_elem_status;

/* Fq::from_slice (lib.rs:154-159): NotMember unless the value is below p */
int bn_fq_from_slice_many(bn_ctx* ctx, const uint8_t* be32, size_t n, bn_fq* out, uint8_t* status);
/* Fq::to_big_endian (lib.rs:160-170): the canonical integer */
int bn_fq_to_big_endian_many(bn_ctx* ctx, const bn_fq* a, size_t n, uint8_t* be32);
/* Fq2::from_slice (lib.rs:260-267): c0 = v mod p, c1 = v div p; NotMember when v >= p^2 */
int bn_fq2_from_slice_many(bn_ctx* ctx, const uint8_t* be64, size_t n, bn_fq2* out, uint8_t* status);
/* Fr::from_slice (lib.rs:45-49): new_mul_factor, reduces any 256-bit value mod r */
int bn_fr_from_slice_many(bn_ctx* ctx, const uint8_t* be32, size_t n, bn_fr* out);
/* Fr::to_big_endian (lib.rs:50-55): writes the RAW Montgomery image, as the reference does */
int bn_fr_to_big_endian_many(bn_ctx* ctx, const bn_fr* a, size_t n, uint8_t* be32);
/* Fq::sqrt / Fq2::sqrt (fp.rs:245-260, fq2.rs:208-224): ok[i] = 0 where the reference returns None */
int bn_fq_sqrt_many(bn_ctx* ctx, const bn_fq* a, size_t n, bn_fq* out, uint8_t* ok);
int bn_fq2_sqrt_many(bn_ctx* ctx, const bn_fq2* a, size_t n, bn_fq2* out, uint8_t* ok);
/* AffineG1::new / AffineG2::new (lib.rs:413-415, 549-551; mod.rs:95-113) then into G1/G2
 * (to_jacobian, mod.rs:220-226).  G2 includes the order check [r]P == 0. */
int bn_g1_affine_new_many(bn_ctx* ctx, const bn_fq* x, const bn_fq* y, size_t n, bn_g1* out, uint8_t* status);
int bn_g2_affine_new_many(bn_ctx* ctx, const bn_fq2* x, const bn_fq2* y, size_t n, bn_g2* out, uint8_t* status);
int bn_g2_affine_new_many_dev(bn_ctx* ctx, const bn_fq2* d_x, const bn_fq2* d_y, size_t n, bn_g2* d_out,
                              uint8_t* d_status, void* stream);
/* G1::from_compressed (lib.rs:359-375, 33-byte records) and G2::from_compressed
 * (lib.rs:506-526, 65-byte records, includes the G2 order check) */
int bn_g1_from_compressed_many(bn_ctx* ctx, const uint8_t* b33, size_t n, bn_g1* out, uint8_t* status);
int bn_g2_from_compressed_many(bn_ctx* ctx, const uint8_t* b65, size_t n, bn_g2* out, uint8_t* status);
int bn_g1_from_compressed_many_dev(bn_ctx* ctx, const uint8_t* d_b33, size_t n, bn_g1* d_out, uint8_t* d_status,
                                   void* stream);
int bn_g2_from_compressed_many_dev(bn_ctx* ctx, const uint8_t* d_b65, size_t n, bn_g2* d_out, uint8_t* d_status,
                                   void* stream);
/* out[i] = Gt::pow(a[i], k[i]) (lib.rs:592-594; generic Fq12 pow, fields/mod.rs:35-46) */
int bn_gt_pow_many(bn_ctx* ctx, const bn_gt* a, const bn_fr* k, size_t n, bn_gt* out);
int bn_gt_pow_many_dev(bn_ctx* ctx, const bn_gt* d_a, const bn_fr* d_k, size_t n, bn_gt* d_out, void* stream);

/* ---- measurement ---- */
/* enable HIP-event timing of each kernel phase of bn_pairing_many_dev (events are
 * recorded on the launch stream between the kernels) */
int bn_set_phase_timing(bn_ctx* ctx, int enable);
/* Batches of at most n elements take the latency path: bn_pairing_many_dev runs
 * k_pairing_latency (up to bn_set_latency_max pairs) or the segmented Miller loop with
 * the recombination + final exponentiation on 16-lane groups, bn_final_exponentiation_many
 * the 16-lane final exponentiation (kernels_wide.hip); larger batches take the throughput
 * path (k_pairing_full: to_affine, lines, Miller loop and the two-lane final-exponentiation
 * step machine in one launch).  Default 8192 (the measured crossover) or
 * $BN254MI_FE_WIDE_MAX; results are identical either way.  On a multi-device
 * context it applies to every device. */
int bn_set_fe_wide_max(bn_ctx* ctx, size_t n);
/* Which build of the two-lane step machine bn_fq12_op_many runs: 0 (default) the final
 * exponentiation unit's (k_fq12_vm), 1 the one inside the throughput kernel's unit
 * (k_fq12_vm_pairing: the Fq12 operations exactly as k_pairing_full runs them).  The two
 * are built with different forms of the Fq12 product, square and cyclotomic square;
 * results are identical.  Meant for checking single operations of the throughput
 * kernel on chosen operands.  On a multi-device context it applies to every device. */
int bn_set_fq12_op_unit(bn_ctx* ctx, int unit);
/* Within the latency path, bn_pairing_many_dev batches of at most n pairs run the
 * whole pairing in ONE launch (k_pairing_latency: a wave computing the 87 lines of
 * each pair feeds, through an LDS ring, 16-lane groups running the Miller loop and
 * the final exponentiation; above 2,048 pairs its two-wave build, two blocks per CU);
 * larger ones the segmented three-kernel form.  pairing_batch / miller_loop_batch take
 * the same kernel for their Miller values up to n pairs.
 * Default 4096 or $BN254MI_LATENCY_MAX; 0 disables it; results are identical. */
int bn_set_latency_max(bn_ctx* ctx, size_t n);
/* device milliseconds per phase of bn_pairing_many_dev since the last read, per chunk
 * launch set: the default throughput form is one kernel (k_pairing_full) and the
 * latency form one kernel (k_pairing_latency), both timed whole in ms[0] (ms[1..3] = 0);
 * the three-launch forms ($BN254MI_MILLER_FORM 0-2) split it as ms[0] k_prepare or
 * k_pairing_fused, ms[1] k_miller / k_miller_seg, ms[2] k_fq12_vm, ms[3] k_fe_out;
 * the segmented latency path ms[0] k_prepare_wide, ms[1] k_miller_seg, ms[2] k_horner_wide.
 * *launches = launch sets measured */
int bn_get_phase_times(bn_ctx* ctx, float ms[4], int* launches);
/* the products that bn_pairing_batch_many and bn_pairing_batch_prepared_many (both forms of
 * each) planned on each path since the last read: counts[0] wide, counts[1] packed, counts[2]
 * alone; the read clears them.  Counted on the host when a call plans its work, so a call
 * refused before that counts nothing.  On a multi-device context: the sum over its devices. */
int bn_get_products_routes(bn_ctx* ctx, size_t counts[3]);

/* ---- workspace ---- */
/* device bytes the context holds for a batch of n pairings (allocated on first use) */
size_t bn_workspace_bytes(size_t n);
/* pre-size the context workspace for batches up to n (avoids allocation inside timed loops) */
int bn_reserve(bn_ctx* ctx, size_t n);

#ifdef __cplusplus
}
#endif
#endif
