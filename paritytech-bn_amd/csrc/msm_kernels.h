// msm_kernels.h -- the kernel layer of the multi-scalar multiplications, once for G1 and
// G2: the bounds checks, the clamping of a run to nent, the msm_run_task guards and the
// point and table accesses around the arithmetic of msm_group.h and msm_basis.h.  One body
// per phase, a template over the field F (Fq: G1; Fq2: G2) and the point type P; the
// __global__ kernels of kernels_msm.hip, kernels_msm_g2.hip, kernels_msm_basis.hip and
// kernels_msm_basis_g2.hip are fold_table_init() and one call of their body with the
// element index, and kernels_msm_basis_many.hip shares the run's clamp and basis_run_sum.
// (F is a parameter of its own and no member of MsmIo<P>: Jac of an alias template is
// another type than Jac<Fq>.  fold_table_init() and the lane index stay in the kernel: moved
// in here they change the kernel's prologue.)
//
// The element index: G1 has one lane per element, lane_id(); G2 runs on the pairing path's
// two-lane layout (fq2_split.h; BN_SPLIT, set by the G2 units): lanes 2j and 2j + 1 hold
// coordinates c0 and c1 of the points of element j = lane_id() / kPathLanes.
//
// Pair-uniform control (G2): every Fq2 product and zero test reads the partner lane over
// DPP, so both lanes of a pair must take every branch and leave every loop together.  Every
// bound here (the element against its count, the run clamped to nent, the slot's task, an
// entry's index against n, msm_basis_run_sum's pending and take) is computed from the
// element index and from loads both lanes make at the same address; jac_add's and
// jac_add_mixed's guards come from fq2_is_zero, which is pair-uniform; only the address of
// a lane's own coordinates (ld_ref2, MsmIo<bn_g2>::entry) differs between the two lanes.
// The block size is even, so a grid covers whole pairs.  Pairs of one wave walk runs of
// different lengths: the wave-uniform guards of jac_add (BN_ANY) see the active lanes only.
//
// Every computed index is bounded against its array in the body; an element whose index is
// out of range does nothing, and no block waits for another.
#pragma once
#include "kernels.h"
#include "msm_basis.h"

namespace bn {

// ---------------------------------------------------------------- group I/O
// kLanes: lanes per element; ld / st: this lane's coordinates of a point's reference image;
// Elem: the table's element type, an entry of a fixed basis (msm_basis.h) being two of them
// per lane; entry: this lane's address of table entry `index`.
template <class P>
struct MsmIo;
template <>
struct MsmIo<bn_g1> {
    static constexpr size_t kLanes = 1;
    using Elem = bn_fq;  // an entry: x, y
    static __device__ __forceinline__ G1J ld(const bn_g1& a) { return ld_g1(a); }
    static __device__ __forceinline__ void st(bn_g1& o, const G1J& r) { st_g1(o, r); }
    template <class T>
    static __device__ __forceinline__ T* entry(T* table, size_t index) {
        return table + 2 * index;
    }
};
// the images of x and y in the lane's address of an entry
struct BasisSlot {
    bn_fq &x, &y;
};
__device__ __forceinline__ BasisSlot basis_slot(bn_fq* e) { return {e[0], e[1]}; }
// this lane's Fq of a field element
template <int B>
__device__ __forceinline__ const Fq<B>& lane_fq(const Fq<B>& x) { return x; }
#if BN_SPLIT
template <>
struct MsmIo<bn_g2> {
    static constexpr size_t kLanes = kPathLanes;
    // an entry is two lane halves [x.c0, y.c0 | x.c1, y.c1]: element 2 * index + h is lane h's
    // half, its c0 the lane's coordinate of x and its c1 that of y, so each lane of a pair
    // gathers its own coordinates with one aligned 64-byte read
    using Elem = bn_fq2;
    static __device__ __forceinline__ G2J ld(const bn_g2& a) { return ld_g2(a); }
    static __device__ __forceinline__ void st(bn_g2& o, const G2J& r) { st_g2(o, r); }
    template <class T>
    static __device__ __forceinline__ T* entry(T* table, size_t index) {
        return table + 2 * index + (lane_odd() ? 1 : 0);
    }
};
__device__ __forceinline__ BasisSlot basis_slot(bn_fq2* e) { return {e->c0, e->c1}; }
template <int B>
__device__ __forceinline__ const Fq<B>& lane_fq(const Fq2<B>& x) { return x.c; }
#endif

// the run of `key` < nkeys in the sorted entries, clamped to nent: offsets[key] ..
// offsets[key + 1] (Key: the caller's index type, so its address arithmetic is as it was)
struct MsmRun {
    uint32_t lo, hi;
};
template <class Key>
__device__ __forceinline__ MsmRun msm_key_run(const uint32_t* offsets, Key key, uint32_t nent) {
    uint32_t hi = offsets[key + 1];
    hi = hi < nent ? hi : nent;
    uint32_t lo = offsets[key];
    lo = lo < hi ? lo : hi;
    return {lo, hi};
}

// ---------------------------------------------------------------- bucket form
// Element `key` of the (window, bucket) keys: the sum of its run of sorted entries
// (msm_group.h msm_bucket_sum).  An empty bucket is zero.  A run of more than L entries is
// left to the chunk and fold kernels, which write its bucket.
template <template <int> class F, class P>
__device__ __forceinline__ void msm_accumulate_body(size_t key, const P* p, size_t n, const uint32_t* sorted,
                                                    const uint32_t* offsets, uint32_t nkeys, uint32_t nent, uint32_t L,
                                                    P* buckets) {
    using IO = MsmIo<P>;
    if (key >= nkeys) return;
    const MsmRun run = msm_key_run(offsets, key, nent);
    if (run.hi - run.lo > L) return;
    const Jac<F> acc = msm_bucket_sum<F>([&](uint32_t idx) { return IO::ld(p[idx]); }, n, sorted, run.lo, run.hi);
    IO::st(buckets[key], acc);
}
// The overlong runs (msm.h).  Element t of the level-0 slots: the sum of one chunk of at most
// L entries of a long key's run (msm_run_task finds the key and the chunk from the slot).  A
// slot no key holds does nothing; with no long key every element returns after one load.
template <template <int> class F, class P>
__device__ __forceinline__ void msm_chunk_body(size_t t, const P* p, size_t n, const uint32_t* sorted,
                                               const uint32_t* offsets, const uint32_t* longinfo, uint32_t nkeys,
                                               uint32_t nent, uint32_t L, P* sums, uint32_t nslots) {
    using IO = MsmIo<P>;
    if (t >= nslots) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, 0, (uint32_t)t);
    if (!task.some) return;
    const Jac<F> acc = msm_bucket_sum<F>([&](uint32_t idx) { return IO::ld(p[idx]); }, n, sorted, task.lo, task.hi);
    IO::st(sums[t], acc);
}
// Element t of the slots of fold level `level` >= 1: the sum of up to kMsmFoldFan consecutive
// partial sums of one long key at the level below (src[0 .. nsrc)), into the key's bucket
// when it is the key's only group, else into dst[slot] (dst[0 .. ndst)).
template <template <int> class F, class P>
__device__ __forceinline__ void msm_fold_body(size_t t, const P* src, uint32_t nsrc, const uint32_t* offsets,
                                              const uint32_t* longinfo, uint32_t nkeys, uint32_t nent, uint32_t L,
                                              int level, P* dst, uint32_t ndst, uint32_t nslots, P* buckets) {
    using IO = MsmIo<P>;
    if (t >= nslots) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, level, (uint32_t)t);
    if (!task.some || task.hi > nsrc || (!task.last && t >= ndst)) return;
    const Jac<F> acc = msm_fold_sum<F>([&](uint32_t i) { return IO::ld(src[i]); }, task.lo, task.hi);
    IO::st(task.last ? buckets[task.key] : dst[t], acc);
}
// Element t = s * nwin + w of the (segment, window) pairs: the segment's weighted sum
// (msm_group.h msm_segment_sum) into parts[t], so that the addition tree over the segments
// is the group's k_*_op on contiguous halves.
template <template <int> class F, class P>
__device__ __forceinline__ void msm_reduce_body(size_t t, const P* buckets, int c, uint32_t nkeys, uint32_t nseg,
                                                P* parts) {
    using IO = MsmIo<P>;
    const uint32_t nwin = (uint32_t)msm_windows(c);
    if (t >= (size_t)nseg * nwin) return;
    const uint32_t s = (uint32_t)(t / nwin), w = (uint32_t)(t % nwin);
    IO::st(parts[t], msm_segment_sum<F>([&](uint32_t key) { return IO::ld(buckets[key]); }, c, nkeys, s, w));
}
// Element 0 alone: Horner over the window sums win[0 .. nwin) (msm_group.h msm_horner_sum).
// finish != 0: the normalized image (msm_finish_point); 0: the Jacobian partial sum as it
// stands (a multi-device context adds the partials first).
template <template <int> class F, class P>
__device__ __forceinline__ void msm_horner_body(size_t t, const P* win, int c, int finish, P* out) {
    using IO = MsmIo<P>;
    if (t != 0) return;
    Jac<F> acc = msm_horner_sum<F>([&](int w) { return IO::ld(win[w]); }, c);
    if (finish) acc = msm_finish_point(acc);
    IO::st(*out, acc);
}
// Element 0 alone: *out = the returned image of *in (msm_finish_point); in == nullptr: of
// zero (n == 0)
template <template <int> class F, class P>
__device__ __forceinline__ void msm_finish_body(size_t t, const P* in, P* out) {
    using IO = MsmIo<P>;
    if (t != 0) return;
    Jac<F> a = jac_zero<F>();
    if (in) a = IO::ld(*in);
    IO::st(*out, msm_finish_point(a));
}

// ---------------------------------------------------------------- fixed-basis form (msm_basis.h)
// Element b of the bases: entries (b, 0 .. W(c)) as reference images (x, y) and the base's
// zero flag (pair-uniform: jac_is_zero; both lanes of a pair store the same byte).  A zero
// base's entries are written as zeros: the accumulation's idle fetches read base 0's entry,
// so every entry holds field elements.
template <template <int> class F, class P>
__device__ __forceinline__ void msm_basis_build_body(size_t t, const P* bases, uint32_t nbases, int c,
                                                     typename MsmIo<P>::Elem* table, uint8_t* zero) {
    using IO = MsmIo<P>;
    if (t >= nbases) return;
    const uint32_t b = (uint32_t)t;
    const Jac<F> base = IO::ld(bases[b]);
    const bool bzero = jac_is_zero(base);
    zero[b] = bzero ? 1 : 0;
    if (bzero) {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t w = 0; w < (uint32_t)msm_windows(c); ++w) {
            const BasisSlot e = basis_slot(IO::entry(table, (size_t)msm_basis_index(nbases, b, w)));
            st_words(&e.x, z);
            st_words(&e.y, z);
        }
        return;
    }
    msm_basis_build<F>(base, c, [&](uint32_t w, const F<kPt>& x, const F<kPt>& y) {
        const BasisSlot e = basis_slot(IO::entry(table, (size_t)msm_basis_index(nbases, b, w)));
        st_ref(e.x, lane_fq(x));
        st_ref(e.y, lane_fq(y));
    });
}

// a lane's 64 bytes of an entry, and its coordinates of x and y (F<2>{..}: Fq itself, or the
// Fq2 of the two-lane layout around the lane's coordinate)
struct BasisRaw {
    uint4 q[4];
};
template <template <int> class F>
__device__ __forceinline__ void basis_decode(const BasisRaw& e, F<2>& x, F<2>& y) {
    const uint32_t wx[8] = {e.q[0].x, e.q[0].y, e.q[0].z, e.q[0].w, e.q[1].x, e.q[1].y, e.q[1].z, e.q[1].w};
    const uint32_t wy[8] = {e.q[2].x, e.q[2].y, e.q[2].z, e.q[2].w, e.q[3].x, e.q[3].y, e.q[3].z, e.q[3].w};
    x = F<2>{fq_load_ref(wx)};
    y = F<2>{fq_load_ref(wy)};
}
// The sum of the entries [lo, hi) of the region that starts at word `first` of sorted (0 for
// a single vector; a set's positions are 32-bit, so the loop keeps one index and the uniform
// base), of a key of window w < W(c) over the first n <= nbases bases.
template <template <int> class F, class P>
__device__ __forceinline__ Jac<F> basis_run_sum(const typename MsmIo<P>::Elem* table, uint32_t nbases, uint32_t n,
                                                uint32_t w, const uint32_t* sorted, uint32_t first, uint32_t lo,
                                                uint32_t hi) {
    const auto* row = MsmIo<P>::entry(table, (size_t)msm_basis_index(nbases, 0, w));
    lo += first, hi += first;
    return msm_basis_run_sum<F>([&](uint32_t e) { return sorted[e]; },
                                [&](uint32_t idx) {
                                    const uint4* p = reinterpret_cast<const uint4*>(row + 2 * (size_t)(idx < n ? idx : 0));
                                    return BasisRaw{{p[0], p[1], p[2], p[3]}};
                                },
                                basis_decode<F>, n, lo, hi);
}
// Element `key` of the (window, bucket) keys: the sum of its run of sorted entries by mixed
// additions.  An empty bucket is zero.  A run of more than L entries is left to the chunk
// and fold kernels, which write its bucket.  n <= nbases terms; nkeys = W(c) * 2^(c-1), so a
// key's window is below W(c).
template <template <int> class F, class P>
__device__ __forceinline__ void msm_basis_accumulate_body(size_t key, const typename MsmIo<P>::Elem* table,
                                                          uint32_t nbases, uint32_t n, int c, const uint32_t* sorted,
                                                          const uint32_t* offsets, uint32_t nkeys, uint32_t nent,
                                                          uint32_t L, P* buckets) {
    if (key >= nkeys || nkeys != msm_num_keys(c) || n > nbases) return;
    const MsmRun run = msm_key_run(offsets, key, nent);
    if (run.hi - run.lo > L) return;
    MsmIo<P>::st(buckets[key], basis_run_sum<F, P>(table, nbases, n, (uint32_t)msm_key_window(c, (uint32_t)key), sorted,
                                                   0, run.lo, run.hi));
}
// Element t of the level-0 slots: the sum of one chunk of at most L entries of a long key's
// run (msm.h msm_run_task), as msm_chunk_body.
template <template <int> class F, class P>
__device__ __forceinline__ void msm_basis_chunk_body(size_t t, const typename MsmIo<P>::Elem* table, uint32_t nbases,
                                                     uint32_t n, int c, const uint32_t* sorted, const uint32_t* offsets,
                                                     const uint32_t* longinfo, uint32_t nkeys, uint32_t nent, uint32_t L,
                                                     P* sums, uint32_t nslots) {
    if (t >= nslots || nkeys != msm_num_keys(c) || n > nbases) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, 0, (uint32_t)t);
    if (!task.some) return;
    MsmIo<P>::st(sums[t], basis_run_sum<F, P>(table, nbases, n, (uint32_t)msm_key_window(c, task.key), sorted, 0,
                                              task.lo, task.hi));
}
// Element t = s * 2 + which of the (segment, which of the two windows) pairs: parts[t] = the
// segment's weighted sum (msm_group.h msm_segment_sum) of the collapsed row (which = 0:
// window 0's slots) or of the top window (which = 1), so that the addition tree over the
// segments is the group's k_*_op on contiguous halves.
template <template <int> class F, class P>
__device__ __forceinline__ void msm_basis_reduce_body(size_t t, const P* buckets, int c, uint32_t nkeys, uint32_t nseg,
                                                      P* parts) {
    using IO = MsmIo<P>;
    if (t >= (size_t)nseg * 2) return;
    const uint32_t s = (uint32_t)(t / 2), w = msm_basis_reduce_window(c, (uint32_t)(t % 2));
    IO::st(parts[t], msm_segment_sum<F>([&](uint32_t key) { return IO::ld(buckets[key]); }, c, nkeys, s, w));
}

}  // namespace bn
