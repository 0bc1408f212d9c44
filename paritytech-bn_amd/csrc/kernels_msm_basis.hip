// kernels_msm_basis.hip -- one large G1 multi-scalar multiplication over a fixed basis
// (bn_g1_basis_prepare, bn_g1_msm_basis; the bodies are msm_basis.h's).
// Once per handle:
//   k_g1_basis_build         one lane per base: its W(c) entries 2^(c*w) * B and its zero flag
// Per call, between the recoding, histogram, scan and scatter of kernels_msm.hip (with the
// zero flags in place of the points) and k_msm_fold, k_g1_op and k_msm_finish as they are:
//   k_msm_basis_accumulate   one lane per (window, bucket) key: mixed additions of its run's entries
//   k_msm_basis_chunk        one lane per chunk of a long key's run: the chunk's sum
//   (k_g1_op add)            the buckets of the windows below the top one added row-wise (capi_msm.hip)
//   k_msm_basis_reduce       one lane per (segment, one of two windows): its weighted sum
// Every computed index is bounded against its array in the kernel; a lane whose index is
// out of range does nothing.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "kernels.h"
#include "msm_basis.h"

namespace bn {

__device__ __forceinline__ G1J ld_g1(const bn_g1& a) {
    return {widen<kPt>(ld_ref(a.x)), widen<kPt>(ld_ref(a.y)), widen<kPt>(ld_ref(a.z))};
}
__device__ __forceinline__ void st_g1(bn_g1& o, const G1J& r) {
    st_ref(o.x, r.x);
    st_ref(o.y, r.y);
    st_ref(o.z, r.z);
}

// ---------------------------------------------------------------- table build
// Lane b: entries (b, 0 .. W(c)) as reference images (x, y) and the base's zero flag.  A zero
// base's entries are written as zeros: the accumulation's idle fetches read base 0's entry,
// so every entry holds a field element.
__global__ void __launch_bounds__(kBlock) k_g1_basis_build(const bn_g1* __restrict__ bases, uint32_t nbases, int c,
                                                           bn_fq* __restrict__ table, uint8_t* __restrict__ zero) {
    fold_table_init();
    const size_t t = lane_id();
    if (t >= nbases) return;
    const uint32_t b = (uint32_t)t;
    const G1J base = ld_g1(bases[b]);
    const bool bzero = jac_is_zero(base);
    zero[b] = bzero ? 1 : 0;
    if (bzero) {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t w = 0; w < (uint32_t)msm_windows(c); ++w) {
            st_words(&table[2 * (size_t)msm_basis_index(nbases, b, w)], z);
            st_words(&table[2 * (size_t)msm_basis_index(nbases, b, w) + 1], z);
        }
        return;
    }
    msm_basis_build<Fq>(base, c, [&](uint32_t w, const Fq<kPt>& x, const Fq<kPt>& y) {
        st_ref(table[2 * (size_t)msm_basis_index(nbases, b, w)], x);
        st_ref(table[2 * (size_t)msm_basis_index(nbases, b, w) + 1], y);
    });
}

// ---------------------------------------------------------------- bucket accumulation
struct BasisRaw {
    uint4 q[4];
};
__device__ __forceinline__ void basis_decode(const BasisRaw& e, Fq<2>& x, Fq<2>& y) {
    const uint32_t wx[8] = {e.q[0].x, e.q[0].y, e.q[0].z, e.q[0].w, e.q[1].x, e.q[1].y, e.q[1].z, e.q[1].w};
    const uint32_t wy[8] = {e.q[2].x, e.q[2].y, e.q[2].z, e.q[2].w, e.q[3].x, e.q[3].y, e.q[3].z, e.q[3].w};
    x = fq_load_ref(wx);
    y = fq_load_ref(wy);
}
// the sum of sorted[lo .. hi) of a key of window w < W(c) over the first n <= nbases bases
__device__ __forceinline__ G1J basis_run_sum(const bn_fq* __restrict__ table, uint32_t nbases, uint32_t n, uint32_t w,
                                             const uint32_t* __restrict__ sorted, uint32_t lo, uint32_t hi) {
    const bn_fq* row = table + 2 * (size_t)msm_basis_index(nbases, 0, w);
    return msm_basis_run_sum<Fq>([&](uint32_t e) { return sorted[e]; },
                                 [&](uint32_t idx) {
                                     const uint4* p = reinterpret_cast<const uint4*>(row + 2 * (size_t)(idx < n ? idx : 0));
                                     return BasisRaw{{p[0], p[1], p[2], p[3]}};
                                 },
                                 basis_decode, n, lo, hi);
}
// One lane per (window, bucket): the sum of its run of sorted entries.  An empty bucket is
// zero.  A run of more than L entries is left to k_msm_basis_chunk / k_msm_fold, which write
// its bucket.  n <= nbases terms; nkeys = W(c) * 2^(c-1), so a key's window is below W(c).
__global__ void __launch_bounds__(kBlock) k_msm_basis_accumulate(const bn_fq* __restrict__ table, uint32_t nbases,
                                                                 uint32_t n, int c, const uint32_t* __restrict__ sorted,
                                                                 const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                                 uint32_t nent, uint32_t L, bn_g1* __restrict__ buckets) {
    fold_table_init();
    const size_t key = lane_id();
    if (key >= nkeys || nkeys != msm_num_keys(c) || n > nbases) return;
    uint32_t hi = offsets[key + 1];
    hi = hi < nent ? hi : nent;
    uint32_t lo = offsets[key];
    lo = lo < hi ? lo : hi;
    if (hi - lo > L) return;
    st_g1(buckets[key], basis_run_sum(table, nbases, n, (uint32_t)msm_key_window(c, (uint32_t)key), sorted, lo, hi));
}
// One lane per level-0 slot: the sum of one chunk of at most L entries of a long key's run
// (msm.h msm_run_task), as k_msm_chunk.
__global__ void __launch_bounds__(kBlock) k_msm_basis_chunk(const bn_fq* __restrict__ table, uint32_t nbases, uint32_t n,
                                                            int c, const uint32_t* __restrict__ sorted,
                                                            const uint32_t* __restrict__ offsets,
                                                            const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                            uint32_t nent, uint32_t L, bn_g1* __restrict__ sums,
                                                            uint32_t nslots) {
    fold_table_init();
    const size_t t = lane_id();
    if (t >= nslots || nkeys != msm_num_keys(c) || n > nbases) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, 0, (uint32_t)t);
    if (!task.some) return;
    st_g1(sums[t], basis_run_sum(table, nbases, n, (uint32_t)msm_key_window(c, task.key), sorted, task.lo, task.hi));
}

// ---------------------------------------------------------------- bucket reduction
// One lane per (segment, which of the two windows): parts[s * 2 + which] = the segment's
// weighted sum (msm_group.h msm_segment_sum) of the collapsed row (which = 0: window 0's
// slots) or of the top window (which = 1), so that the addition tree over the segments is
// k_g1_op on contiguous halves.
__global__ void __launch_bounds__(kBlock) k_msm_basis_reduce(const bn_g1* __restrict__ buckets, int c, uint32_t nkeys,
                                                             uint32_t nseg, bn_g1* __restrict__ parts) {
    fold_table_init();
    const size_t t = lane_id();
    if (t >= (size_t)nseg * 2) return;
    const uint32_t s = (uint32_t)(t / 2), w = msm_basis_reduce_window(c, (uint32_t)(t % 2));
    st_g1(parts[t], msm_segment_sum<Fq>([&](uint32_t key) { return ld_g1(buckets[key]); }, c, nkeys, s, w));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_basis)
