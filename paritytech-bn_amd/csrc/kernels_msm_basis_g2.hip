// kernels_msm_basis_g2.hip -- one large G2 multi-scalar multiplication over a fixed basis
// (bn_g2_basis_prepare, bn_g2_msm_basis; the bodies are msm_basis.h's over
// Fq2) on the pairing path's two-lane layout (fq2_split.h): lanes 2j and 2j + 1 hold
// coordinates c0 and c1 of the points of element j.
// Once per handle:
//   k_g2_basis_build           one lane pair per base: its W(c) entries 2^(c*w) * B and its zero flag
// Per call, between the recoding, histogram, scan and scatter of kernels_msm.hip over the
// zero flags (k_msm_count_basis, k_msm_scatter_basis, k_msm_scan) and k_msm_fold_g2, k_g2_op
// and k_msm_finish_g2 as they are:
//   k_msm_basis_accumulate_g2  one lane pair per (window, bucket) key: mixed additions of its run's entries
//   k_msm_basis_chunk_g2       one lane pair per chunk of a long key's run: the chunk's sum
//   (k_g2_op add)              the buckets of the windows below the top one added row-wise (capi_msm.hip)
//   k_msm_basis_reduce_g2      one lane pair per (segment, one of two windows): its weighted sum
// Table: entry (b, w) at index w * nbases + b (msm_basis.h), 128 bytes stored as two lane
// halves [x.c0, y.c0 | x.c1, y.c1]: bn_fq2 number 2 * index + h is lane h's half, its c0 the
// lane's coordinate of x and its c1 that of y, so each lane of a pair gathers its own
// coordinates with one aligned 64-byte read.
// Pair-uniform control (kernels_msm_g2.hip): every Fq2 product and zero test reads the
// partner lane over DPP, so both lanes of a pair must take every branch and leave every
// loop together.  The element is lane_id() / kL; the run's bounds, each entry's word, its
// sign and its index against n (msm_basis_run_sum's pending and take) come from loads both
// lanes make at the same address, and jac_add_mixed's guards from fq2_is_zero, which is
// pair-uniform; only the table address differs between the two lanes.  The block size is
// even, so a grid covers whole pairs.  Every computed index is bounded against its array in
// the kernel; a lane pair whose index is out of range does nothing, and no block waits for
// another.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "fq.h"
#define BN_SPLIT 1
#include "kernels.h"
#include "msm_basis.h"

namespace bn {

constexpr size_t kL = kPathLanes;  // lanes per element in this translation unit

// this lane's coordinates of a point's reference image
__device__ __forceinline__ G2J ld_g2(const bn_g2& a) {
    return {widen<kPt>(ld_ref2(a.x)), widen<kPt>(ld_ref2(a.y)), widen<kPt>(ld_ref2(a.z))};
}
__device__ __forceinline__ void st_g2(bn_g2& o, const G2J& r) {
    st_ref2(o.x, r.x);
    st_ref2(o.y, r.y);
    st_ref2(o.z, r.z);
}
// this lane's half of table entry `index`: c0 holds the lane's coordinate of x, c1 of y
__device__ __forceinline__ bn_fq2* basis_half(bn_fq2* table, size_t index) {
    return table + 2 * index + (lane_odd() ? 1 : 0);
}
__device__ __forceinline__ const bn_fq2* basis_half(const bn_fq2* table, size_t index) {
    return table + 2 * index + (lane_odd() ? 1 : 0);
}

// ---------------------------------------------------------------- table build
// Lane pair b: entries (b, 0 .. W(c)) and the base's zero flag.  A zero base's entries are
// written as zeros: the accumulation's idle fetches read base 0's entry, so every entry
// holds field elements.  The flag is pair-uniform (jac_is_zero over Fq2).
__global__ void __launch_bounds__(kBlock) k_g2_basis_build(const bn_g2* __restrict__ bases, uint32_t nbases, int c,
                                                           bn_fq2* __restrict__ table, uint8_t* __restrict__ zero) {
    fold_table_init();
    const size_t t = lane_id() / kL;
    if (t >= nbases) return;
    const uint32_t b = (uint32_t)t;
    const G2J base = ld_g2(bases[b]);
    const bool bzero = jac_is_zero(base);
    zero[b] = bzero ? 1 : 0;  // both lanes of the pair store the same byte
    if (bzero) {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t w = 0; w < (uint32_t)msm_windows(c); ++w) {
            bn_fq2* e = basis_half(table, (size_t)msm_basis_index(nbases, b, w));
            st_words(&e->c0, z);
            st_words(&e->c1, z);
        }
        return;
    }
    msm_basis_build<Fq2>(base, c, [&](uint32_t w, const Fq2<kPt>& x, const Fq2<kPt>& y) {
        bn_fq2* e = basis_half(table, (size_t)msm_basis_index(nbases, b, w));
        st_ref(e->c0, x.c);
        st_ref(e->c1, y.c);
    });
}

// ---------------------------------------------------------------- bucket accumulation
struct BasisRaw2 {
    uint4 q[4];
};
__device__ __forceinline__ void basis_decode2(const BasisRaw2& e, Fq2<2>& x, Fq2<2>& y) {
    const uint32_t wx[8] = {e.q[0].x, e.q[0].y, e.q[0].z, e.q[0].w, e.q[1].x, e.q[1].y, e.q[1].z, e.q[1].w};
    const uint32_t wy[8] = {e.q[2].x, e.q[2].y, e.q[2].z, e.q[2].w, e.q[3].x, e.q[3].y, e.q[3].z, e.q[3].w};
    x = {fq_load_ref(wx)};
    y = {fq_load_ref(wy)};
}
// the sum of sorted[lo .. hi) of a key of window w < W(c) over the first n <= nbases bases
__device__ __forceinline__ G2J basis_run_sum2(const bn_fq2* __restrict__ table, uint32_t nbases, uint32_t n, uint32_t w,
                                              const uint32_t* __restrict__ sorted, uint32_t lo, uint32_t hi) {
    const bn_fq2* row = basis_half(table, (size_t)msm_basis_index(nbases, 0, w));
    return msm_basis_run_sum<Fq2>([&](uint32_t e) { return sorted[e]; },
                                  [&](uint32_t idx) {
                                      const uint4* p = reinterpret_cast<const uint4*>(row + 2 * (size_t)(idx < n ? idx : 0));
                                      return BasisRaw2{{p[0], p[1], p[2], p[3]}};
                                  },
                                  basis_decode2, n, lo, hi);
}
// One lane pair per (window, bucket): the sum of its run of sorted entries.  An empty bucket
// is zero.  A run of more than L entries is left to k_msm_basis_chunk_g2 / k_msm_fold_g2,
// which write its bucket.  n <= nbases terms; nkeys = W(c) * 2^(c-1), so a key's window is
// below W(c).
__global__ void __launch_bounds__(kBlock) k_msm_basis_accumulate_g2(const bn_fq2* __restrict__ table, uint32_t nbases,
                                                                    uint32_t n, int c,
                                                                    const uint32_t* __restrict__ sorted,
                                                                    const uint32_t* __restrict__ offsets, uint32_t nkeys,
                                                                    uint32_t nent, uint32_t L,
                                                                    bn_g2* __restrict__ buckets) {
    fold_table_init();
    const size_t key = lane_id() / kL;
    if (key >= nkeys || nkeys != msm_num_keys(c) || n > nbases) return;
    uint32_t hi = offsets[key + 1];
    hi = hi < nent ? hi : nent;
    uint32_t lo = offsets[key];
    lo = lo < hi ? lo : hi;
    if (hi - lo > L) return;
    st_g2(buckets[key], basis_run_sum2(table, nbases, n, (uint32_t)msm_key_window(c, (uint32_t)key), sorted, lo, hi));
}
// One lane pair per level-0 slot: the sum of one chunk of at most L entries of a long key's
// run (msm.h msm_run_task), as k_msm_chunk_g2.
__global__ void __launch_bounds__(kBlock) k_msm_basis_chunk_g2(const bn_fq2* __restrict__ table, uint32_t nbases,
                                                               uint32_t n, int c, const uint32_t* __restrict__ sorted,
                                                               const uint32_t* __restrict__ offsets,
                                                               const uint32_t* __restrict__ longinfo, uint32_t nkeys,
                                                               uint32_t nent, uint32_t L, bn_g2* __restrict__ sums,
                                                               uint32_t nslots) {
    fold_table_init();
    const size_t t = lane_id() / kL;
    if (t >= nslots || nkeys != msm_num_keys(c) || n > nbases) return;
    const MsmRunTask task = msm_run_task(longinfo + 1, offsets, longinfo[0], nkeys, nent, L, 0, (uint32_t)t);
    if (!task.some) return;
    st_g2(sums[t], basis_run_sum2(table, nbases, n, (uint32_t)msm_key_window(c, task.key), sorted, task.lo, task.hi));
}

// ---------------------------------------------------------------- bucket reduction
// One lane pair per (segment, which of the two windows): parts[s * 2 + which] = the segment's
// weighted sum (msm_group.h msm_segment_sum) of the collapsed row (which = 0: window 0's
// slots) or of the top window (which = 1), so that the addition tree over the segments is
// k_g2_op on contiguous halves.
__global__ void __launch_bounds__(kBlock) k_msm_basis_reduce_g2(const bn_g2* __restrict__ buckets, int c, uint32_t nkeys,
                                                                uint32_t nseg, bn_g2* __restrict__ parts) {
    fold_table_init();
    const size_t t = lane_id() / kL;
    if (t >= (size_t)nseg * 2) return;
    const uint32_t s = (uint32_t)(t / 2), w = msm_basis_reduce_window(c, (uint32_t)(t % 2));
    st_g2(parts[t], msm_segment_sum<Fq2>([&](uint32_t key) { return ld_g2(buckets[key]); }, c, nkeys, s, w));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_basis_g2)
