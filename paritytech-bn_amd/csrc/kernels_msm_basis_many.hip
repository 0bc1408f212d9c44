// kernels_msm_basis_many.hip -- a batch of scalar vectors over one fixed G1 basis in one pass
// (bn_g1_msm_basis_many).  Every vector is the pipeline of
// kernels_msm_basis.hip on arrays of its own; a launch set of S vectors runs each phase in
// one launch, the lanes indexed (vector, term), (vector, key), (vector, slot) or (segment,
// window, vector) by msm_basis_many.h, so a set pays the single call's chain of dependent
// launches once:
//   k_msm_basis_many_count       one lane per (vector, term): histogram of the vector's keys
//   k_msm_basis_many_scan        one block per vector: the one-block scan (msm_sort.h)
//   k_msm_basis_many_scatter     one lane per (vector, term): its entries into the vector's region
//   k_msm_basis_many_accumulate  one lane per (vector, key): mixed additions of its run's entries
//   k_msm_basis_many_chunk       one lane per (vector, chunk of a long key's run)
//   k_msm_basis_many_fold        one lane per (vector, group of partial sums), once per level
//   (k_g1_op add)                the rows of the windows below the top one added, all vectors at once
//   k_msm_basis_many_reduce      one lane per (segment, one of two windows, vector)
//   (k_g1_op add, k_g1_msm_fixed_finish)  the trees over the parts, the S returned images
//   k_msm_basis_many_zero        one lane per output: the image of zero (n == 0)
// Every computed index is bounded against its array in the kernel; a lane whose index is
// out of range does nothing.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "kernels.h"
#include "msm_kernels.h"
#include "msm_basis_many.h"
#include "msm_sort.h"

namespace bn {

// a set's lane indices are 32-bit (msm_basis_many.h); S: no such lane
__device__ __forceinline__ MsmBasisManyLane many_lane(uint32_t per, uint32_t S) {
    const size_t t = lane_id();
    return t >> 32 ? MsmBasisManyLane{S, 0u} : msm_basis_many_lane((uint32_t)t, per, S);
}
// the set's shape is one vector's plan: nkeys keys at width c, nent = n * W(c) positions
__device__ __forceinline__ bool many_shape_ok(const MsmBasisManyShape& g, uint32_t nbases) {
    return msm_window_ok(g.c) && g.nkeys == msm_num_keys(g.c) && g.n <= nbases &&
           (uint64_t)g.n * (uint32_t)msm_windows(g.c) == g.nent;
}

// ---------------------------------------------------------------- recoding, histogram, scatter
// One lane per (vector, term): kernels_msm.hip's msm_digits with the vector's block of `keys`
// and region of `sorted`.  The claim's key is the word's index in `keys` (block and key), so
// lanes of one wave that hold the same key of different vectors do not share an atomic.
template <bool kScatter>
__device__ __forceinline__ void many_digits(const uint8_t* __restrict__ zero, uint32_t nbases,
                                            const bn_fr* __restrict__ k, size_t k_stride, MsmBasisManyShape g,
                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ sorted) {
    fold_table_init();
    if (!many_shape_ok(g, nbases) || k_stride < g.n) return;
    const MsmBasisManyLane at = many_lane(g.n, g.S);
    if (at.v >= g.S) return;
    if (zero[at.i] != 0) return;
    uint32_t s[8];
    fr_to_canonical(k[(size_t)at.v * k_stride + at.i], s);
    const uint32_t first = (uint32_t)(kScatter ? msm_basis_many_cursors_at(g.nkeys, at.v) : msm_basis_many_counts_at(g.nkeys, at.v));
    const uint32_t* offsets = keys + msm_basis_many_offsets_at(g.nkeys, at.v);
    uint32_t* region = sorted + msm_basis_many_sorted_at(g.nent, at.v);
    uint32_t carry = 0;
    const int nw = msm_windows(g.c);
    for (int w = 0; w < nw; ++w) {  // the same trip count on every lane: msm_claim's ballots see the whole wave
        const int32_t d = msm_signed_digit(msm_raw_window(s, g.c, w), g.c, &carry);
        const uint32_t key = d != 0 ? msm_key(g.c, w, d, at.i) : g.nkeys;
        const bool has = key < g.nkeys;
        const uint32_t pos = msm_claim(keys, first + (has ? key : 0u), has);
        if constexpr (kScatter) {
            if (has && pos < offsets[key + 1] && pos < g.nent) region[pos] = msm_entry(at.i, d);
        }
    }
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_many_count(const uint8_t* __restrict__ zero, uint32_t nbases,
                                                                 const bn_fr* __restrict__ k, size_t k_stride,
                                                                 MsmBasisManyShape g, uint32_t* __restrict__ keys) {
    many_digits<false>(zero, nbases, k, k_stride, g, keys, nullptr);
}
__global__ void __launch_bounds__(kBlock) k_msm_basis_many_scatter(const uint8_t* __restrict__ zero, uint32_t nbases,
                                                                   const bn_fr* __restrict__ k, size_t k_stride,
                                                                   MsmBasisManyShape g, uint32_t* __restrict__ keys,
                                                                   uint32_t* __restrict__ sorted) {
    many_digits<true>(zero, nbases, k, k_stride, g, keys, sorted);
}
// Block v: k_msm_scan's block on vector v's words.  The S scans run side by side.
__global__ void __launch_bounds__(kMsmScanBlock) k_msm_basis_many_scan(uint32_t* __restrict__ keys, uint32_t nkeys,
                                                                       uint32_t S, uint32_t L) {
    const uint32_t v = blockIdx.x;
    if (v >= S) return;  // block-uniform
    msm_scan_block(keys + msm_basis_many_counts_at(nkeys, v), nkeys, keys + msm_basis_many_offsets_at(nkeys, v),
                   keys + msm_basis_many_cursors_at(nkeys, v), L, keys + msm_basis_many_longinfo_at(nkeys, v));
}

// ---------------------------------------------------------------- bucket accumulation
// One lane per (vector, key): the sum of the key's run in the vector's region, into the
// vector's bucket of that key (k_msm_basis_accumulate with the vector index around it).  A
// run above L entries is left to the chunk and fold kernels.
__global__ void __launch_bounds__(kBlock) k_msm_basis_many_accumulate(const bn_fq* __restrict__ table, uint32_t nbases,
                                                                      MsmBasisManyShape g,
                                                                      const uint32_t* __restrict__ keys,
                                                                      const uint32_t* __restrict__ sorted, uint32_t L,
                                                                      bn_g1* __restrict__ buckets) {
    fold_table_init();
    if (!many_shape_ok(g, nbases)) return;
    const MsmBasisManyLane at = many_lane(g.nkeys, g.S);
    if (at.v >= g.S) return;
    const uint32_t key = at.i;
    const MsmRun run = msm_key_run(keys + msm_basis_many_offsets_at(g.nkeys, at.v), key, g.nent);
    if (run.hi - run.lo > L) return;
    // the bucket's index is 32-bit (S * nkeys < 2^30): all the loop keeps of (vector, key)
    const uint32_t dst = (uint32_t)msm_basis_many_bucket(g.c, g.S, at.v, key);
    st_g1(buckets[dst], basis_run_sum<Fq, bn_g1>(table, nbases, g.n, (uint32_t)msm_key_window(g.c, key), sorted,
                                                 (uint32_t)msm_basis_many_sorted_at(g.nent, at.v), run.lo, run.hi));
}
// One lane per (vector, level-0 slot): the sum of one chunk of at most L entries of a long
// key's run of that vector (msm.h msm_run_task on the vector's block), into slot
// v * slots + t of sums.
__global__ void __launch_bounds__(kBlock) k_msm_basis_many_chunk(const bn_fq* __restrict__ table, uint32_t nbases,
                                                                 MsmBasisManyShape g, const uint32_t* __restrict__ keys,
                                                                 const uint32_t* __restrict__ sorted, uint32_t L,
                                                                 bn_g1* __restrict__ sums, uint32_t slots) {
    fold_table_init();
    if (!many_shape_ok(g, nbases)) return;
    const MsmBasisManyLane at = many_lane(slots, g.S);
    if (at.v >= g.S) return;
    const uint32_t* longinfo = keys + msm_basis_many_longinfo_at(g.nkeys, at.v);
    const MsmRunTask task = msm_run_task(longinfo + 1, keys + msm_basis_many_offsets_at(g.nkeys, at.v), longinfo[0],
                                         g.nkeys, g.nent, L, 0, at.i);
    if (!task.some) return;
    st_g1(sums[(size_t)at.v * slots + at.i],
          basis_run_sum<Fq, bn_g1>(table, nbases, g.n, (uint32_t)msm_key_window(g.c, task.key), sorted,
                                   (uint32_t)msm_basis_many_sorted_at(g.nent, at.v), task.lo, task.hi));
}
// One lane per (vector, slot of fold level `level` >= 1): k_msm_fold on the vector's slots.
// src holds src_slots slots per vector, dst dst_slots (0 at the last level, which writes
// buckets only); the level has `slots` lanes per vector.
__global__ void __launch_bounds__(kBlock) k_msm_basis_many_fold(MsmBasisManyShape g, const uint32_t* __restrict__ keys,
                                                                uint32_t L, int level, const bn_g1* __restrict__ src,
                                                                uint32_t src_slots, bn_g1* __restrict__ dst,
                                                                uint32_t dst_slots, uint32_t slots,
                                                                bn_g1* __restrict__ buckets) {
    fold_table_init();
    if (!msm_window_ok(g.c) || g.nkeys != msm_num_keys(g.c)) return;
    const MsmBasisManyLane at = many_lane(slots, g.S);
    if (at.v >= g.S) return;
    const uint32_t* longinfo = keys + msm_basis_many_longinfo_at(g.nkeys, at.v);
    const MsmRunTask task = msm_run_task(longinfo + 1, keys + msm_basis_many_offsets_at(g.nkeys, at.v), longinfo[0],
                                         g.nkeys, g.nent, L, level, at.i);
    if (!task.some || task.hi > src_slots || (!task.last && at.i >= dst_slots)) return;
    const bn_g1* from = src + (size_t)at.v * src_slots;
    const G1J acc = msm_fold_sum<Fq>([&](uint32_t i) { return ld_g1(from[i]); }, task.lo, task.hi);
    st_g1(task.last ? buckets[msm_basis_many_bucket(g.c, g.S, at.v, task.key)] : dst[(size_t)at.v * dst_slots + at.i], acc);
}

// ---------------------------------------------------------------- bucket reduction
// One lane per (segment, which of the two windows, vector): parts[(s * 2 + which) * S + v] =
// the segment's weighted sum (msm_group.h msm_segment_sum) of the vector's collapsed row
// (which = 0) or top window (which = 1).
__global__ void __launch_bounds__(kBlock) k_msm_basis_many_reduce(const bn_g1* __restrict__ buckets, int c,
                                                                  uint32_t nkeys, uint32_t nseg, uint32_t S,
                                                                  bn_g1* __restrict__ parts) {
    fold_table_init();
    const size_t t = lane_id();
    if (S == 0 || t >> 32 || t >= (size_t)nseg * 2 * S || !msm_window_ok(c) || nkeys != msm_num_keys(c)) return;
    const MsmBasisManyPart at = msm_basis_many_part((uint32_t)t, S);
    st_g1(parts[t], msm_segment_sum<Fq>([&](uint32_t key) { return ld_g1(buckets[msm_basis_many_bucket(c, S, at.v, key)]); },
                                        c, nkeys, at.s, msm_basis_reduce_window(c, at.which)));
}
// out[j * stride] = the returned image of zero, j < m (a call of n == 0 terms)
__global__ void __launch_bounds__(kBlock) k_msm_basis_many_zero(size_t m, bn_g1* __restrict__ out, size_t stride) {
    fold_table_init();
    const size_t j = lane_id();
    if (j >= m) return;
    st_g1(out[j * stride], msm_finish_point(jac_zero<Fq>()));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_basis_many)
