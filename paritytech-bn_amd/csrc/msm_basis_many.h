// msm_basis_many.h -- the index arithmetic of a BATCH of scalar vectors over one fixed basis
// (bn_g1_msm_basis_many; kernels_msm_basis_many.hip).  Plain integer code,
// host and device, so tests/native/msm_basis_many_emul.cpp compiles with g++ alone the same
// positions the kernels compute.
//
// Every vector is the single call's pipeline (msm_basis.h) on arrays of its own; what is new
// is the vector index v < S around them, S the vectors of one launch set:
//   integer words   vector v's block of msm_basis_many_words(nkeys) words at v times that:
//                   counts | cursors | offsets (nkeys + 1) | long keys (1 + nkeys), as the
//                   single call carves them, so msm_run_task runs unchanged on a block
//   sorted entries  vector v's region of nent = n * W(c) words at v * nent (zero digits leave
//                   a region partly empty: the vector's offsets[nkeys] says how far it is filled)
//   chunk sums      vector v's slots of a level at v * (the level's array's slots per vector)
//   buckets         key (w, slot) of vector v at (w * S + v) * 2^(c-1) + slot: a window's row
//                   is S * 2^(c-1) points wide, so the collapse of the windows below the top
//                   one is one addition tree over rows for all vectors at once
//   parts           segment s, window `which` of two, vector v at (s * 2 + which) * S + v: the
//                   tree over the segments is on width 2 S, the two window sums on width S
// A lane index t of a kernel with `per` lanes per vector is (v, local) = (t / per, t % per),
// but the reduction's, which has the vector innermost like its output.  Lane indices are
// 32-bit: msm_basis_many_set keeps S * n * W(c) <= 2^31 - 1, S times the level-0 slots and S
// times a block's 4 nkeys + 2 words below 2^32.
#pragma once
#include "msm_basis.h"

namespace bn {

// the most vectors of a call, and the most a launch set can be forced to
constexpr uint64_t kMsmBasisManyMaxVectors = 1ull << 26;
// Default bound on S * nkeys, the (vector, key) lanes and bucket sums of a launch set: 2^23
// is 768 MiB of bucket sums, the fastest of 2^21, 2^22 and 2^23 at both measured shapes
// (profiles/msm_basis_many_set.jsonl).
constexpr uint64_t kMsmBasisManySetKeys = 1ull << 23;

// The shape of a launch set, a kernel argument: S vectors of n terms at width c, each with
// nkeys = W(c) * 2^(c-1) keys and a region of nent = n * W(c) sorted positions.
struct MsmBasisManyShape {
    uint32_t S, n, nkeys, nent;
    int c;
};

// words of one vector's block of the integer buffer
BN_INLINE uint64_t msm_basis_many_words(uint32_t nkeys) { return 4ull * nkeys + 2ull; }
// the parts of vector v's block, as word offsets into the integer buffer
BN_INLINE uint64_t msm_basis_many_counts_at(uint32_t nkeys, uint32_t v) { return v * msm_basis_many_words(nkeys); }
BN_INLINE uint64_t msm_basis_many_cursors_at(uint32_t nkeys, uint32_t v) {
    return msm_basis_many_counts_at(nkeys, v) + nkeys;
}
BN_INLINE uint64_t msm_basis_many_offsets_at(uint32_t nkeys, uint32_t v) {
    return msm_basis_many_counts_at(nkeys, v) + 2ull * nkeys;
}
BN_INLINE uint64_t msm_basis_many_longinfo_at(uint32_t nkeys, uint32_t v) {
    return msm_basis_many_counts_at(nkeys, v) + 3ull * nkeys + 1ull;
}
// first word of vector v's region of sorted entries
BN_INLINE uint64_t msm_basis_many_sorted_at(uint32_t nent, uint32_t v) { return (uint64_t)v * nent; }

// (vector, local index) of lane t with `per` lanes per vector; v >= S: no such lane
struct MsmBasisManyLane {
    uint32_t v, i;
};
BN_INLINE MsmBasisManyLane msm_basis_many_lane(uint32_t t, uint32_t per, uint32_t S) {
    if (per == 0) return {S, 0u};
    const uint32_t v = t / per;
    return {v < S ? v : S, t - v * per};
}
// bucket of key < W(c) * 2^(c-1) of vector v < S
BN_INLINE uint64_t msm_basis_many_bucket(int c, uint32_t S, uint32_t v, uint32_t key) {
    const uint32_t nb = msm_buckets(c);
    return ((uint64_t)(key >> (c - 1)) * S + v) * nb + (key & (nb - 1u));
}
// (segment, which of the two reduced windows, vector) of lane t of the reduction; the lane
// writes parts[t]
struct MsmBasisManyPart {
    uint32_t s, which, v;
};
BN_INLINE MsmBasisManyPart msm_basis_many_part(uint32_t t, uint32_t S) {
    const uint32_t q = t / S;
    return {q / 2u, q & 1u, t - q * S};
}

// The slots per vector of the even levels' array (a) and the odd levels' (b) of the chunk and
// fold tree: the bounds of levels 0 and 1 (msm.h msm_level_slots), which bound every level
// above them too -- s_1 <= s_0 because the long keys are at most floor(nent / L), and
// s_(k+1) = s_k / F + l <= s_(k-1) / F + l = s_k from there on.
BN_INLINE uint32_t msm_basis_many_slots(uint32_t nent, uint32_t nkeys, uint32_t L, int levels, int odd) {
    if (levels <= odd) return 0u;
    return msm_level_slots(nent, nkeys, L, odd);
}

// The vectors of a launch set of a call of m vectors of n terms at width c: the largest S with
// S * nkeys <= max_keys (the bound on bucket memory; 0: kMsmBasisManySetKeys) and
// S * n * W(c) <= 2^31 - 1, at least 1 and at most m; `forced` != 0 takes the place of the
// bucket bound.  Whatever is asked, a set's lanes and positions stay 32-bit: the level-0
// slots of a vector are at most 2 n W(c) (msm.h msm_level_slots), so S times them stays below
// 2^32 with the entries, and S times a block's words is held below 2^32 here.
BN_INLINE uint64_t msm_basis_many_set(uint64_t m, uint64_t n, int c, uint64_t max_keys, uint64_t forced) {
    const uint64_t nkeys = msm_num_keys(c), nent = n * (uint64_t)msm_windows(c);
    const uint64_t words = msm_basis_many_words((uint32_t)nkeys);
    uint64_t S = forced ? forced : (max_keys ? max_keys : kMsmBasisManySetKeys) / nkeys;
    if (nent && S > kMsmBasisMaxEntries / nent) S = kMsmBasisMaxEntries / nent;
    if (S > 0xffffffffull / words) S = 0xffffffffull / words;
    if (S > m) S = m;
    return S ? S : 1;
}

}  // namespace bn
