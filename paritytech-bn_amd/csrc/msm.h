// msm.h -- scalar recoding and bucket keys of the G1 and G2 multi-scalar multiplication
// (kernels_msm.hip, kernels_msm_g2.hip).  Plain integer code over the canonical scalar's eight
// 32-bit words, host and device, so tests/native/msm_emul.cpp compiles it with
// g++ alone; and the plan of the split of overlong bucket runs (run cap, chunk and group
// positions, levels, array bounds), which tests/native/msm_split_emul.cpp compiles the same way.
//
// A canonical scalar k < r < 2^254 becomes W(c) signed digits of c bits,
//     k = sum_w d_w * 2^(c*w),   d_w in [-2^(c-1), 2^(c-1)],
// so a window has 2^(c-1) buckets (|d| = 1 .. 2^(c-1)) and the sign is applied
// to the point.  A raw window value plus the carry from below that exceeds
// 2^(c-1) is replaced by its value minus 2^c and carries one into the next
// window.  W(c) = floor(254 / c) + 1 windows cover c * W(c) >= 255 bits, so the
// top window's raw value is below 2^(c-1) for every k < 2^254 and, with the
// carry, never exceeds 2^(c-1): the top window never carries out.
#pragma once
#include <stdint.h>

#ifndef BN_INLINE
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BN_INLINE __host__ __device__ __forceinline__
#else
#define BN_INLINE inline __attribute__((always_inline))
#endif
#endif

namespace bn {

constexpr int kMsmMinWindow = 2;
constexpr int kMsmMaxWindow = 16;
constexpr int kMsmScalarBits = 254;  // r < 2^254
// the most windows any supported width has (c = 2)
constexpr int kMsmMaxWindows = kMsmScalarBits / kMsmMinWindow + 1;
// buckets per lane of the bucket reduction: a lane's dependent chain is
// 2 * kMsmSegment + 2 * (c - 1) + 1 group operations
constexpr uint32_t kMsmSegment = 16;

BN_INLINE bool msm_window_ok(int c) { return c >= kMsmMinWindow && c <= kMsmMaxWindow; }
// W(c)
BN_INLINE int msm_windows(int c) { return kMsmScalarBits / c + 1; }
// buckets per window
BN_INLINE uint32_t msm_buckets(int c) { return 1u << (c - 1); }

// bits [c*w, c*w + c) of k (bits at and above 256 read as zero)
BN_INLINE uint32_t msm_raw_window(const uint32_t k[8], int c, int w) {
    const int lo = c * w;
    const int word = lo >> 5, sh = lo & 31;
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // no dynamic index into k: it stays in registers
        if (j == word) v |= (uint64_t)k[j];
        if (j == word + 1) v |= (uint64_t)k[j] << 32;
    }
    return (uint32_t)(v >> sh) & ((1u << c) - 1u);
}
// one step of the signed recoding: the digit of a raw window value given the
// carry from the window below; *carry becomes the carry into the window above
BN_INLINE int32_t msm_signed_digit(uint32_t raw, int c, uint32_t* carry) {
    const uint32_t v = raw + *carry;  // <= 2^c
    const bool high = v > (1u << (c - 1));
    *carry = high ? 1u : 0u;
    return high ? (int32_t)v - (int32_t)(1u << c) : (int32_t)v;
}
// all W(c) digits of k; returns the carry out of the top window (0 for k < 2^254)
BN_INLINE uint32_t msm_recode(const uint32_t k[8], int c, int32_t* digits) {
    uint32_t carry = 0;
    const int nw = msm_windows(c);
    for (int w = 0; w < nw; ++w) digits[w] = msm_signed_digit(msm_raw_window(k, c, w), c, &carry);
    return carry;
}

// The top window holds only t(c) = 254 - c * (W(c) - 1) scalar bits (0 <= t <= c - 1), so
// its digits are 0 .. 2^t, never negative: with one bucket per digit a few buckets would
// each take n / 2^t terms, a dependent chain of that length on one lane.  Its 2^(c-1)
// bucket slots are used instead as 2^t digits x 2^(c-1-t) replicas, the replica chosen by
// the low bits of the term's index, so its entries spread as evenly as any other
// window's.  Every other window has one replica.
BN_INLINE int msm_top_bits(int c) { return kMsmScalarBits - c * (msm_windows(c) - 1); }
// log2 of the replicas per digit in window w
BN_INLINE int msm_replica_shift(int c, int w) { return w == msm_windows(c) - 1 ? (c - 1) - msm_top_bits(c) : 0; }
// (window, bucket) key of term `index`'s nonzero digit d in window w: window-major,
// bucket ((|d| - 1) << replica shift) | replica
BN_INLINE uint32_t msm_key(int c, int w, int32_t d, uint32_t index) {
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    const int rs = msm_replica_shift(c, w);
    return (uint32_t)w * msm_buckets(c) + (((mag - 1u) << rs) | (index & ((1u << rs) - 1u)));
}
BN_INLINE int msm_key_window(int c, uint32_t key) { return (int)(key >> (c - 1)); }
// the weight |d| of the key's bucket
BN_INLINE uint32_t msm_key_weight(int c, uint32_t key) {
    return ((key & (msm_buckets(c) - 1u)) >> msm_replica_shift(c, msm_key_window(c, key))) + 1u;
}
// number of keys
BN_INLINE uint32_t msm_num_keys(int c) { return (uint32_t)msm_windows(c) * msm_buckets(c); }

// a sorted entry: the term's index with the digit's sign in bit 31 (n <= 2^26)
constexpr uint32_t kMsmNegBit = 0x80000000u;
BN_INLINE uint32_t msm_entry(uint32_t index, int32_t d) { return index | (d < 0 ? kMsmNegBit : 0u); }
BN_INLINE uint32_t msm_entry_index(uint32_t e) { return e & ~kMsmNegBit; }
BN_INLINE bool msm_entry_neg(uint32_t e) { return (e & kMsmNegBit) != 0; }

// ---------------------------------------------------------------- overlong runs
// A key whose run has more than L entries (the run cap) is long.  One lane per key would walk
// its run as one chain of dependent additions, so a long run is cut into chunks of at most L
// entries, one lane each (level 0), and the chunk sums are folded by a tree of fan-in
// kMsmFoldFan, one lane per group of consecutive partial sums of one key (levels 1, 2, ..);
// the level at which a key is down to one group writes its bucket.  Positions are arithmetic
// on the key's offset o in the sorted entries and its rank r among the long keys (in key
// order), so one scan of the histogram is all the device needs:
//     start_0 = floor(o / L) + r,            m_0 = ceil(cnt / L)   chunks
//     start_k = floor(start_{k-1} / F) + r,  m_k = ceil(m_{k-1} / F) groups.
// The ranges [start_k, start_k + m_k) of the long keys are disjoint and increasing in r at
// every level: for the next long key, o' >= o + cnt and r' = r + 1, and
// floor(a + b) + 1 >= floor(a) + ceil(b).  The critical path of a bucket is at most
// L + F * levels additions.
constexpr uint32_t kMsmFoldFan = 32;
// the default cap is max(kMsmRunMin, 2 * ceil(n / 2^(c-1))): twice the mean run of uniform
// scalars, so that they essentially never split
constexpr uint32_t kMsmRunMin = 128;
constexpr uint32_t kMsmRunMax = 1u << 16;         // the largest cap that can be set
constexpr uint32_t kMsmRunUnsplit = 0xffffffffu;  // no key is long
// the fold levels of 2^26 terms at L = 1
constexpr int kMsmMaxFoldLevels = 6;

BN_INLINE uint32_t msm_ceil_div(uint32_t a, uint32_t b) { return a / b + (a % b != 0 ? 1u : 0u); }
BN_INLINE uint32_t msm_run_cap_default(uint32_t n, int c) {
    const uint32_t twice = 2u * msm_ceil_div(n, msm_buckets(c));
    return twice > kMsmRunMin ? twice : kMsmRunMin;
}
// The fold levels a call of n terms launches: a run has at most n entries (one per term), so
// at most ceil(n / L) chunks.  0: no key can be long.
BN_INLINE int msm_fold_levels(uint32_t n, uint32_t L) {
    if (L == kMsmRunUnsplit || n <= L) return 0;
    int levels = 0;
    for (uint32_t m = msm_ceil_div(n, L); m > 1; m = msm_ceil_div(m, kMsmFoldFan)) ++levels;
    return levels;
}
// the first slot and the number of slots of a long key at a level (0: its chunks)
struct MsmRunPos {
    uint32_t start, m;
};
BN_INLINE uint32_t msm_run_start(uint32_t o, uint32_t r, uint32_t L, int level) {
    uint32_t start = o / L + r;
    for (int k = 0; k < level; ++k) start = start / kMsmFoldFan + r;
    return start;
}
BN_INLINE MsmRunPos msm_run_pos(uint32_t o, uint32_t cnt, uint32_t r, uint32_t L, int level) {
    uint32_t m = msm_ceil_div(cnt, L);
    for (int k = 0; k < level; ++k) m = msm_ceil_div(m, kMsmFoldFan);
    return {msm_run_start(o, r, L, level), m};
}
// the most long keys among nent entries over nkeys keys: each has more than L entries
BN_INLINE uint32_t msm_long_keys_bound(uint32_t nent, uint32_t nkeys, uint32_t L) {
    const uint32_t by_count = nent / (L + 1u);
    return by_count < nkeys ? by_count : nkeys;
}
// The slots of a level, an upper bound from what the host knows: every start + m is at most
// floor(end_{k-1} / F) + 1 + r with end_{k-1} the level below's bound (nent entries at level
// 0), so level 0 has at most floor(nent / L) + (long keys) slots -- at most 2 * nent / L --
// and every further level 1 / F of the level below plus the long keys.
BN_INLINE uint32_t msm_level_slots(uint32_t nent, uint32_t nkeys, uint32_t L, int level) {
    const uint32_t nl = msm_long_keys_bound(nent, nkeys, L);
    uint32_t s = nent / L + nl;
    for (int k = 0; k < level; ++k) s = s / kMsmFoldFan + nl;
    return s;
}
// The long key whose slots at `level` hold slot t: the largest rank r < nlong with
// start(r) <= t (start is increasing in r), or nlong if there is none.  start(r) reads the
// key's offset through the caller's functor.
template <class Offset>
BN_INLINE uint32_t msm_find_long(Offset&& offset_of_rank, uint32_t nlong, uint32_t t, uint32_t L, int level) {
    uint32_t lo = 0, hi = nlong;  // ranks below lo start at or before t, ranks from hi on after it
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (msm_run_start(offset_of_rank(mid), mid, L, level) <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo == 0 ? nlong : lo - 1;
}
// What the lane of slot t does at a level.  Level 0: the sum of the entries sorted[lo .. hi)
// of `key`, into slot t of level 0.  Level k >= 1: the sum of the slots [lo, hi) of level
// k - 1, into the key's bucket (last: the key is down to one group) or into slot t of level
// k.  !some: nothing (no key holds the slot, or the key finished at a level below).  Every
// index is bounded here: the rank against nlong <= nkeys, the key against nkeys, the run
// against nent; the caller bounds the slots against its arrays.  longkeys[0 .. nlong): the
// long keys in key order; offsets[0 .. nkeys]: the scan.
struct MsmRunTask {
    bool some, last;
    uint32_t key, lo, hi;
};
BN_INLINE MsmRunTask msm_run_task(const uint32_t* longkeys, const uint32_t* offsets, uint32_t nlong, uint32_t nkeys,
                                  uint32_t nent, uint32_t L, int level, uint32_t t) {
    const MsmRunTask none = {false, false, 0, 0, 0};
    if (nlong > nkeys) nlong = nkeys;
    if (nlong == 0 || L == 0) return none;
    auto offset_of_rank = [&](uint32_t r) {
        const uint32_t key = longkeys[r];
        return key < nkeys ? offsets[key] : nent;
    };
    const uint32_t r = msm_find_long(offset_of_rank, nlong, t, L, level);
    if (r >= nlong) return none;
    const uint32_t key = longkeys[r];
    if (key >= nkeys) return none;
    uint32_t e = offsets[key + 1];
    e = e < nent ? e : nent;
    uint32_t o = offsets[key];
    o = o < e ? o : e;
    const uint32_t cnt = e - o;
    if (cnt <= L) return none;
    const MsmRunPos pos = msm_run_pos(o, cnt, r, L, level);
    if (t < pos.start || t - pos.start >= pos.m) return none;
    const uint32_t j = t - pos.start;
    if (level == 0) {
        const uint32_t lo = o + j * L;  // j < ceil(cnt / L): below e
        return {true, false, key, lo, e - lo < L ? e : lo + L};
    }
    const MsmRunPos prev = msm_run_pos(o, cnt, r, L, level - 1);
    if (prev.m <= 1) return none;  // finished below
    const uint32_t lo = prev.start + j * kMsmFoldFan, end = prev.start + prev.m;
    return {true, pos.m == 1, key, lo, end - lo < kMsmFoldFan ? end : lo + kMsmFoldFan};
}

}  // namespace bn
