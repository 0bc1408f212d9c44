// msm.h -- scalar recoding and bucket keys of the G1 and G2 multi-scalar multiplication
// (kernels_msm.hip, kernels_msm_g2.hip).  Plain integer code over the canonical scalar's eight
// 32-bit words, host and device, so tests/native/msm_emul.cpp compiles it with
// g++ alone.
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

}  // namespace bn
