// tail_epoch.h -- the arithmetic of bn_ctx.tail_epoch, the counter that stamps every word
// k_seg_tail and k_fe_ds poll (kernels_tail.hip; DESIGN.md §4.10, "the whole tail in one
// launch").  Pure: the standard integer types only, so it runs (and is tested, tests/native/
// tail_epoch_main.cpp) without a GPU.
#pragma once
#include <stdint.h>

#pragma GCC visibility push(hidden)  // nothing here is part of the library's interface
namespace bn {

// The last epoch before the counter returns to 1: the role word holds epoch * 8 + three
// bits (kernels_tail.hip tail_bits), so epoch * 8 must fit 32 bits.
constexpr uint32_t kTailEpochWrapDefault = (1u << 29) - 1;
// the wraps $BN254MI_TAIL_EPOCH_WRAP may ask for (a wrap of 1 would stamp every launch alike)
constexpr bool tail_epoch_wrap_ok(unsigned long long v) { return v >= 2 && v <= kTailEpochWrapDefault; }

struct TailEpochStep {
    uint32_t epoch;  // the next launch's stamp: 1 .. wrap, never 0 (the buffers are created zeroed)
    bool clear;      // the counter came back to 1: words stamped in the last cycle must go first
};
// The epochs run 1, 2, ..., wrap, 1, 2, ...; a fresh context (current == 0) starts at 1 over
// buffers that hold no stamp yet.  The kernels do not rewrite every word on every launch
// (k_fe_ds touches pair i's words only when n > i and its channel only with three blocks
// per pair; k_seg_tail writes the links of its plan's S segments), so a word stamped e may
// still be there when the counter returns to e, one cycle later, and would then count as
// published: the caller zeroes both buffers in front of the launch that gets epoch 1 again.
inline TailEpochStep tail_epoch_next(uint32_t current, uint32_t wrap) {
    if (current == 0) return {1u, false};
    if (current < wrap) return {current + 1, false};
    return {1u, true};
}

}  // namespace bn
#pragma GCC visibility pop
