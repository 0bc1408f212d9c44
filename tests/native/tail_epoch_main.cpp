// tail_epoch_main.cpp -- stand-alone checks of csrc/tail_epoch.h (the counter that stamps
// the words k_seg_tail and k_fe_ds poll, and when its buffers are due a clear), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_tail_epoch.py.  Prints
// "tail epoch ok" when every check holds.
#include "../../paritytech-bn_amd/csrc/tail_epoch.h"

#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

using namespace bn;

#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                \
        }                                                           \
    } while (0)

// `cycles` full cycles and a launch more from a fresh context: the epochs are 1, 2, ...,
// wrap, 1, ...; never 0, never above the wrap; the clear is flagged on every return to 1
// and nowhere else; the first epoch is 1 with no clear
static void run_cycles(uint32_t wrap, int cycles) {
    uint32_t cur = 0, want = 1;  // want: position t of 1, 2, ..., wrap, 1, ...
    uint64_t clears = 0;
    const uint64_t launches = (uint64_t)wrap * (uint64_t)cycles + 1;
    for (uint64_t t = 0; t < launches; ++t) {
        const TailEpochStep st = tail_epoch_next(cur, wrap);
        CHECK(st.epoch >= 1 && st.epoch <= wrap);
        CHECK(st.epoch == want);
        CHECK(st.clear == (t > 0 && st.epoch == 1));
        CHECK(st.epoch <= (0xffffffffu - 7u) / 8u);  // the role word: epoch * 8 + three bits
        clears += st.clear ? 1 : 0;
        cur = st.epoch;
        want = want == wrap ? 1 : want + 1;
    }
    CHECK(clears == (uint64_t)cycles && cur == 1);
    CHECK(tail_epoch_next(0, wrap).epoch == 1 && !tail_epoch_next(0, wrap).clear);
}

// the default wrap without 3 * 2^29 steps: the counter's every value near both ends of a
// cycle, entered directly, three cycles over
static void run_default_ends() {
    const uint32_t wrap = kTailEpochWrapDefault;
    CHECK(wrap == (1u << 29) - 1);
    CHECK(tail_epoch_next(0, wrap).epoch == 1 && !tail_epoch_next(0, wrap).clear);
    for (int cycle = 0; cycle < 3; ++cycle) {
        uint32_t cur = cycle == 0 ? 0 : wrap - 1000;
        for (int t = 0; t < 2000; ++t) {
            const TailEpochStep st = tail_epoch_next(cur, wrap);
            // the rule the launch sites used before the helper: epoch + 1 < 2^29 ? epoch + 1 : 1
            CHECK(st.epoch == (cur + 1 < (1u << 29) ? cur + 1 : 1u));
            CHECK(st.clear == (cur == wrap));
            CHECK(st.epoch >= 1 && st.epoch <= wrap);
            cur = st.epoch;
        }
        CHECK(cur == (cycle == 0 ? 2000u : 1000u));
    }
    // the last values of the cycle one by one
    CHECK(tail_epoch_next(wrap - 2, wrap).epoch == wrap - 1 && !tail_epoch_next(wrap - 2, wrap).clear);
    CHECK(tail_epoch_next(wrap - 1, wrap).epoch == wrap && !tail_epoch_next(wrap - 1, wrap).clear);
    CHECK(tail_epoch_next(wrap, wrap).epoch == 1 && tail_epoch_next(wrap, wrap).clear);
}

static void run_override_range() {
    CHECK(!tail_epoch_wrap_ok(0) && !tail_epoch_wrap_ok(1) && tail_epoch_wrap_ok(2) && tail_epoch_wrap_ok(3));
    CHECK(tail_epoch_wrap_ok((1ull << 29) - 1) && !tail_epoch_wrap_ok(1ull << 29) && !tail_epoch_wrap_ok(~0ull));
    // a counter above a lowered wrap (not reachable: the wrap is fixed at creation) still
    // comes back to 1 with a clear instead of running on
    CHECK(tail_epoch_next(9, 3).epoch == 1 && tail_epoch_next(9, 3).clear);
}

int main() {
    for (uint32_t wrap : {2u, 3u, 7u}) run_cycles(wrap, 5);
    run_cycles(kTailEpochWrapDefault, 3);  // 1.6e9 steps of a few instructions: seconds
    run_default_ends();
    run_override_range();
    printf("tail epoch ok\n");
    return 0;
}
