// msm_emul.cpp -- the MSM scalar recoding and bucket keys of csrc/msm.h compiled
// for the host (TEST INFRASTRUCTURE ONLY; tests/test_msm_recode.py).
#include "../../paritytech-bn_amd/csrc/msm.h"

extern "C" {

int msm_emul_min_window() { return bn::kMsmMinWindow; }
int msm_emul_max_window() { return bn::kMsmMaxWindow; }
int msm_emul_max_windows() { return bn::kMsmMaxWindows; }
int msm_emul_window_ok(int c) { return bn::msm_window_ok(c) ? 1 : 0; }
int msm_emul_windows(int c) { return bn::msm_windows(c); }
unsigned msm_emul_buckets(int c) { return bn::msm_buckets(c); }
unsigned msm_emul_num_keys(int c) { return bn::msm_num_keys(c); }
// digits[0 .. W(c)) of each of the n scalars (8 words each); returns the OR of the carries out
unsigned msm_emul_recode_many(const uint32_t* k, int n, int c, int32_t* digits) {
    unsigned carry = 0;
    const int nw = bn::msm_windows(c);
    for (int i = 0; i < n; ++i) carry |= bn::msm_recode(k + 8 * i, c, digits + (long)i * nw);
    return carry;
}
unsigned msm_emul_key(int c, int w, int d, unsigned index) { return bn::msm_key(c, w, d, index); }
int msm_emul_top_bits(int c) { return bn::msm_top_bits(c); }
int msm_emul_replica_shift(int c, int w) { return bn::msm_replica_shift(c, w); }
int msm_emul_key_window(int c, unsigned key) { return bn::msm_key_window(c, key); }
unsigned msm_emul_key_weight(int c, unsigned key) { return bn::msm_key_weight(c, key); }
unsigned msm_emul_entry(unsigned index, int d) { return bn::msm_entry(index, d); }
unsigned msm_emul_entry_index(unsigned e) { return bn::msm_entry_index(e); }
int msm_emul_entry_neg(unsigned e) { return bn::msm_entry_neg(e) ? 1 : 0; }

}  // extern "C"
