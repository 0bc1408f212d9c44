// msm_sort.h -- the device bodies the recoding kernels of kernels_msm.hip and of
// kernels_msm_basis_many.hip share: the wave-aggregated claim of a position in a key's run,
// and the one-block scan of a histogram.  Device code only.
#pragma once
#include "kernels.h"
#include "msm.h"

namespace bn {

// The lanes of a wave that hold the same key share one atomic: skewed scalars (all equal, a
// witness of zeros and ones) send most of a wave to one address, and 2^18 x W(c) atomics on
// one address per hot key took 4.2 ms (count) and 8.6 ms (scatter) of an all-equal batch whose
// group-law kernels took 2 ms.  kMsmAggRounds times: the first lane not yet
// served names its key, the lanes with that key (a ballot) take consecutive positions from
// one atomicAdd of their count by that lane; whoever is left adds alone.  Two rounds find a
// key that half the wave holds with probability 3/4 and cost uniform scalars two ballots and
// two broadcasts per round.  Returns the value of counts[key] before this lane's own
// increment; every lane of the wave that has not returned calls it together (`has`: with a key).
constexpr int kMsmAggRounds = 2;
__device__ __forceinline__ uint32_t msm_claim(uint32_t* __restrict__ counts, uint32_t key, bool has) {
    const uint32_t lane = __lane_id();
    uint32_t pos = 0;
    bool done = !has;
#pragma unroll
    for (int round = 0; round < kMsmAggRounds; ++round) {
        const uint64_t rem = __ballot(!done);
        if (rem == 0) break;  // wave-uniform
        const int leader = __ffsll((long long)rem) - 1;
        const uint32_t lkey = __shfl(key, leader);
        const bool mine = !done && key == lkey;
        const uint64_t grp = __ballot(mine);
        uint32_t base = 0;
        if (mine && lane == (uint32_t)leader) base = atomicAdd(&counts[key], (uint32_t)__popcll(grp));
        base = __shfl(base, leader);
        if (mine) {
            pos = base + (uint32_t)__popcll(grp & ((1ull << lane) - 1ull));
            done = true;
        }
    }
    if (!done) pos = atomicAdd(&counts[key], 1u);
    return pos;
}

// One block of kMsmScanBlock threads: offsets[0 .. nkeys] = exclusive scan of
// counts[0 .. nkeys), cursors[key] = offsets[key]; longinfo[0] = the number of keys with more
// than L entries, longinfo[1 ..] those keys in key order (at most nkeys; none at
// L = kMsmRunUnsplit).  Each thread scans a contiguous piece, the piece totals (entries in
// the low half, long keys in the high half of one 64-bit word: the entries stay below 2^31) go
// through LDS.
__device__ __forceinline__ void msm_scan_block(const uint32_t* __restrict__ counts, uint32_t nkeys,
                                               uint32_t* __restrict__ offsets, uint32_t* __restrict__ cursors,
                                               uint32_t L, uint32_t* __restrict__ longinfo) {
    __shared__ uint64_t tot[kMsmScanBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nkeys + kMsmScanBlock - 1) / kMsmScanBlock;
    const uint32_t lo = t * per < nkeys ? t * per : nkeys;
    const uint32_t hi = lo + per < nkeys ? lo + per : nkeys;
    uint64_t sum = 0;
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t cnt = counts[j];
        sum += (uint64_t)cnt + ((uint64_t)(cnt > L ? 1u : 0u) << 32);
    }
    tot[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < kMsmScanBlock; d <<= 1) {  // inclusive scan of the piece totals
        const uint64_t v = t >= d ? tot[t - d] : 0u;
        __syncthreads();
        tot[t] += v;
        __syncthreads();
    }
    const uint64_t before = tot[t] - sum;
    uint32_t run = (uint32_t)before, rank = (uint32_t)(before >> 32);
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t cnt = counts[j];
        offsets[j] = run;
        cursors[j] = run;
        run += cnt;
        if (cnt > L) {
            if (rank < nkeys) longinfo[1 + rank] = j;
            ++rank;
        }
    }
    if (t == kMsmScanBlock - 1) {
        offsets[nkeys] = (uint32_t)tot[t];
        longinfo[0] = (uint32_t)(tot[t] >> 32);
    }
}

}  // namespace bn
