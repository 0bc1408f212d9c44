// kernels_msm_fixed.hip -- G1 multi-scalar multiplications over prepared bases
// (bn_g1_bases_prepare, bn_g1_msm_prepared_many; the bodies are
// msm_fixed.h's).  The phases pass data only across kernel boundaries on one stream (no
// block waits for another):
//   k_g1_table_build      once per handle, one lane per (base, window): its 2^(c-1) entries
//   k_g1_msm_fixed        L lanes per output: a lane's share of the table lookups, summed
//   (k_g1_op add)         halving tree over the L partial sums of every output (capi_msm.hip)
//   k_g1_msm_fixed_finish one lane per output: the returned image, stored at its stride
// Every computed index is bounded against its array in the kernel; a lane whose index is
// out of range does nothing.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "kernels.h"
#include "msm_fixed.h"

namespace bn {

// ---------------------------------------------------------------- table build
// Lane t = b * W(c) + w builds entries (b, w, 0 .. 2^(c-1)) as reference images (x, y); the
// lane of window 0 writes the base's zero flag.  A zero base's entries are written as
// zeros: the lookup's idle fetches read entry 0, so every entry holds a field element.
__global__ void __launch_bounds__(kBlock) k_g1_table_build(const bn_g1* __restrict__ bases, uint32_t k, int c,
                                                           bn_fq* __restrict__ table, uint8_t* __restrict__ zero,
                                                           uint32_t nent) {
    fold_table_init();
    const size_t t = lane_id();
    const uint32_t nwin = (uint32_t)msm_windows(c);
    if (t >= (size_t)k * nwin) return;
    const uint32_t b = (uint32_t)(t / nwin), w = (uint32_t)(t % nwin);
    const G1J base = ld_g1(bases[b]);
    const bool bzero = jac_is_zero(base);
    if (w == 0) zero[b] = bzero ? 1 : 0;
    const uint32_t first = msm_fixed_index(c, nwin, b, w, 1);
    if (bzero) {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t j = 0; j < msm_buckets(c); ++j)
            if (first + j < nent) {
                st_words(&table[2 * (size_t)(first + j)], z);
                st_words(&table[2 * (size_t)(first + j) + 1], z);
            }
        return;
    }
    msm_fixed_build<Fq>(base, c, (int)w, first, nent, [&](uint32_t idx, const Fq<kPt>& x, const Fq<kPt>& y) {
        st_ref(table[2 * (size_t)idx], x);
        st_ref(table[2 * (size_t)idx + 1], y);
    });
}

// ---------------------------------------------------------------- table lookups
// Thread t of m * L: output j = t % m, lane l = t / m of its L, so the lanes of a wave share
// l (but for the one wave that crosses a multiple of m): they walk the same (base, window)
// pairs, read their scalars and their entries at the same step, and a step's entries come
// from one window's 2^(c-1) * 64 bytes.  parts[l * m + j] = the lane's Jacobian partial sum:
// the tree over l adds contiguous halves.
struct FixedRaw {
    uint4 q[4];
};
__global__ void __launch_bounds__(kBlock) k_g1_msm_fixed(const bn_fq* __restrict__ table,
                                                         const uint8_t* __restrict__ zero, uint32_t nent, uint32_t k,
                                                         int c, const bn_fr* __restrict__ scalars, size_t m, uint32_t L,
                                                         bn_g1* __restrict__ parts) {
    fold_table_init();
    const size_t t = lane_id();
    if (t >= m * L) return;
    const size_t j = t % m;
    const uint32_t l = (uint32_t)(t / m);
    const bn_fr* row = scalars + j * k;
    const G1J acc = msm_fixed_lane_sum<Fq>(
        [&](uint32_t b, uint32_t* s) { fr_to_canonical(row[b < k ? b : 0], s); },
        [&](uint32_t b) { return b >= k || zero[b] != 0; },
        [&](uint32_t idx) {
            const uint4* e = reinterpret_cast<const uint4*>(table + 2 * (size_t)(idx < nent ? idx : 0));
            return FixedRaw{{e[0], e[1], e[2], e[3]}};
        },
        [](const FixedRaw& e, Fq<2>& x, Fq<2>& y) {
            const uint32_t wx[8] = {e.q[0].x, e.q[0].y, e.q[0].z, e.q[0].w, e.q[1].x, e.q[1].y, e.q[1].z, e.q[1].w};
            const uint32_t wy[8] = {e.q[2].x, e.q[2].y, e.q[2].z, e.q[2].w, e.q[3].x, e.q[3].y, e.q[3].z, e.q[3].w};
            x = fq_load_ref(wx);
            y = fq_load_ref(wy);
        },
        k, c, nent, l, L);
    st_g1(parts[(size_t)l * m + j], acc);
}

// ---------------------------------------------------------------- finish
// out[j * stride] = the returned image of sums[j] (msm_finish_point), j < m; nothing between
// the strided outputs is written
__global__ void __launch_bounds__(kBlock) k_g1_msm_fixed_finish(const bn_g1* __restrict__ sums, size_t m,
                                                                bn_g1* __restrict__ out, size_t stride) {
    fold_table_init();
    const size_t j = lane_id();
    if (j >= m) return;
    st_g1(out[j * stride], msm_finish_point(ld_g1(sums[j])));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_fixed)
