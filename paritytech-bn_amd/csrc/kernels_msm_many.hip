// kernels_msm_many.hip -- many small G1 multi-scalar multiplications over fresh bases in one
// launch set (bn_g1_msm_many; the bodies are msm_many.h's).  The phases pass
// data only across kernel boundaries on one stream (no block waits for another):
//   k_g1_msm_many_table   one lane per term: its W(c) digit bytes and its 2^(c-1) multiples
//   k_g1_msm_many_unit    one lane per unit (a run of terms of one segment): shared
//                         doublings, one signed table entry added per term and window
//   k_g1_msm_many_finish  one lane per segment: the sum of its units' partials, the returned
//                         image stored at its stride
// Every computed index is bounded against its array in the kernel; a lane whose index is
// out of range does nothing.
#ifndef BN_FOLD_LDS
#define BN_FOLD_LDS 1
#endif
#include "kernels.h"
#include "msm_many.h"

namespace bn {

// ---------------------------------------------------------------- digits and multiples
// Lane t: term t of the set's nt.  digits: W(c) * nt bytes; table: nt << (c - 1) points.
__global__ void __launch_bounds__(kBlock) k_g1_msm_many_table(const bn_g1* __restrict__ p, const bn_fr* __restrict__ k,
                                                              uint32_t nt, int c, uint8_t* __restrict__ digits,
                                                              bn_g1* __restrict__ table) {
    fold_table_init();
    const size_t t = lane_id();
    if (t >= nt || !msm_many_window_ok(c)) return;
    uint32_t s[8];
    fr_to_canonical(k[t], s);
    msm_many_term<Fq>(
        ld_g1(p[t]), s, c, (uint32_t)t, nt, msm_many_digits(nt, c), msm_many_entries(nt, c),
        [&](uint64_t i, uint8_t b) { digits[i] = b; }, [&](uint64_t i, const G1J& e) { st_g1(table[i], e); });
}

// ---------------------------------------------------------------- units
// Lane u of nunits: the terms unit_off[u] .. unit_off[u + 1] - 1 of the set (the plan's words,
// bounded here against nt and the 64 terms of a unit).  parts[u] = the Jacobian partial sum.
struct ManyRaw {
    uint4 q[6];
};
__global__ void __launch_bounds__(kBlock) k_g1_msm_many_unit(const uint8_t* __restrict__ digits,
                                                             const bn_g1* __restrict__ table, uint32_t nt, int c,
                                                             const uint32_t* __restrict__ unit_off, uint32_t nunits,
                                                             bn_g1* __restrict__ parts) {
    fold_table_init();
    const size_t u = lane_id();
    if (u >= nunits || !msm_many_window_ok(c) || nt == 0) return;
    uint32_t t1 = unit_off[u + 1];
    t1 = t1 < nt ? t1 : nt;
    uint32_t t0 = unit_off[u];
    t0 = t0 < t1 ? t0 : t1;
    uint32_t cnt = t1 - t0;
    cnt = cnt < 64u ? cnt : 64u;
    const G1J acc = msm_many_unit_sum<Fq>(
        [&](uint64_t i) { return digits[i]; },
        [&](uint64_t i) {
            const uint4* e = reinterpret_cast<const uint4*>(table + i);
            return ManyRaw{{e[0], e[1], e[2], e[3], e[4], e[5]}};
        },
        [](const ManyRaw& e) {
            const uint32_t wx[8] = {e.q[0].x, e.q[0].y, e.q[0].z, e.q[0].w, e.q[1].x, e.q[1].y, e.q[1].z, e.q[1].w};
            const uint32_t wy[8] = {e.q[2].x, e.q[2].y, e.q[2].z, e.q[2].w, e.q[3].x, e.q[3].y, e.q[3].z, e.q[3].w};
            const uint32_t wz[8] = {e.q[4].x, e.q[4].y, e.q[4].z, e.q[4].w, e.q[5].x, e.q[5].y, e.q[5].z, e.q[5].w};
            return G1J{widen<kPt>(fq_load_ref(wx)), widen<kPt>(fq_load_ref(wy)), widen<kPt>(fq_load_ref(wz))};
        },
        c, t0, cnt, nt, msm_many_digits(nt, c), msm_many_entries(nt, c));
    st_g1(parts[u], acc);
}

// ---------------------------------------------------------------- finish
// Lane j of m: out[j * stride] = the returned image of the sum of parts[seg_unit[j] ..
// seg_unit[j + 1]) (bounded against nunits and the 64 units of a segment); nothing between
// the strided outputs is written
__global__ void __launch_bounds__(kBlock) k_g1_msm_many_finish(const bn_g1* __restrict__ parts, uint32_t nunits,
                                                               const uint32_t* __restrict__ seg_unit, size_t m,
                                                               bn_g1* __restrict__ out, size_t stride) {
    fold_table_init();
    const size_t j = lane_id();
    if (j >= m) return;
    uint32_t u1 = seg_unit[j + 1];
    u1 = u1 < nunits ? u1 : nunits;
    uint32_t u0 = seg_unit[j];
    u0 = u0 < u1 ? u0 : u1;
    u1 = u1 - u0 < 64u ? u1 : u0 + 64u;
    st_g1(out[j * stride], msm_many_segment<Fq>([&](uint32_t u) { return ld_g1(parts[u]); }, u0, u1));
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(msm_many)
