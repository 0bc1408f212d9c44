// kernels_products_wide.hip -- k_fq12_products_wide, the per-product reduction of the pairing
// products' wide path (bn_pairing_batch_many, bn_pairing_batch_prepared_many).
// Built as kernels_reduce.hip is: it multiplies with w12_mul only, so four operand arrays per
// group (55.9 KB of LDS per block) and two blocks share a CU.  A unit of its own because the
// out-of-line w12_mul is compiled per unit: a second kernel in kernels_reduce.hip changed the
// operand staging of the w12_mul that k_fq12_reduce_wide calls, and that kernel's code is to
// stay as measured.
#define BN_FOLD_LDS 1
#define BN_WIDE_ARRS 4
#include "fq.h"
#define BN_SPLIT 1
#include "fq12_wide.h"

namespace bn {

// Many small independent products, one 16-lane group each (bn_pairing_batch_many's wide
// path): group g of block b takes product j = 16 b + g and multiplies the
// elements off[j] .. off[j + 1] - 1 of `in` (split layout, stride in_stride, nt elements) in
// one chain, the next factor's load issued before the product that precedes it, and writes
// the value as element j of `out` (stride m).  off: m + 1 device words, non-decreasing from
// 0 to nt; a range is clamped to the nt elements before any address is formed.  An empty
// range gives one; a group with j >= m does nothing.  The groups never meet: no barrier
// after the fold table's, and every guard around w12_mul is uniform per group.
__global__ void __launch_bounds__(kBlock) k_fq12_products_wide(const uint32_t* __restrict__ in, size_t in_stride,
                                                               size_t nt, const uint32_t* __restrict__ off, size_t m,
                                                               uint32_t* __restrict__ out) {
    fold_table_init();
    const WL w = wl();
    const size_t j = (size_t)blockIdx.x * kWGroups + threadIdx.x / kWLanes;
    const bool live = j < m;  // uniform per group
    const size_t bound = nt < in_stride ? nt : in_stride;
    size_t lo = 0, hi = 0;
    if (live) {
        hi = off[j + 1] < bound ? off[j + 1] : bound;
        lo = off[j] < hi ? off[j] : hi;
    }
    const Fq<2> one = fq_select(w.e == 0 && w.c == 0, widen<2>(fq_one()), widen<2>(fq_zero()));
    Fq<2> x = lo < hi ? w_ld_split(in, in_stride, lo, w) : one;
    Fq<2> y = lo + 1 < hi ? w_ld_split(in, in_stride, lo + 1, w) : one;
#pragma unroll 1
    for (size_t t = lo + 1; t < hi; ++t) {  // (the trip count is uniform per group)
        const Fq<2> y_next = t + 1 < hi ? w_ld_split(in, in_stride, t + 1, w) : one;
        x = w12_mul(x, y);
        y = y_next;
    }
    if (live) w_st_split(out, m, j, w, x);
}

}  // namespace bn

BN_EXPORT_FOLD_CHECK(products_wide)
