// mul12_ubench.hip -- the Fq12 product of the final-exponentiation step machine
// with its second operand (a) loaded into registers from a lane-strided HBM
// slot, or (b) copied into LDS by buffer_load ... lds and streamed per Fq2
// (mul12_lds), at one wave per SIMD.  The slot stride is laundered per
// iteration so the loads are not hoisted out of the loop (as in the step
// machine, where every step names different slots).  Both variants must give
// the same values.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/mul12_ubench tools/mul12_ubench.hip
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../paritytech-bn_amd/csrc/kernels.h"

#define CK(x)                                                                                      \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

namespace bn {
// The LDS-operand form of the Fq12 product, measured here and not built into the library
// (one-lane layout: this file includes kernels.h with BN_SPLIT = 0).
// Fq6 product (fq6.rs:197-207, the same Karatsuba as fq6_mul) with operand b
// supplied per Fq2 coordinate by g(j), fetched right before each product that
// needs it (mem_fence keeps the loads from being hoisted), so b never has to be
// held in registers.
template <int A, class G>
__device__ __forceinline__ auto fq6_mul_g(const Fq6<A>& a, G&& g) {
    if constexpr (kv(A) > 20) {
        return fq6_mul_g(fq6_fold(a), g);
    } else {
        mem_fence();
        auto a_a = fq2_mul(a.c0, g(0));
        mem_fence();
        auto b_b = fq2_mul(a.c1, g(1));
        mem_fence();
        auto c_c = fq2_mul(a.c2, g(2));
        mem_fence();
        auto t0 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c1, a.c2), fq2_add(g(1), g(2))), b_b), c_c);
        mem_fence();
        auto t1 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(g(0), g(1))), a_a), b_b);
        mem_fence();
        auto t2 = fq2_sub(fq2_mul(fq2_add(a.c0, a.c2), fq2_add(g(0), g(2))), a_a);
        return mk6(fq2_add(fq2_mul_xi(t0), a_a), fq2_add(t1, fq2_mul_xi(c_c)), fq2_sub(fq2_add(t2, b_b), c_c));
    }
}

// a * b (fq12.rs:319-327 Karatsuba) with b read per Fq2 from `y`, the calling
// lane's strided copy of an Fq12 (word w at y[w * stride]: an LDS image with
// stride kBlock, or a lane-strided HBM slot with stride n); conj_b multiplies
// by conj(b) instead (fq12.rs:126-128).  b is never held in registers whole.
__device__ __forceinline__ Fq12<kF> mul12_strided(const Fq12<kF>& a, const uint32_t* y, size_t stride, bool conj_b) {
    auto ld = [&](int j) {  // Fq2 coordinate j of b (0..2: b.c0, 3..5: b.c1)
        Fq2<kF> r;
#pragma unroll
        for (int l = 0; l < 9; ++l) {
            r.c0.v[l] = y[((2 * j) * 9 + l) * stride];
            r.c1.v[l] = y[((2 * j + 1) * 9 + l) * stride];
        }
        return r;
    };
    auto g0 = [&](int j) { return ld(j); };
    auto g1 = [&](int j) {
        Fq2<kF> r = ld(3 + j);
        if (conj_b) r = fq2_neg(r);
        return r;
    };
    auto gs = [&](int j) { return fq2_add(g0(j), g1(j)); };
    const auto aa = fq6_fold(fq6_mul_g(a.c0, g0));
    const auto s = fq6_add(a.c0, a.c1);
    const auto bb = fq6_fold(fq6_mul_g(a.c1, g1));
    const auto t = fq6_mul_g(s, gs);
    return narrow12<kF>(mk12(fq6_add(fq6_mul_by_nonresidue(bb), aa), fq6_sub(fq6_sub(t, aa), bb)));
}
__device__ __forceinline__ Fq12<kF> mul12_lds(const Fq12<kF>& a, const uint32_t* yl, bool conj_b) {
    return mul12_strided(a, yl, kBlock, conj_b);
}

// Asynchronous copy of a lane-strided Fq12 (108 words, stride n) from global
// memory into the block's LDS image (stride kBlock) with buffer_load ... lds:
// no VGPRs and no vector ALU (SGPR offsets, M0 = the wave's LDS base).  The
// caller waits with lds_copy_wait() before reading.
__device__ __forceinline__ void lds_copy_fq12(const uint32_t* src_block, size_t n, uint32_t* yl_block) {
    // src_block = slot base + blockIdx.x * kBlock; yl_block = LDS image base
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)src_block, 0, 0x7fffffff, 0x00020000);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    const int lane_off = (int)(threadIdx.x & 63u) * 4 + (int)wave * 4;
#pragma unroll
    for (int w = 0; w < kSlotWords; ++w)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void*)(yl_block + w * kBlock + wave), 4, lane_off,
            (int)((size_t)w * n * 4), 0, 0);
}
__device__ __forceinline__ void lds_copy_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int V>
__global__ void __launch_bounds__(kBlock) k_mul(uint32_t* slots, size_t n, int reps) {
    const size_t i = lane_id();
    if (i >= n) return;
    __shared__ uint32_t yl[V == 1 ? kSlotWords * kBlock : 1];
    Fq12<kF> x = ld_fq12<kF>(slots, n, i);
#pragma unroll 1
    for (int r = 0; r < reps; ++r) {
        size_t nn = n;
        asm volatile("" : "+s"(nn));
        const uint32_t* yb = slots + kSlotWords * nn;
        if constexpr (V == 0) {
            x = mul12(x, ld_fq12<kF>(yb, nn, i));
        } else {
            lds_copy_fq12(yb + (size_t)blockIdx.x * kBlock, nn, yl);
            lds_copy_wait();
            mem_fence();
            x = mul12_lds(x, yl + threadIdx.x, false);
        }
    }
    st_fq12(slots + 2 * kSlotWords * n, n, i, x);
}
}  // namespace bn
using namespace bn;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? strtoull(argv[1], 0, 0) : 65536;
    const int reps = 40;
    uint32_t* slots;
    const size_t words = 3 * kSlotWords * n;
    CK(hipMalloc(&slots, words * 4));
    std::vector<uint32_t> h(words), r0(words), r1(words);
    uint64_t s = 0x1234567;
    for (size_t k = 0; k < words; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const size_t digit = (k / n) % 9;
        h[k] = (uint32_t)(s >> 35) & (digit == 8 ? 0x3fffffu : 0x1fffffffu);
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto run = [&](const char* name, void (*k)(uint32_t*, size_t, int), std::vector<uint32_t>& keep) {
        CK(hipMemcpy(slots, h.data(), words * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(kBlock), 0, 0, slots, n, 2);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(slots, h.data(), words * 4, hipMemcpyHostToDevice));
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(kBlock), 0, 0, slots, n, reps);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipMemcpy(keep.data(), slots, words * 4, hipMemcpyDeviceToHost));
        printf("{\"case\": \"%s\", \"n\": %zu, \"ms\": %.4f, \"us_per_mul12\": %.3f}\n", name, n, ms, 1e3 * ms / reps);
    };
    run("mul12, operand in registers", k_mul<0>, r0);
    run("mul12_lds, operand in LDS", k_mul<1>, r1);
    size_t diff = 0;
    for (size_t k = 2 * kSlotWords * n; k < words; ++k) diff += r0[k] != r1[k];
    printf("{\"check\": \"register vs LDS operand\", \"differing_words\": %zu}\n", diff);
    return diff != 0;
}
