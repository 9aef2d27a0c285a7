// Device helpers shared by the matrix-core kernels (fused convolution K loops, weight gradient): vector types,
// LDS-DMA copies and the explicit LDS-read / counted-wait idiom.  Everything is __forceinline__.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace mpg::dev {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// LDS reads in the K loops use clang vector types only: a read through HIP's struct `int4` makes the compiler put an
// `s_waitcnt vmcnt(0)` in front of it while LDS-DMA pieces are in flight (it cannot tell the read from the DMA's
// destination), which serialises every stage behind its own weight / image DMAs; ext_vector_type reads do not.
typedef int v4i __attribute__((ext_vector_type(4)));

// at most N LDS-DMA (vector memory) operations of this wave still in flight, every LDS read done, then the barrier
template <int N>
__device__ __forceinline__ void wait_dma_and_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
// ... with `extra` (0..7, wave-uniform) more of the newest operations allowed in flight
__device__ __forceinline__ void wait_dma_rt(int base, int extra) {
    switch (base + extra) {
#define MPG_W(n) case n: wait_dma_and_barrier<n>(); break;
        MPG_W(0) MPG_W(1) MPG_W(2) MPG_W(3) MPG_W(4) MPG_W(5) MPG_W(6) MPG_W(7) MPG_W(8) MPG_W(9) MPG_W(10) MPG_W(11)
        MPG_W(12) MPG_W(13) MPG_W(14) MPG_W(15)
#undef MPG_W
        default: wait_dma_and_barrier<0>(); break;
    }
}

__device__ __forceinline__ void dma16(const char* src, char* lds_wave_base) {
    // lane l of the wave copies 16 bytes from its own `src` to lds_wave_base + 16*l
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ void dma16_stream(const char* src, char* lds_wave_base) {
    // same, with the non-temporal hint: activation tiles are read once or twice and should not push the weights
    // (re-read by every tile) out of L2
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 2);
}

// f(integral_constant<int, I>) for I .. N - 1, unrolled at compile time
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
// LDS byte address of p, for reads written as volatile asm: they stay in program order, which is what the counted waits
// count
__device__ __forceinline__ unsigned lds_off(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}
// wait until at most N of the LDS reads issued so far are outstanding (they return in order)
template <int N>
__device__ __forceinline__ void lgkm_wait() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N < 15 ? N : 15) : "memory");
}
// no instruction: makes every later use of `frag` depend on the preceding (volatile) wait
template <class T>
__device__ __forceinline__ void tie(T& frag) {
    asm volatile("" : "+v"(frag));
}

}  // namespace mpg::dev
