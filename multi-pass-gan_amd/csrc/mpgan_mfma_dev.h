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
// at most `late` (0..4, wave-uniform) of the newest LDS-DMA operations still in flight, every LDS read done, then the
// barrier -- as ONE asm statement: the compiler sees no branch, so a K loop with several hundred live registers keeps
// one register allocation around it (a `switch` in a stage body splits the allocation at every stage and spills)
__device__ __forceinline__ void wait_dma_late_and_barrier(int late) {
    asm volatile(
        "s_cmp_lt_u32 %0, 1\n\t"
        "s_cbranch_scc1 .Lmpg_w0_%=\n\t"
        "s_cmp_lt_u32 %0, 2\n\t"
        "s_cbranch_scc1 .Lmpg_w1_%=\n\t"
        "s_cmp_lt_u32 %0, 3\n\t"
        "s_cbranch_scc1 .Lmpg_w2_%=\n\t"
        "s_cmp_lt_u32 %0, 4\n\t"
        "s_cbranch_scc1 .Lmpg_w3_%=\n\t"
        "s_waitcnt vmcnt(4)\n\t"
        "s_branch .Lmpg_wb_%=\n"
        ".Lmpg_w3_%=:\n\t"
        "s_waitcnt vmcnt(3)\n\t"
        "s_branch .Lmpg_wb_%=\n"
        ".Lmpg_w2_%=:\n\t"
        "s_waitcnt vmcnt(2)\n\t"
        "s_branch .Lmpg_wb_%=\n"
        ".Lmpg_w1_%=:\n\t"
        "s_waitcnt vmcnt(1)\n\t"
        "s_branch .Lmpg_wb_%=\n"
        ".Lmpg_w0_%=:\n\t"
        "s_waitcnt vmcnt(0)\n"
        ".Lmpg_wb_%=:\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "s_barrier" ::"s"(late)
        : "memory", "scc");
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
