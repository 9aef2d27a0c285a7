// Internal helpers shared by the HIP translation units of libmpgan_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#include "mpgan.h"

namespace mpg {

void set_error(const char* fmt, ...);

inline int hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return MPG_ERR_HIP;
    }
    return MPG_OK;
}

#define MPG_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            mpg::set_error(__VA_ARGS__);  \
            return MPG_ERR_ARG;           \
        }                                 \
    } while (0)

#define MPG_LAUNCH_CHECK(name) return mpg::hip_check(hipGetLastError(), name)

// Zero `bytes` (a multiple of 4) of device memory with a kernel on `stream`.  Used instead of
// hipMemsetAsync for buffers that atomics accumulate into: memset nodes of a captured hipGraph were
// observed to lose their ordering against the neighbouring kernels on replay (ROCm 7.2), a plain
// kernel node does not.
hipError_t zero_async(void* ptr, size_t bytes, hipStream_t stream);

// 256 zero bytes of device memory (per device, allocated on first use outside any capture): the source of LDS-DMA lanes
// that must deliver zeros.  nullptr when the allocation failed.
const char* zero_page();

__device__ __forceinline__ float apply_act(float v, int act, float leak) {
    // MPG_ACT_RELU: tf.nn.relu; MPG_ACT_LRELU: 0.5(1+leak) x + 0.5(1-leak)|x| (GAN.py:733-737)
    if (act == MPG_ACT_RELU) return fmaxf(v, 0.f);
    if (act == MPG_ACT_LRELU) return 0.5f * (1.f + leak) * v + 0.5f * (1.f - leak) * fabsf(v);
    if (act == MPG_ACT_TANH) return tanhf(v);
    return v;
}

// power-of-two scale 2^k that brings a tensor with absolute maximum `amax` into [2^8, 2^9): fp16 hi/lo splits of
// gradients (1e-4 .. 1e-8 in magnitude) would otherwise land in the fp16 subnormal range.  amax = m 2^e with m in
// [0.5, 1) gives k = min(9 - e, 126): the cap (it bites below 2^-118, where the scaled maximum stays under 2^8) keeps
// 2^k and its reciprocal normal fp32 numbers -- 2^(9 - e) is inf from amax < 2^-119 on, which turned zeros into NaN
// (0 * inf) and every unscaled sum into 0 (1 / inf).  k is 0 (scale 1) for amax <= 0, NaN and amax >= 3.0e38 (inf).
__device__ __forceinline__ int pow2_scale_exp(float amax) {
    if (!(amax > 0.f) || !(amax < 3.0e38f)) return 0;
    int e;
    frexpf(amax, &e);
    return 9 - e < 126 ? 9 - e : 126;
}
__device__ __forceinline__ float pow2_scale(float amax) { return ldexpf(1.f, pow2_scale_exp(amax)); }

// Raise a kernel's dynamic-LDS limit once per (kernel, device): hipFuncSetAttribute is a driver call and the
// value never has to shrink, so a launch only pays for it the first time a size above the recorded one is asked.
// `slot` is a per-kernel static array of 64 ints (one per device), zero-initialised.
inline hipError_t ensure_dyn_lds(const void* kern, int bytes, int* slot) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    int seen = __atomic_load_n(&slot[dev], __ATOMIC_ACQUIRE);
    if (bytes <= seen) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    while (seen < bytes && !__atomic_compare_exchange_n(&slot[dev], &seen, bytes, false, __ATOMIC_RELEASE, __ATOMIC_ACQUIRE)) {
    }
    return hipSuccess;
}

// Launch `Kernel` with `lds` bytes of dynamic LDS.  Above the 48 KiB a kernel gets by default its limit is raised
// first (ensure_dyn_lds; the array below is the kernel's own, one entry per device), to max(lds, Reserve): a kernel
// that names a Reserve pays the driver call once, whatever sizes its later launches ask for.  The launch's own
// error is left in hipGetLastError().
template <auto Kernel, size_t Reserve = 0, class... A>
hipError_t launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
    static int lds_limit[64] = {0};
    const size_t want = lds > Reserve ? lds : Reserve;
    if (want > 48 * 1024) {
        hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(Kernel), (int)want, lds_limit);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return hipSuccess;
}

}  // namespace mpg
