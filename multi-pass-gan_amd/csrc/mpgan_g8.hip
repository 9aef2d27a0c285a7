// fp32 NHWC <-> G8 ([N][ceil(C/8)][2 planes: hi, lo][H][W][8 x fp16], value = hi + lo), the tensor layout of the fused
// convolutions and the weight gradient; and the pixel norm of a G8 tensor wider than one fused launch (mpg_pixel_norm_g8).
#include "mpgan_internal.h"
#include "mpgan_mfma_dev.h"

namespace {

using mpg::dev::half8;

// fp32 NHWC -> G8
__global__ void f32_to_g8_kernel(const float* __restrict__ x, int n, int h, int w, int c, int c_off, int cin,
                                 const float* __restrict__ amax, _Float16* __restrict__ out) {
    const float scale = amax != nullptr ? mpg::pow2_scale(*amax) : 1.f;
    const int cg_n = (cin + 7) >> 3;
    const size_t plane_px = (size_t)h * w;
    const size_t total = (size_t)n * cg_n * plane_px;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const size_t px = idx % plane_px;
    const size_t t = idx / plane_px;
    const int cg = t % cg_n;
    const int b = t / cg_n;
    const float* src = x + ((size_t)b * plane_px + px) * c + c_off + cg * 8;
    half8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = (cg * 8 + j < cin) ? src[j] * scale : 0.f;
        hi[j] = (_Float16)v;
        lo[j] = (_Float16)(v - (float)hi[j]);
    }
    _Float16* dst = out + ((((size_t)b * cg_n + cg) * 2) * plane_px + px) * 8;
    *reinterpret_cast<half8*>(dst) = hi;
    *reinterpret_cast<half8*>(dst + plane_px * 8) = lo;
}

// The same conversion for wide tensors (cin >= 32, 16-byte aligned rows): the kernel above reads 32 bytes per thread at a
// stride of c floats (2.0 TB/s on a 128-channel tensor).  Here a block takes 32 pixels x up to 128 channels: the pixel
// rows are read as float4 by 32 consecutive threads (512 contiguous bytes), staged in LDS, and every (pixel, group) pair is
// then converted by one thread that writes 16 bytes per plane next to its neighbour pixel's.
constexpr int G8T_PX = 32, G8T_CH = 128, G8T_STRIDE = G8T_CH + 4;

__global__ __launch_bounds__(256) void f32_to_g8_tiled_kernel(const float* __restrict__ x, int n, int h, int w, int c, int c_off,
                                                              int cin, const float* __restrict__ amax,
                                                              _Float16* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[G8T_PX * G8T_STRIDE];
    const float scale = amax != nullptr ? mpg::pow2_scale(*amax) : 1.f;
    const int cg_n = (cin + 7) >> 3;
    const size_t plane_px = (size_t)h * w;
    const size_t px0 = (size_t)blockIdx.x * G8T_PX;          // first pixel of the tile within image b
    const int ch0 = blockIdx.y * G8T_CH;                      // first channel (of the cin window) of the tile
    const int b = blockIdx.z;
    const int nch = min(G8T_CH, cin - ch0);                   // channels of this tile
    const int tid = threadIdx.x;
    const int q = tid & 31, pr = tid >> 5;                    // channel quad, pixel sub-row
#pragma unroll
    for (int i = 0; i < G8T_PX / 8; ++i) {
        const int p = pr + 8 * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (px0 + p < plane_px && q * 4 < nch) {
            const float* src = x + ((size_t)b * plane_px + px0 + p) * c + c_off + ch0 + q * 4;
            if (q * 4 + 3 < nch) {
                v = *reinterpret_cast<const float4*>(src);
            } else {
                v.x = src[0];
                if (q * 4 + 1 < nch) v.y = src[1];
                if (q * 4 + 2 < nch) v.z = src[2];
            }
        }
        *reinterpret_cast<float4*>(tile + p * G8T_STRIDE + q * 4) = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
    }
    __syncthreads();
    const int ng = (nch + 7) >> 3;
    for (int u = tid; u < ng * G8T_PX; u += 256) {
        const int p = u % G8T_PX, g = u / G8T_PX;
        if (px0 + p >= plane_px) continue;
        const float4 a0 = *reinterpret_cast<const float4*>(tile + p * G8T_STRIDE + g * 8);
        const float4 a1 = *reinterpret_cast<const float4*>(tile + p * G8T_STRIDE + g * 8 + 4);
        float vv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        half8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            hi[j] = (_Float16)vv[j];
            lo[j] = (_Float16)(vv[j] - (float)hi[j]);
        }
        _Float16* dst = out + ((((size_t)b * cg_n + (ch0 >> 3) + g) * 2) * plane_px + px0 + p) * 8;
        *reinterpret_cast<half8*>(dst) = hi;
        *reinterpret_cast<half8*>(dst + plane_px * 8) = lo;
    }
}

// G8 -> fp32 NHWC
__global__ void g8_to_f32_kernel(const _Float16* __restrict__ g, int n, int h, int w, int c, float* __restrict__ y) {
    const int cg_n = (c + 7) >> 3;
    const size_t plane_px = (size_t)h * w;
    const size_t total = (size_t)n * plane_px * c;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int ch = idx % c;
    const size_t t = idx / c;
    const size_t px = t % plane_px;
    const int b = t / plane_px;
    const _Float16* src = g + ((((size_t)b * cg_n + (ch >> 3)) * 2) * plane_px + px) * 8 + (ch & 7);
    y[idx] = (float)src[0] + (float)src[plane_px * 8];
}

// GAN.pixel_norm (GAN.py:472-474) of a G8 tensor in place: y = x * rsqrt(mean_c(x^2) + eps) with x = hi + lo, written
// back as hi / lo planes and, when y32 is given, as fp32 NHWC too.  The fused epilogue does this for up to 128 channels
// inside the launch; a wider layer is several window launches (mpg_conv2d_fused_window) and this pass behind them.
// A block takes 64 consecutive pixels of one image; wave s of its S waves takes the channel groups s, s + S, ... (at
// most PN_GPT of them: c <= 64 S), so a wave's 64 lanes read 1 KiB of consecutive 16-byte pixels of a group plane per
// access and every value is read from memory once and kept in registers until it is scaled.  The S partial sums of a
// pixel meet in LDS and are added in the same order by every wave.  Channels beyond c (padding of the last group) are
// taken as zero and written as zero.
constexpr int PN_PX = 64, PN_GPT = 8;

template <int S>
__global__ __launch_bounds__(PN_PX * S) void pixel_norm_g8_kernel(_Float16* __restrict__ g, int h, int w, int c, float eps,
                                                                  float* __restrict__ y32) {
    __shared__ float part[S][PN_PX];
    const int cg_n = (c + 7) >> 3;
    const size_t plane_px = (size_t)h * w;
    const int lane = threadIdx.x & (PN_PX - 1), slice = threadIdx.x / PN_PX;
    const size_t px = (size_t)blockIdx.x * PN_PX + lane;
    const int b = blockIdx.y;
    const bool ok = px < plane_px;
    float v[PN_GPT][8];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < PN_GPT; ++k) {
        const int cg = slice + k * S;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
        if (ok && cg < cg_n) {
            const _Float16* src = g + ((((size_t)b * cg_n + cg) * 2) * plane_px + px) * 8;
            const half8 hi = *reinterpret_cast<const half8*>(src);
            const half8 lo = *reinterpret_cast<const half8*>(src + plane_px * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = (cg * 8 + j < c) ? (float)hi[j] + (float)lo[j] : 0.f;
                v[k][j] = x;
                ss = fmaf(x, x, ss);
            }
        }
    }
    part[slice][lane] = ss;
    __syncthreads();
    if (!ok) return;
    float tot = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) tot += part[s][lane];
    const float sc = rsqrtf(tot / (float)c + eps);
#pragma unroll
    for (int k = 0; k < PN_GPT; ++k) {
        const int cg = slice + k * S;
        if (cg < cg_n) {
            // lo is the rest behind the hi that is STORED: the compiler is kept from forming hi a second time for the
            // subtraction (it folds the scaling into the conversion, v_fma_mixlo_f16, whose rounding of the product
            // need not be that of v_cvt_pk_f16_f32 on the rounded product: a pair off by an fp16 ulp now and then).
            // The product itself is pinned too: hi, lo and y32 are all taken from the ROUNDED fp32 product.  Left alone
            // the compiler contracts the subtraction below with the multiply, lo = fp16(fma(x, sc, -hi)) of the
            // unrounded product, and one lo in eleven was an ulp off the canonical split of the y32 beside it
            // (tests/test_g8_gpu.py: test_pixel_norm_g8_planes).
            half8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[k][j] *= sc;
                asm volatile("" : "+v"(v[k][j]));
                hi[j] = (_Float16)v[k][j];
            }
            asm volatile("" : "+v"(hi));
#pragma unroll
            for (int j = 0; j < 8; ++j) lo[j] = (_Float16)(v[k][j] - (float)hi[j]);
            _Float16* dst = g + ((((size_t)b * cg_n + cg) * 2) * plane_px + px) * 8;
            *reinterpret_cast<half8*>(dst) = hi;
            *reinterpret_cast<half8*>(dst + plane_px * 8) = lo;
            if (y32 != nullptr) {
                float* q = y32 + ((size_t)b * plane_px + px) * c + cg * 8;
                if (cg * 8 + 8 <= c && (c & 3) == 0) {
                    *reinterpret_cast<float4*>(q) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
                    *reinterpret_cast<float4*>(q + 4) = make_float4(v[k][4], v[k][5], v[k][6], v[k][7]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (cg * 8 + j < c) q[j] = v[k][j];
                }
            }
        }
    }
}

}  // namespace

extern "C" size_t mpg_g8_bytes(int n, int h, int w, int c) {
    if (n < 1 || h < 1 || w < 1 || c < 1) return 0;
    return (size_t)n * ((c + 7) / 8) * 2 * h * w * 16;
}

extern "C" int mpg_f32_to_g8_scaled(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int c_off, int cin,
                                    int flavour, const float* amax, void* out) {
    MPG_REQUIRE(flavour == MPG_G8_F16, "mpg_f32_to_g8: bad flavour %d", flavour);
    MPG_REQUIRE(x && out, "mpg_f32_to_g8: null pointer");
    MPG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1 && c_off >= 0 && cin >= 1 && c_off + cin <= c, "mpg_f32_to_g8: bad shape");
    const size_t total = (size_t)n * ((cin + 7) / 8) * h * w;
    if (cin >= 32 && (c % 4) == 0 && (c_off % 4) == 0 && (((uintptr_t)x) & 15) == 0 && n <= 65535) {
        const dim3 grid((unsigned)(((size_t)h * w + G8T_PX - 1) / G8T_PX), (unsigned)((cin + G8T_CH - 1) / G8T_CH), (unsigned)n);
        hipLaunchKernelGGL(f32_to_g8_tiled_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, n, h, w, c, c_off, cin,
                           amax, (_Float16*)out);
        MPG_LAUNCH_CHECK("f32_to_g8_tiled_kernel");
    }
    hipLaunchKernelGGL(f32_to_g8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, h,
                       w, c, c_off, cin, amax, (_Float16*)out);
    MPG_LAUNCH_CHECK("f32_to_g8_kernel");
}

extern "C" int mpg_f32_to_g8(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int c_off, int cin,
                             int flavour, void* out) {
    return mpg_f32_to_g8_scaled(stream, x, n, h, w, c, c_off, cin, flavour, nullptr, out);
}

extern "C" int mpg_g8_to_f32(mpg_stream_t stream, const void* g8, int n, int h, int w, int c, float* y) {
    MPG_REQUIRE(g8 && y, "mpg_g8_to_f32: null pointer");
    MPG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1, "mpg_g8_to_f32: bad shape");
    const size_t total = (size_t)n * h * w * c;
    hipLaunchKernelGGL(g8_to_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16*)g8, n, h, w, c, y);
    MPG_LAUNCH_CHECK("g8_to_f32_kernel");
}

extern "C" int mpg_pixel_norm_g8(mpg_stream_t stream, void* g8, int n, int h, int w, int c, float eps, float* y) {
    MPG_REQUIRE(g8 != nullptr, "mpg_pixel_norm_g8: null pointer");
    MPG_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && c >= 1, "mpg_pixel_norm_g8: bad shape");
    // a thread keeps PN_GPT groups of its pixel: 8 waves cover 64 groups
    MPG_REQUIRE(c <= 8 * PN_GPT * 8, "mpg_pixel_norm_g8: %d channels (at most %d)", c, 8 * PN_GPT * 8);
    MPG_REQUIRE((((uintptr_t)g8) & 15) == 0 && (((uintptr_t)y) & 15) == 0, "mpg_pixel_norm_g8: misaligned tensor");
    const size_t blocks = ((size_t)h * w + PN_PX - 1) / PN_PX;
    MPG_REQUIRE(blocks < ((size_t)1 << 31), "mpg_pixel_norm_g8: %dx%d too large", h, w);
    const dim3 grid((unsigned)blocks, (unsigned)n);
    if ((c + 7) / 8 <= 4 * PN_GPT)
        hipLaunchKernelGGL(pixel_norm_g8_kernel<4>, grid, dim3(PN_PX * 4), 0, (hipStream_t)stream, (_Float16*)g8, h, w, c, eps, y);
    else
        hipLaunchKernelGGL(pixel_norm_g8_kernel<8>, grid, dim3(PN_PX * 8), 0, (hipStream_t)stream, (_Float16*)g8, h, w, c, eps, y);
    MPG_LAUNCH_CHECK("pixel_norm_g8_kernel");
}
