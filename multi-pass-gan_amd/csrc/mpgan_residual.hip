// The residual term of the upsampling_mode 0 growing generator (GAN/multipassGAN-8x.py:720-721):
//   out = dens + resize_images(slice(src, channel c_src), [h, wl * f], bicubic)
// for src fp32 NHWC [n, h, wl, c] and dens / out fp32 [n, h, wl * f, 1].  The resize keeps the rows: at row scale 1 the
// source coordinate of row o is o, its fraction 0, its table offset 0, and the four Keys weights of offset 0 are exactly
// (0, 1, 0, 0) -- so the sixteen taps of mpg_resize_bicubic are the four column taps of the same row, and that is all this
// kernel reads: coordinate, table offset, weights and the order of the four-term sum are those of resize_bicubic_kernel's
// inner row (mpgan_resize.h).  One pass: dens is read once and out written once, V floats a thread (one 16-byte access each
// when the row length is a multiple of 4 and both pointers are 16-byte aligned, scalar accesses otherwise); the taps of
// src come through the cache, every line of the low plane leaves HBM once.  Bytes per output pixel: 4 (dens) + 4 (out) +
// 4 c / f (the lines of src hold all c channels).  Grid-stride over the V-wide units with a capped grid; 64-bit offsets.
// out and dens are different buffers.
#include "mpgan_resize.h"
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

constexpr unsigned COLS_GRID = 2048;

template <int V>
__global__ void bicubic_cols_add_kernel(const float* __restrict__ src, size_t rows, int wl, int c, int c_src, int wo, float sx,
                                        const float* __restrict__ dens, float* __restrict__ out) {
    const size_t upr = (size_t)(wo / V);                   // units per row (V divides wo)
    const size_t units = rows * upr;
    for (size_t u = (size_t)blockIdx.x * BLK + threadIdx.x; u < units; u += (size_t)gridDim.x * BLK) {
        const size_t row = u / upr;
        const int x0 = (int)(u - row * upr) * V;
        const float* base = src + row * (size_t)wl * c + c_src;
        const size_t o = row * (size_t)wo + x0;
        float d[V], r[V];
        ldv<V>(dens + o, d);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            int ix[4];
            float wx[4];
            bicubic_taps(x0 + j, sx, wl, ix, wx);
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc += base[(size_t)ix[t] * c] * wx[t];
            r[j] = d[j] + acc;
        }
        stv<V>(out + o, r);
    }
}

}  // namespace

extern "C" int mpg_bicubic_cols_add(mpg_stream_t stream, const float* src, int n, int h, int wl, int c, int c_src, int f,
                                    const float* dens, float* out) {
    MPG_REQUIRE(src && dens && out, "mpg_bicubic_cols_add: null pointer");
    MPG_REQUIRE(out != dens && out != src, "mpg_bicubic_cols_add: out must be a buffer of its own");
    MPG_REQUIRE(n >= 1 && h >= 1 && wl >= 1 && c >= 1, "mpg_bicubic_cols_add: bad shape [%d,%d,%d,%d]", n, h, wl, c);
    MPG_REQUIRE(c_src >= 0 && c_src < c, "mpg_bicubic_cols_add: channel %d of %d", c_src, c);
    MPG_REQUIRE(f >= 1 && (f & (f - 1)) == 0 && f <= 64 && (long long)wl * f <= 0x7fffffffLL,
                "mpg_bicubic_cols_add: factor %d on %d columns (a power of two up to 64)", f, wl);
    const int wo = wl * f;
    const size_t rows = (size_t)n * h;
    const float sx = (float)wl / (float)wo;                   // as mpg_resize_bicubic forms it
    const bool vec = wo % 4 == 0 && ((reinterpret_cast<uintptr_t>(dens) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const size_t units = rows * (size_t)(vec ? wo / 4 : wo);
    size_t blocks = (units + BLK - 1) / BLK;
    if (blocks > COLS_GRID) blocks = COLS_GRID;
    if (vec)
        hipLaunchKernelGGL(bicubic_cols_add_kernel<4>, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, src, rows, wl, c,
                           c_src, wo, sx, dens, out);
    else
        hipLaunchKernelGGL(bicubic_cols_add_kernel<1>, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, src, rows, wl, c,
                           c_src, wo, sx, dens, out);
    MPG_LAUNCH_CHECK("bicubic_cols_add_kernel");
}
