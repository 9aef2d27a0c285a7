// The tempoGAN vorticity input channels (useVorticities): addVorticity of GAN/multipassGAN-8x.py:1440-1446, 2D branch, as
// written -- velocity component 0 is tile channel 1, component 1 is tile channel 2, and only the third of the three
// appended channels is filled:
//   y[..., :c] = x,  y[..., c] = y[..., c+1] = 0,
//   y[i, j, c+2] = 0.5 * ((x[i+1, j, 2] - x[i-1, j, 2]) - (x[i, j+1, 1] - x[i, j-1, 1]))   for 1 <= i <= h-2, 1 <= j <= w-2
// and 0 on the border (i the row, j the column).  Two subtractions, one subtraction, one product: nothing can contract, so
// the result is defined bit for bit.  One pass: x is read once (the four neighbours of a pixel come from cache), y is
// written once.  c + 3 floats a pixel are no multiple of 16 bytes, so a thread owns V consecutive floats of the FLAT
// output (one 16-byte store when y is 16-byte aligned), whatever pixels they belong to.  Offsets are 64-bit: a 4x pass-2
// batch [256,256,256,4] -> [...,7] is past 2^32 bytes.
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

template <int V>
__global__ void vorticity_append_kernel(const float* __restrict__ x, size_t total, int h, int w, int c, float* __restrict__ y) {
    const unsigned t = blockIdx.x * BLK + threadIdx.x;      // the host checks that threads and pixels fit 32 bits
    const size_t o0 = (size_t)t * V;
    if (o0 >= total) return;
    const unsigned cc = c + 3;
    // pixel of the first element, its channel, column and row, in 32-bit divisions: V * cc floats are V whole pixels,
    // thread t owns part t % cc of group t / cc.  (64-bit divisions of the flat offset timed the same: 0.306 against
    // 0.310 ms on [256,256,256,4], profiles/vorticity/timing.md -- the kernel waits for its loads.)
    const unsigned g = t / cc, r = (t - g * cc) * V;
    size_t p = (size_t)g * V + r / cc;
    int k = (int)(r % cc);
    const unsigned row = (unsigned)p / (unsigned)w;
    int j = (int)((unsigned)p - row * (unsigned)w);
    int i = (int)(row % (unsigned)h);
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        float val = 0.f;
        if (o0 + e < total) {
            const float* px = x + p * c;
            if (k < c) {
                val = px[k];
            } else if (k == c + 2 && i >= 1 && i <= h - 2 && j >= 1 && j <= w - 2) {
                const size_t rs = (size_t)w * c;
                const float dy = px[rs + 2] - *(px - rs + 2);
                const float dx = px[c + 1] - *(px - c + 1);
                val = 0.5f * (dy - dx);
            }
        }
        v[e] = val;
        if (++k == (int)cc) {
            k = 0; ++p;
            if (++j == w) {
                j = 0;
                if (++i == h) i = 0;
            }
        }
    }
    if (V == 1 || o0 + V <= total) {
        stv<V>(y + o0, v);
    } else {
        for (int e = 0; e < V && o0 + e < total; ++e) y[o0 + e] = v[e];
    }
}

}  // namespace

extern "C" int mpg_vorticity_append(mpg_stream_t stream, const float* x, int n, int h, int w, int c, float* y) {
    MPG_REQUIRE(c >= 4, "mpg_vorticity_append: %d channels (density and three velocity components come first: c >= 4)", c);
    MPG_REQUIRE(n >= 0 && h >= 1 && w >= 1, "mpg_vorticity_append: bad shape [%d,%d,%d,%d]", n, h, w, c);
    if (n == 0) return MPG_OK;               // an empty batch has no storage: its pointers are not looked at
    MPG_REQUIRE(x && y, "mpg_vorticity_append: null pointer");
    const size_t total = (size_t)n * h * w * (c + 3);
    const bool vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    const size_t threads = vec ? (total + 3) / 4 : total;
    MPG_REQUIRE(threads + BLK <= 0xffffffffull && (size_t)n * h * w <= 0xffffffffull,
                "mpg_vorticity_append: [%d,%d,%d,%d] is too large for one launch (2^32 pixels, 2^32 threads)", n, h, w, c);
    if (vec)
        hipLaunchKernelGGL(vorticity_append_kernel<4>, dim3(grid_for(threads)), dim3(BLK), 0, (hipStream_t)stream, x, total, h, w, c, y);
    else
        hipLaunchKernelGGL(vorticity_append_kernel<1>, dim3(grid_for(threads)), dim3(BLK), 0, (hipStream_t)stream, x, total, h, w, c, y);
    MPG_LAUNCH_CHECK("vorticity_append_kernel");
}
