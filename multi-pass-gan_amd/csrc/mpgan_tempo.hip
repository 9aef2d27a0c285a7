// The input of the 8x temporal critic with `useVelInTDisc` (multipassGAN-8x.py:1204-1208, read at :878) in one pass.
// The reference appends three channels float(upresFac) * resize_images(vel_t, [th, th], method=0) to the advected
// [3B, th, th, 1] frames, reshapes the [3B, th, th, 4] tensor F to [-1, 3, P] (P = th th), transposes (0, 2, 1) and reads
// the result as [-1, th, th, 12].  With four channels that is a fixed permutation of the 12 B P values; for output flat
// index o
//     m = o / (3P),  q = (o % (3P)) / 3,  t = o % 3;    f = (3m + t) P + q  (flat index into F)
//     n = f / (4P),  p = (f % (4P)) / 4,  c = f % 4     (frame row, pixel, channel of F)
// Entries: mpg_tempo_vel_pack (out[o] = F[f], the velocity channels interpolated and scaled on the fly, so the upsampled
// [3B, th, th, 3] tensor, the concatenation and the transpose are never written) and mpg_tempo_vel_pack_bwd (the gradient
// with respect to the frames: the inverse map, one output element per read).  HBM-bound; the loads are gathers inside the
// three frames of a row, every lane stores V consecutive floats.
#include "mpgan_resize.h"
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

template <int V>
__global__ void tempo_vel_pack_kernel(const float* __restrict__ frames, const float* __restrict__ x_t, size_t total, int tl,
                                      int th, float s_res, float scale, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (idx * V >= total) return;
    const size_t P = (size_t)th * th, P3 = 3 * P, P4 = 4 * P;
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const size_t o = idx * V + j;
        const size_t m = o / P3, r = o - m * P3;
        const size_t q = r / 3, t = r - q * 3;
        const size_t f = (3 * m + t) * P + q;
        const size_t n = f / P4, rem = f - n * P4;
        const size_t p = rem >> 2;
        const int c = (int)(rem & 3);
        if (c == 0) {
            v[j] = frames[n * P + p];
        } else {
            const int oy = (int)(p / th), ox = (int)(p - (size_t)oy * th);
            // a separately rounded product: scale * resize, never contracted into the last lerp of the look-up
            v[j] = __fmul_rn(scale, resize_bilinear_at(x_t + n * ((size_t)tl * tl * 4) + c, tl, tl, 4, oy, ox, s_res, s_res));
        }
    }
    stv<V>(out + idx * V, v);
}

// dframes[n P + p] = dout[o], o the position of F[n, p, 0]:  f = 4 (n P + p);  m = f / (3P), t = (f % (3P)) / P, q = f % P;
// o = 3 P m + 3 q + t
template <int V>
__global__ void tempo_vel_pack_bwd_kernel(const float* __restrict__ dout, size_t total, size_t P,
                                          float* __restrict__ dframes) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (idx * V >= total) return;
    const size_t P3 = 3 * P;
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const size_t f = 4 * (idx * V + j);
        const size_t m = f / P3, r = f - m * P3;
        const size_t t = r / P, q = r - t * P;
        v[j] = dout[m * P3 + 3 * q + t];
    }
    stv<V>(dframes + idx * V, v);
}

}  // namespace

extern "C" int mpg_tempo_vel_pack(mpg_stream_t stream, const float* frames, const float* x_t, int B, int tl, int th,
                                  float scale, float* out) {
    MPG_REQUIRE(frames && x_t && out, "mpg_tempo_vel_pack: null pointer");
    MPG_REQUIRE(B >= 1 && tl >= 1 && th >= tl, "mpg_tempo_vel_pack: bad shape (B %d, %d -> %d)", B, tl, th);
    MPG_REQUIRE(th % tl == 0, "mpg_tempo_vel_pack: tile size %d is no multiple of the low-res tile size %d", th, tl);
    const size_t total = (size_t)12 * B * th * th;            // 12 P: always a multiple of 4
    const float s_res = (float)tl / (float)th;                // as mpg_resize_bilinear forms it
    if ((((uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL((tempo_vel_pack_kernel<4>), dim3(grid_for(total / 4)), dim3(BLK), 0, (hipStream_t)stream, frames,
                           x_t, total, tl, th, s_res, scale, out);
    else
        hipLaunchKernelGGL((tempo_vel_pack_kernel<1>), dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, frames, x_t,
                           total, tl, th, s_res, scale, out);
    MPG_LAUNCH_CHECK("tempo_vel_pack_kernel");
}

extern "C" int mpg_tempo_vel_pack_bwd(mpg_stream_t stream, const float* dout, int B, int th, float* dframes) {
    MPG_REQUIRE(dout && dframes, "mpg_tempo_vel_pack_bwd: null pointer");
    MPG_REQUIRE(B >= 1 && th >= 1, "mpg_tempo_vel_pack_bwd: bad shape (B %d, tile size %d)", B, th);
    const size_t P = (size_t)th * th, total = 3 * (size_t)B * P;
    if ((total & 3) == 0 && (((uintptr_t)dframes) & 15) == 0)
        hipLaunchKernelGGL((tempo_vel_pack_bwd_kernel<4>), dim3(grid_for(total / 4)), dim3(BLK), 0, (hipStream_t)stream, dout,
                           total, P, dframes);
    else
        hipLaunchKernelGGL((tempo_vel_pack_bwd_kernel<1>), dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, dout,
                           total, P, dframes);
    MPG_LAUNCH_CHECK("tempo_vel_pack_bwd_kernel");
}
