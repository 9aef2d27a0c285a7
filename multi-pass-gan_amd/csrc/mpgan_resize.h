// The legacy-TF1 resize look-ups that mpgan_elem.hip (mpg_resize_bilinear, mpg_resize_bicubic), mpgan_tempo.hip
// (mpg_tempo_vel_pack) and mpgan_train_elem.hip (mpg_resize_bilinear_bwd, mpg_resize_bicubic_bwd) share: ONE statement of the
// coordinate, of the taps of an output index along one axis and of the three bilinear lerps, so that the forward kernels give
// the same bits and the adjoints gather with the forward's own indices and weights.
#pragma once
#include "mpgan_internal.h"

namespace mpg::valu {

// The source coordinate float32(o) * scale, rounded to float32 before its floor and fraction are taken, as TF1 does.  With
// contraction allowed the compiler folds the product into the later `s - floor(s)` as an FMA, which takes the fraction of
// the UNROUNDED product: a bilinear weight a float32 ulp off, and a bicubic table offset one off where frac * 1024 is a tie.
__device__ __forceinline__ float resize_src_coord(int o, float scale) {
#pragma clang fp contract(off)
    return (float)o * scale;
}

// The two taps of output index o along an axis of in_size sources: i0 = floor(s) and its upper neighbour, clamped to the last
// source, with the weights (1 - l, l) of the fraction l.  The forward lerps with l alone; the adjoint uses both weights.
__device__ __forceinline__ void bilinear_taps(int o, float scale, int in_size, int idx[2], float wt[2]) {
    const float s = resize_src_coord(o, scale);
    const int i0 = (int)floorf(s);
    const float l = s - i0;
    idx[0] = i0;
    idx[1] = min(i0 + 1, in_size - 1);
    wt[0] = 1.f - l;
    wt[1] = l;
}

// output pixel (oy, ox) of the resize of one channel plane: `base` points at the channel's value of pixel (0, 0) of an
// [h, w] image whose pixels lie c floats apart; sy = h / oh, sx = w / ow; the upper neighbours are clamped to the last
// row / column
__device__ __forceinline__ float resize_bilinear_at(const float* __restrict__ base, int h, int w, int c, int oy, int ox,
                                                    float sy, float sx) {
    int iy[2], ix[2];
    float wy[2], wx[2];
    bilinear_taps(oy, sy, h, iy, wy);
    bilinear_taps(ox, sx, w, ix, wx);
    const int y0 = iy[0], y1 = iy[1], x0 = ix[0], x1 = ix[1];
    const float ly = wy[1], lx = wx[1];
    const float tl = base[((size_t)y0 * w + x0) * c], tr = base[((size_t)y0 * w + x1) * c];
    const float bl = base[((size_t)y1 * w + x0) * c], br = base[((size_t)y1 * w + x1) * c];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    return top + (bot - top) * ly;
}

// The four Keys weights (A = -0.75) of table offset `off` in 0..1024: the entries (off, 1024 - off) of the TF1 coefficient
// table, evaluated in place.  Stated once and expanded under either contraction setting (a pragma is lexical).
#define MPG_KEYS_WEIGHTS(off, wt)                                                  \
    do {                                                                           \
        const float A = -0.75f;                                                    \
        const float x0 = (float)(off) / 1024.f;                                    \
        const float x1 = (float)(1024 - (off)) / 1024.f;                           \
        const float xa = x0 + 1.f, xb = x1 + 1.f;                                  \
        (wt)[0] = ((A * xa - 5.f * A) * xa + 8.f * A) * xa - 4.f * A;              \
        (wt)[1] = ((A + 2.f) * x0 - (A + 3.f)) * x0 * x0 + 1.f;                    \
        (wt)[2] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;                    \
        (wt)[3] = ((A * xb - 5.f * A) * xb + 8.f * A) * xb - 4.f * A;              \
    } while (0)

// TABLE_BITS false: contraction as the compiler likes it, the weights mpg_resize_bicubic has always used (FMA chains, up to
// 10 x 2^-24 from the float32 table in absolute terms -- nothing next to the weight sum of an output, which is what the
// forward's error is measured against).  TABLE_BITS true: every product and sum rounded, the bits of the TF1 table itself.
// The adjoint takes these: a source that only an outer tap (weight -0.07) reaches has nothing to dilute the deviation.
template <bool TABLE_BITS>
__device__ __forceinline__ void keys_weights(int off, float wt[4]) {
    if constexpr (TABLE_BITS) {
#pragma clang fp contract(off)
        MPG_KEYS_WEIGHTS(off, wt);
    } else {
        MPG_KEYS_WEIGHTS(off, wt);
    }
}

// TF 1.x ResizeBicubic: fraction quantised to 1/1024, taps i - 1 .. i + 2 clamped to the axis.
template <bool TABLE_BITS = false>
__device__ __forceinline__ void bicubic_taps(int o, float scale, int in_size, int idx[4], float wt[4]) {
    const float s = resize_src_coord(o, scale);
    const int i = (int)floorf(s);
    const float delta = s - (float)i;
    const int off = (int)lrintf(delta * 1024.f);
    keys_weights<TABLE_BITS>(off, wt);
#pragma unroll
    for (int t = 0; t < 4; ++t) idx[t] = min(max(i - 1 + t, 0), in_size - 1);
}

}  // namespace mpg::valu
