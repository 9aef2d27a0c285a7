// The legacy-TF1 bilinear look-up that mpgan_elem.hip (mpg_resize_bilinear) and mpgan_tempo.hip (mpg_tempo_vel_pack) share:
// ONE statement of the coordinate and of the three lerps, so that both kernels give the same bits.
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

// output pixel (oy, ox) of the resize of one channel plane: `base` points at the channel's value of pixel (0, 0) of an
// [h, w] image whose pixels lie c floats apart; sy = h / oh, sx = w / ow; the upper neighbours are clamped to the last
// row / column
__device__ __forceinline__ float resize_bilinear_at(const float* __restrict__ base, int h, int w, int c, int oy, int ox,
                                                    float sy, float sx) {
    const float fy = resize_src_coord(oy, sy), fx = resize_src_coord(ox, sx);
    const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = fy - y0, lx = fx - x0;
    const float tl = base[((size_t)y0 * w + x0) * c], tr = base[((size_t)y0 * w + x1) * c];
    const float bl = base[((size_t)y1 * w + x0) * c], br = base[((size_t)y1 * w + x1) * c];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    return top + (bot - top) * ly;
}

}  // namespace mpg::valu
