// Elementwise and reducing companions of the training step on the vector ALUs, fp32 NHWC: the backward passes of the
// activations, pixel norm, nearest / bilinear / bicubic resize and 2x2 average pool, lerp, the |a - b| / (a - b)^2 loss
// sums, the backward of the backward pass of the minibatch-stddev layer (WGAN-GP), and what held-out evaluation adds: the
// six means of a critic's logits and the 8-bit grey mosaics of test tiles.  Entries: mpg_act_bwd, mpg_pixel_norm_bwd,
// mpg_resize_nearest_bwd, mpg_resize_bilinear_bwd, mpg_resize_bicubic_bwd, mpg_avg_pool2_bwd, mpg_lerp, mpg_pair_reduce,
// mpg_minibatch_stddev_bwd2, mpg_logit_stats, mpg_tiles_to_gray8; and the second-order companions of tanh, pixel norm and
// max pool (a gradient penalty through them): mpg_act_bwd2, mpg_pixel_norm_bwd2, mpg_max_pool_gather.
#include "mpgan_resize.h"
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

// act_bwd2_tanh_kernel runs grid-stride: at most this many blocks, each thread then takes several float4
constexpr size_t ACT_BWD2_GRID = 1u << 16;

// ---------------------------------------------------------------- elementwise backward
// derivative expressed through the activation OUTPUT y (relu: y>0; lrelu: slope 1 / leak by sign of y,
// 0.5(1+leak) at 0 as tf.abs has a zero gradient there, GAN.py:733-737; tanh: 1 - y^2)
__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, size_t n, int act,
                               float leak, float* __restrict__ dx, unsigned int* __restrict__ amax) {
    float m = 0.f;
    auto one = [&](float g, float o) {
        float d = 1.f;
        if (act == MPG_ACT_RELU) d = o > 0.f ? 1.f : 0.f;
        else if (act == MPG_ACT_LRELU) d = o > 0.f ? 1.f : (o < 0.f ? leak : 0.5f * (1.f + leak));
        else if (act == MPG_ACT_TANH) d = 1.f - o * o;
        const float v = g * d;
        m = fmaxf(m, fabsf(v));
        return v;
    };
    const bool vec = ((((uintptr_t)dy) | ((uintptr_t)y) | ((uintptr_t)dx)) & 15) == 0;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < n4; i += (size_t)gridDim.x * BLK) {
        const float4 g = reinterpret_cast<const float4*>(dy)[i], o = reinterpret_cast<const float4*>(y)[i];
        reinterpret_cast<float4*>(dx)[i] = make_float4(one(g.x, o.x), one(g.y, o.y), one(g.z, o.z), one(g.w, o.w));
    }
    for (size_t idx = n4 * 4 + (size_t)blockIdx.x * BLK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * BLK)
        dx[idx] = one(dy[idx], y[idx]);
    if (amax != nullptr) block_absmax_to(m, amax);
}

// The derivative of act_bwd_kernel's dx = dy * (1 - y^2) (tanh) in y for a cotangent g of dx: d_y = ((-2 y) dy) g.  -2 y is
// exact, so an element is two rounded products and there is no sum for the compiler to contract.
__global__ void act_bwd2_tanh_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ g,
                                     size_t n, float* __restrict__ d_y) {
    auto one = [](float d, float o, float u) { return ((-2.f * o) * d) * u; };
    const bool vec = ((((uintptr_t)dy) | ((uintptr_t)y) | ((uintptr_t)g) | ((uintptr_t)d_y)) & 15) == 0;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < n4; i += (size_t)gridDim.x * BLK) {
        const float4 d = reinterpret_cast<const float4*>(dy)[i], o = reinterpret_cast<const float4*>(y)[i],
                     u = reinterpret_cast<const float4*>(g)[i];
        reinterpret_cast<float4*>(d_y)[i] = make_float4(one(d.x, o.x, u.x), one(d.y, o.y, u.y), one(d.z, o.z, u.z),
                                                        one(d.w, o.w, u.w));
    }
    for (size_t idx = n4 * 4 + (size_t)blockIdx.x * BLK + threadIdx.x; idx < n; idx += (size_t)gridDim.x * BLK)
        d_y[idx] = one(dy[idx], y[idx], g[idx]);
}

// y = x * r, r = rsqrt(mean_c x^2 + eps);  dx = r * (dy - y * mean_c(dy * y)); `lanes` consecutive lanes per pixel
__global__ void pixel_norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, size_t npix, int c,
                                      int lanes, float eps, float* __restrict__ dx) {
    const size_t gid = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t pix = gid / lanes;
    const int l = (int)(gid % lanes);
    const bool ok = pix < npix;
    const float* xp = x + (ok ? pix : 0) * c;
    const float* dp = dy + (ok ? pix : 0) * c;
    float ss = 0.f, dot = 0.f;
    if (ok)
        for (int i = l; i < c; i += lanes) { ss = fmaf(xp[i], xp[i], ss); dot = fmaf(dp[i], xp[i], dot); }
    for (int m = lanes >> 1; m > 0; m >>= 1) { ss += __shfl_xor(ss, m); dot += __shfl_xor(dot, m); }
    if (!ok) return;
    const float r = rsqrtf(ss / c + eps);
    const float k = dot * r * r / c;
    for (int i = l; i < c; i += lanes) dx[pix * c + i] = r * (dp[i] - xp[i] * k);
}

// The derivative of pixel_norm_bwd_kernel's dx = r dy - r^3 s x (s = mean_c(x dy)) in x, for a cotangent g of dx:
//   phi = g . dx = C (r u - r^3 s t),  t = mean_c(x g),  u = mean_c(dy g);  dr/dx_j = -r^3 x_j / C,  ds/dx_j = dy_j / C,
//   dt/dx_j = g_j / C   =>   d_x = -r^3 (u x + s g + t dy) + 3 r^5 s t x.
// The work split of pixel_norm_bwd_kernel: `lanes` consecutive lanes per pixel.  Every sum is an fmaf chain over the lane's
// channels l, l + lanes, ... from 0.f, then the xor tree from lanes / 2 down to 1, then one division by (float)c; every
// addition of the output is an explicit fmaf too, so nothing is left for the compiler to contract and the bits are those of
//   m = Sxx / c + eps, r = rsqrtf(m), s = Sxd / c, t = Sxg / c, u = Sdg / c, r2 = r r, r3 = r2 r, k = (((3 r3) r2) s) t,
//   p_i = fmaf(t, dy_i, fmaf(s, g_i, u x_i)),  d_x_i = fmaf(k, x_i, -(r3 p_i)).
// x, dy and g come from HBM once, for the sums; the second read, for the output, hits the cache.
// Error bound (tests/second_order_ref.py: pixel_norm_bwd2_bound), e = 2^-24, first order in e.  A sum has
// E = ceil(c / lanes) + log2(lanes) + 1 roundings (chain, tree, division): |s^ - s| <= E e S with S = mean_c |x dy|, the
// same for t (T = mean_c |x g|) and u (U = mean_c |dy g|); m has positive terms only and one more rounding, rsqrtf is within
// 1 ulp = 2 e, so r is off by rho = ((E + 1) / 2 + 2) e relative, r2 by 2 rho + e, r3 by 3 rho + 2 e.  With
// P = U |x| + S |g| + T |dy| >= |p| and every partial sum of p: |p^ - p| <= (E + 3) e P (E e per mean, one rounding each for
// the product and the two fmaf), and r3 p adds 3 rho + 3 e: (2.5 E + 13.5) e r^3 P.  k has four rounded products, r3 r2 is off
// by 5 rho + 3 e, s and t by E e of S and T: (4.5 E + 19.5) e K with K = 3 r^5 S T >= |k|.  The last fmaf rounds once at a
// magnitude of at most K |x| + r^3 P.  Together |error| <= (4.5 E + 20.5) e (r^3 P + K |x|); the test holds the kernel to
// (2.25 E + 10.5) 2^-23 (r^3 (U |x| + S |g| + T |dy|) + 3 r^5 S T |x|), the quarter added for the second-order terms.
__global__ void pixel_norm_bwd2_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ g,
                                       size_t npix, int c, int lanes, float eps, float* __restrict__ d_x) {
    const size_t gid = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t pix = gid / lanes;
    const int l = (int)(gid % lanes);
    const bool ok = pix < npix;
    const size_t base = (ok ? pix : 0) * (size_t)c;
    const float* xp = x + base;
    const float* dp = dy + base;
    const float* gp = g + base;
    float sxx = 0.f, sxd = 0.f, sxg = 0.f, sdg = 0.f;
    if (ok)
        for (int i = l; i < c; i += lanes) {
            const float xv = xp[i], dv = dp[i], gv = gp[i];
            sxx = fmaf(xv, xv, sxx);
            sxd = fmaf(xv, dv, sxd);
            sxg = fmaf(xv, gv, sxg);
            sdg = fmaf(dv, gv, sdg);
        }
    // all 64 lanes of the wave take part, those past the last pixel with zeros: a lane group never crosses a wave
    for (int m = lanes >> 1; m > 0; m >>= 1) {
        sxx += __shfl_xor(sxx, m);
        sxd += __shfl_xor(sxd, m);
        sxg += __shfl_xor(sxg, m);
        sdg += __shfl_xor(sdg, m);
    }
    if (!ok) return;
    const float fc = (float)c;
    const float r = rsqrtf(sxx / fc + eps);
    const float s = sxd / fc, t = sxg / fc, u = sdg / fc;
    const float r2 = r * r;
    const float r3 = r2 * r;
    const float k = (((3.f * r3) * r2) * s) * t;
    for (int i = l; i < c; i += lanes) {
        const float xv = xp[i];
        const float p = fmaf(t, dp[i], fmaf(s, gp[i], u * xv));
        d_x[base + i] = fmaf(k, xv, -(r3 * p));
    }
}

// The adjoint of max_pool_bwd_kernel (mpgan_elem.hip), which sends dy[b,oy,ox,ch] to position arg of its window: every
// output element reads the g at its arg position, out = g[b, s oy + a / k, s ox + a % k, ch].  A copy: no arithmetic on the
// value, no atomics, one thread per output element.  An arg byte outside the window (mpg_max_pool writes none) has no
// element to read and gives 0.
__global__ void max_pool_gather_kernel(const float* __restrict__ g, const unsigned char* __restrict__ arg, int n, int h, int w,
                                       int c, int k, int s, float* __restrict__ out) {
    const int oh = (h - k) / s + 1, ow = (w - k) / s + 1;
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t total = (size_t)n * oh * ow * c;
    if (idx >= total) return;
    const int ch = idx % c;
    size_t p = idx / c;
    const int ox = p % ow; p /= ow;
    const int oy = p % oh;
    const int b = p / oh;
    const int at = arg[idx];
    out[idx] = at < k * k ? g[(((size_t)b * h + (size_t)s * oy + at / k) * w + (size_t)s * ox + at % k) * c + ch] : 0.f;
}

// nearest upsample by integer factors: dx[iy,ix] = sum of the fy x fx block of dy
__global__ void resize_nearest_bwd_kernel(const float* __restrict__ dy, int n, int oh, int ow, int c,
                                          float* __restrict__ dx, int h, int w, float scale) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t total = (size_t)n * h * w * c;
    if (idx >= total) return;
    const int ch = idx % c;
    size_t p = idx / c;
    const int ix = p % w; p /= w;
    const int iy = p % h;
    const int b = p / h;
    const int fy = oh / h, fx = ow / w;
    float s = 0.f;
    for (int dyy = 0; dyy < fy; ++dyy)
        for (int dxx = 0; dxx < fx; ++dxx)
            s += dy[(((size_t)b * oh + iy * fy + dyy) * ow + ix * fx + dxx) * c + ch];
    dx[idx] = s * scale;
}

// One axis of the adjoint of the bilinear (METHOD 0) / bicubic (METHOD 2) resize: Y = R_h X R_w^T, so dX = R_h^T dY R_w, one
// launch per axis.  src is [outer, out, inner], dst [outer, in, inner]; a thread owns one dst element, source index i of the
// axis, and GATHERS: it walks the outputs o that can have a tap on i in ascending order, forms the forward's taps of o
// (mpgan_resize.h) and adds weight * src[o] for every tap whose clamped index is i -- at the borders two taps of one o can be.
// No scatter, no atomics, a fixed order: the same input gives the same bits.  An i that no output reads is written 0.
// The window [first, last] is integer arithmetic.  With e = floor(o * in / out) taken exactly, a tap i0 + t (t in LO .. HI) of o can
// be i only if i - HI <= i0 <= i - LO; clamping widens that only at i = 0 and i = in - 1, where the window is cut at 0 and
// out - 1 anyway.  The forward's i0 = floor(float32(o) * float32(in / out)) is within 1 of e, so e is in
// [i - HI - 1, i - LO + 1]: (i - HI - 1) * out / in <= o < (i - LO + 2) * out / in.  Only o in [0, out) is ever read.
template <int METHOD>
__global__ void resize_axis_bwd_kernel(const float* __restrict__ src, size_t outer, int out, int in, size_t inner,
                                       float scale, float* __restrict__ dst) {
    constexpr int T = METHOD == 0 ? 2 : 4, LO = METHOD == 0 ? 0 : -1, HI = METHOD == 0 ? 1 : 2;
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (idx >= outer * in * inner) return;
    const size_t k = idx % inner;
    const size_t p = idx / inner;
    const int i = (int)(p % in);
    const size_t b = p / in;
    const long long lo_num = (long long)(i - HI - 1) * out, hi_num = (long long)(i - LO + 2) * out;     // hi_num > 0
    const int first = lo_num > 0 ? (int)((lo_num + in - 1) / in) : 0;
    const long long past = (hi_num + in - 1) / in;
    const int last = past < out ? (int)past - 1 : out - 1;
    const float* col = src + b * out * inner + k;
    float s = 0.f;
    for (int o = first; o <= last; ++o) {
        int ti[T];
        float tw[T];
        if constexpr (METHOD == 0) bilinear_taps(o, scale, in, ti, tw);
        else bicubic_taps<true>(o, scale, in, ti, tw);
        const float v = col[(size_t)o * inner];
#pragma unroll
        for (int t = 0; t < T; ++t)
            if (ti[t] == i) s += tw[t] * v;
    }
    dst[idx] = s;
}

// 2x2 average pool backward: every input pixel receives a quarter of its output pixel
__global__ void avg_pool2_bwd_kernel(const float* __restrict__ dy, int n, int h, int w, int c,
                                     float* __restrict__ dx) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t total = (size_t)n * h * w * c;
    if (idx >= total) return;
    const int ch = idx % c;
    size_t p = idx / c;
    const int ix = p % w; p /= w;
    const int iy = p % h;
    const int b = p / h;
    const int oh = h / 2, ow = w / 2;
    const int oy = iy / 2, ox = ix / 2;
    dx[idx] = (oy < oh && ox < ow) ? 0.25f * dy[(((size_t)b * oh + oy) * ow + ox) * c + ch] : 0.f;
}

// out = x + (y - x) * t   (x may be null: zeros)
__global__ void lerp_kernel(const float* __restrict__ x, const float* __restrict__ y, size_t n, float t,
                            float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (idx >= n) return;
    const float a = x ? x[idx] : 0.f;
    out[idx] = a + (y[idx] - a) * t;
}

// out[0] += sum_i |a_i - b_i| (mode 0) or sum_i (a_i - b_i)^2 (mode 1); block partials, one atomic per block
__global__ __launch_bounds__(256) void pair_reduce_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          size_t n, int mode, float* __restrict__ out) {
    __shared__ float red[1][BLK];
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLK) {
        const float d = a[i] - (b ? b[i] : 0.f);
        s += mode == 0 ? fabsf(d) : d * d;
    }
    red[0][threadIdx.x] = s;
    block_tree_sum(red);
    if (threadIdx.x == 0) atomicAdd(out, red[0][0]);
}

// Double backward of GAN.minibatch_stddev_layer.  G members per group, M = n / G groups, K = h w c features; per (m, f):
// u = x - mean_g x, s_f = sqrt(mean_g u^2 + 1e-8).  Pass 1 (grid: slices x M): per group the block sums of
// D_m = sum over members and pixels of dy[.., c] and of sum_{g,f} ggx u / s_f, into `partials` ([m][block][2]);
// pass 2 adds them in block order; pass 3 is elementwise over (m, f) with a loop over the members.
constexpr int MBSTD2_MAX_BLOCKS = 256;
static_assert(MBSTD2_MAX_BLOCKS <= BLK, "mbstd_bwd2_finalize_kernel: one thread per block sum");
// `partials`, floats per group: MBSTD2_MAX_BLOCKS x 2 block sums ([m][block][2], rows of bx blocks), then, behind the block
// sums of all groups, the 2 statistics of pass 2 ([m][2])
constexpr int MBSTD2_FLOATS_PER_GROUP = 2 * MBSTD2_MAX_BLOCKS + 2;

__global__ __launch_bounds__(256) void mbstd_bwd2_sum_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ ggx, int g, int m, size_t npix_per,
                                                             int c, float* __restrict__ partials) {
    __shared__ float red[2][BLK];
    const int mi = blockIdx.y;
    const size_t hwc = npix_per * (size_t)c;
    const size_t stride = (size_t)gridDim.x * BLK;
    float t = 0.f, dsum = 0.f;
    for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < hwc; i += stride) {
        float mean = 0.f;
        for (int k = 0; k < g; ++k) mean += x[((size_t)k * m + mi) * hwc + i];
        mean /= (float)g;
        float var = 0.f, q = 0.f;
        for (int k = 0; k < g; ++k) {
            const size_t o = ((size_t)k * m + mi) * hwc + i;
            const float u = x[o] - mean;
            var = fmaf(u, u, var);
            q = fmaf(ggx[o], u, q);
        }
        t += q / sqrtf(var / (float)g + 1e-8f);
    }
    const size_t per_group = (size_t)g * npix_per;
    for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < per_group; i += stride) {
        const size_t k = i / npix_per, p = i - k * npix_per;
        dsum += dy[(((size_t)k * m + mi) * npix_per + p) * (c + 1) + c];
    }
    red[0][threadIdx.x] = dsum;
    red[1][threadIdx.x] = t;
    block_tree_sum(red);
    if (threadIdx.x == 0) {
        partials[((size_t)mi * gridDim.x + blockIdx.x) * 2] = red[0][0];
        partials[((size_t)mi * gridDim.x + blockIdx.x) * 2 + 1] = red[1][0];
    }
}

// stats[2 m] = D_m / (K G), stats[2 m + 1] = T_m = sum_{g,f} ggx u / (K G s_f); one block per group, the nblocks
// (<= BLK) block sums added in a fixed tree
__global__ __launch_bounds__(256) void mbstd_bwd2_finalize_kernel(const float* __restrict__ partials, int nblocks, float inv_kg,
                                                                  float* __restrict__ stats) {
    __shared__ float red[2][BLK];
    const int mi = blockIdx.x, b = threadIdx.x;
    red[0][b] = b < nblocks ? partials[((size_t)mi * nblocks + b) * 2] : 0.f;
    red[1][b] = b < nblocks ? partials[((size_t)mi * nblocks + b) * 2 + 1] : 0.f;
    block_tree_sum(red);
    if (b == 0) {
        stats[2 * mi] = red[0][0] * inv_kg;
        stats[2 * mi + 1] = red[1][0] * inv_kg;
    }
}

// g_x = D_m / (K G) ((ggx - mean_g ggx) / s_f - Q_f u / (G s_f^3)),  Q_f = sum_g ggx u;
// g_dy = (ggx, T_m) -- the statistic channel written by the thread of feature channel 0
__global__ void mbstd_bwd2_apply_kernel(const float* __restrict__ x, const float* __restrict__ ggx,
                                        const float* __restrict__ stats, int g, int m, size_t hwc, int c,
                                        float* __restrict__ g_x, float* __restrict__ g_dy) {
    const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
    const int mi = blockIdx.y;
    if (i >= hwc) return;
    float mx = 0.f, mg = 0.f;
    for (int k = 0; k < g; ++k) {
        const size_t o = ((size_t)k * m + mi) * hwc + i;
        mx += x[o];
        mg += ggx[o];
    }
    mx /= (float)g;
    mg /= (float)g;
    float var = 0.f, q = 0.f;
    for (int k = 0; k < g; ++k) {
        const size_t o = ((size_t)k * m + mi) * hwc + i;
        const float u = x[o] - mx;
        var = fmaf(u, u, var);
        q = fmaf(ggx[o], u, q);
    }
    const float is = 1.f / sqrtf(var / (float)g + 1e-8f);
    const float dk = stats[2 * mi], tm = stats[2 * mi + 1];
    const float qc = q * is * is * is / (float)g;
    const size_t pix = i / c;
    const int ch = (int)(i - pix * c);
    for (int k = 0; k < g; ++k) {
        const int nn = k * m + mi;
        const size_t o = (size_t)nn * hwc + i;
        const float gg = ggx[o];
        g_x[o] = dk * ((gg - mg) * is - qc * (x[o] - mx));
        const size_t oy = ((size_t)nn * (hwc / c) + pix) * (c + 1);
        g_dy[oy + ch] = gg;
        if (ch == 0) g_dy[oy + c] = tm;
    }
}

// The six means the test section forms from one critic output: logit, sigmoid, sigmoid cross entropy against label 1 and
// label 0 in TensorFlow's stable form max(l, 0) - l z + log1p(exp(-|l|)), and the LSGAN squares.  A critic output has one
// logit per tile, so ONE block covers it: every thread sums its strided share, the 256 sums are folded in a fixed tree.
// No atomics and nothing to clear: the same input gives the same bits, inside a captured graph too.
__global__ __launch_bounds__(256) void logit_stats_kernel(const float* __restrict__ l, size_t n, float inv_n,
                                                          float* __restrict__ out) {
    __shared__ float red[6][BLK];
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, comp[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (size_t i = threadIdx.x; i < n; i += BLK) {
        const float v = l[i];
        const float e = expf(-fabsf(v));                     // in (0, 1]
        const float soft = log1pf(e);
        const float pos = fmaxf(v, 0.f);
        const float t[6] = {v, (v >= 0.f ? 1.f : e) / (1.f + e),      // sigmoid(v) without overflow
                            pos - v + soft,                            // label 1
                            pos + soft,                                // label 0
                            (v - 1.f) * (v - 1.f), v * v};
#pragma unroll
        for (int k = 0; k < 6; ++k) {                         // compensated: a long vector costs a thread hundreds of terms
            const float yk = t[k] - comp[k];
            const float sk = s[k] + yk;
            comp[k] = (sk - s[k]) - yk;
            s[k] = sk;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k][threadIdx.x] = s[k];
    block_tree_sum(red);
    if (threadIdx.x < 6) out[threadIdx.x] = red[threadIdx.x][0] * inv_n;
}

// [tiles, th, tw, c] fp32 tiles -> count = tiles / (rows * cols) mosaics of rows x cols tiles, channel `ch`, as 8-bit grey:
// uint8(clip(v, 0, 1) * 255), truncated (savePngsGrayscale).  QUAD: tw % 4 == 0, a thread packs four pixels of one tile
// row into one 32-bit store; otherwise one byte per thread.
__device__ __forceinline__ unsigned gray8(float v) { return (unsigned)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

template <bool QUAD>
__global__ void tiles_to_gray8_kernel(const float* __restrict__ tiles, size_t total, int th, int tw, int c, int ch, int rows,
                                      int cols, unsigned char* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (idx >= total) return;
    const size_t o = QUAD ? idx * 4 : idx;                      // first output byte of this thread
    const size_t W = (size_t)cols * tw, H = (size_t)rows * th;
    const size_t X = o % W, Y = (o / W) % H, m = o / (W * H);
    const size_t tile = (m * rows + Y / th) * cols + X / tw;
    const float* src = tiles + (((tile * th + Y % th) * tw + X % tw) * c + ch);
    if (QUAD) {
        const unsigned p = gray8(src[0]) | (gray8(src[c]) << 8) | (gray8(src[2 * (size_t)c]) << 16) |
                           (gray8(src[3 * (size_t)c]) << 24);
        reinterpret_cast<unsigned*>(out)[idx] = p;
    }
    else
        out[idx] = (unsigned char)gray8(src[0]);
}

}  // namespace

extern "C" int mpg_act_bwd(mpg_stream_t stream, const float* dy, const float* y, size_t n, int act, float leak,
                           float* dx, float* amax) {
    MPG_REQUIRE(dy && y && dx, "mpg_act_bwd: null pointer");
    MPG_REQUIRE(act >= MPG_ACT_NONE && act <= MPG_ACT_TANH, "mpg_act_bwd: bad activation %d", act);
    if (amax != nullptr) {
        hipError_t e = mpg::zero_async(amax, sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) return mpg::hip_check(e, "mpg_act_bwd: zero");
    }
    if (n == 0) return MPG_OK;
    unsigned g = grid_for((n + 3) / 4);
    if (g > AMAX_GRID) g = AMAX_GRID;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(g), dim3(BLK), 0, (hipStream_t)stream, dy, y, n, act, leak, dx, (unsigned int*)amax);
    MPG_LAUNCH_CHECK("act_bwd_kernel");
}

extern "C" int mpg_pixel_norm_bwd(mpg_stream_t stream, const float* dy, const float* x, size_t npix, int c, float eps,
                                  float* dx) {
    MPG_REQUIRE(dy && x && dx, "mpg_pixel_norm_bwd: null pointer");
    MPG_REQUIRE(npix >= 1 && c >= 1, "mpg_pixel_norm_bwd: bad shape");
    int lanes = 1;
    while (lanes * 2 <= c && lanes < 64) lanes <<= 1;
    hipLaunchKernelGGL(pixel_norm_bwd_kernel, dim3(grid_for(npix * lanes)), dim3(BLK), 0, (hipStream_t)stream, dy, x, npix,
                       c, lanes, eps, dx);
    MPG_LAUNCH_CHECK("pixel_norm_bwd_kernel");
}

extern "C" int mpg_act_bwd2(mpg_stream_t stream, const float* dy, const float* y, const float* g, size_t n, int act,
                            float leak, float* d_y) {
    (void)leak;
    MPG_REQUIRE(dy && y && g && d_y, "mpg_act_bwd2: null pointer");
    MPG_REQUIRE(act == MPG_ACT_TANH, "mpg_act_bwd2: activation %d has no second derivative in y (tanh only)", act);
    if (n == 0) return MPG_OK;
    size_t blocks = ((n + 3) / 4 + BLK - 1) / BLK;
    if (blocks > ACT_BWD2_GRID) blocks = ACT_BWD2_GRID;
    hipLaunchKernelGGL(act_bwd2_tanh_kernel, dim3((unsigned)blocks), dim3(BLK), 0, (hipStream_t)stream, dy, y, g, n, d_y);
    MPG_LAUNCH_CHECK("act_bwd2_tanh_kernel");
}

extern "C" int mpg_pixel_norm_bwd2(mpg_stream_t stream, const float* dy, const float* x, const float* g, size_t npix, int c,
                                   float eps, float* d_x) {
    MPG_REQUIRE(dy && x && g && d_x, "mpg_pixel_norm_bwd2: null pointer");
    MPG_REQUIRE(npix >= 1 && c >= 1, "mpg_pixel_norm_bwd2: bad shape");
    int lanes = 1;
    while (lanes * 2 <= c && lanes < 64) lanes <<= 1;
    MPG_REQUIRE(npix <= ((size_t)0x7fffffff * BLK) / lanes, "mpg_pixel_norm_bwd2: %zu pixels are more than one grid takes", npix);
    hipLaunchKernelGGL(pixel_norm_bwd2_kernel, dim3(grid_for(npix * lanes)), dim3(BLK), 0, (hipStream_t)stream, dy, x, g, npix,
                       c, lanes, eps, d_x);
    MPG_LAUNCH_CHECK("pixel_norm_bwd2_kernel");
}

extern "C" int mpg_max_pool_gather(mpg_stream_t stream, const float* g, const unsigned char* arg, int n, int h, int w, int c,
                                   int k, int s, float* out) {
    MPG_REQUIRE(g && arg && out, "mpg_max_pool_gather: null pointer");
    MPG_REQUIRE(n >= 1 && c >= 1 && k >= 1 && k <= 15 && s >= 1 && h >= k && w >= k, "mpg_max_pool_gather: bad shape");
    const size_t total = (size_t)n * ((h - k) / s + 1) * ((w - k) / s + 1) * c;
    MPG_REQUIRE(total <= (size_t)0x7fffffff * BLK, "mpg_max_pool_gather: %zu outputs are more than one grid takes", total);
    hipLaunchKernelGGL(max_pool_gather_kernel, dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, g, arg, n, h, w, c, k,
                       s, out);
    MPG_LAUNCH_CHECK("max_pool_gather_kernel");
}

extern "C" int mpg_resize_nearest_bwd(mpg_stream_t stream, const float* dy, int n, int oh, int ow, int c, float* dx,
                                      int h, int w) {
    MPG_REQUIRE(dy && dx, "mpg_resize_nearest_bwd: null pointer");
    MPG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1 && oh >= h && ow >= w, "mpg_resize_nearest_bwd: bad shape");
    MPG_REQUIRE(oh % h == 0 && ow % w == 0, "mpg_resize_nearest_bwd: only integer factors (%dx%d -> %dx%d)", h, w, oh, ow);
    const size_t total = (size_t)n * h * w * c;
    hipLaunchKernelGGL(resize_nearest_bwd_kernel, dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, dy, n, oh,
                       ow, c, dx, h, w, 1.f);
    MPG_LAUNCH_CHECK("resize_nearest_bwd_kernel");
}

// dy [n,oh,ow,c] -> tmp [n,h,ow,c] along H -> dx [n,h,w,c] along W; the scales are the forward's (float)in / (float)out
template <int METHOD>
static int resize_bwd(const char* name, mpg_stream_t stream, const float* dy, int n, int oh, int ow, int c, float* dx, int h,
                      int w, float* tmp) {
    MPG_REQUIRE(dy && dx && tmp, "%s: null pointer", name);
    MPG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1 && oh >= 1 && ow >= 1, "%s: bad shape", name);
    const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
    const size_t rows = (size_t)n * h, inner_h = (size_t)ow * c;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((resize_axis_bwd_kernel<METHOD>), dim3(grid_for(rows * inner_h)), dim3(BLK), 0, s, dy, (size_t)n, oh, h,
                       inner_h, sy, tmp);
    hipLaunchKernelGGL((resize_axis_bwd_kernel<METHOD>), dim3(grid_for(rows * w * c)), dim3(BLK), 0, s, (const float*)tmp, rows,
                       ow, w, (size_t)c, sx, dx);
    MPG_LAUNCH_CHECK(name);
}

extern "C" int mpg_resize_bilinear_bwd(mpg_stream_t stream, const float* dy, int n, int oh, int ow, int c, float* dx, int h,
                                       int w, float* tmp) {
    return resize_bwd<0>("mpg_resize_bilinear_bwd", stream, dy, n, oh, ow, c, dx, h, w, tmp);
}

extern "C" int mpg_resize_bicubic_bwd(mpg_stream_t stream, const float* dy, int n, int oh, int ow, int c, float* dx, int h,
                                      int w, float* tmp) {
    return resize_bwd<2>("mpg_resize_bicubic_bwd", stream, dy, n, oh, ow, c, dx, h, w, tmp);
}

extern "C" int mpg_avg_pool2_bwd(mpg_stream_t stream, const float* dy, int n, int h, int w, int c, float* dx) {
    MPG_REQUIRE(dy && dx, "mpg_avg_pool2_bwd: null pointer");
    MPG_REQUIRE(n >= 1 && h >= 2 && w >= 2 && c >= 1, "mpg_avg_pool2_bwd: bad shape");
    const size_t total = (size_t)n * h * w * c;
    hipLaunchKernelGGL(avg_pool2_bwd_kernel, dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, dy, n, h, w, c,
                       dx);
    MPG_LAUNCH_CHECK("avg_pool2_bwd_kernel");
}

extern "C" int mpg_lerp(mpg_stream_t stream, const float* x, const float* y, size_t n, float t, float* out) {
    MPG_REQUIRE(y && out, "mpg_lerp: null pointer");
    if (n == 0) return MPG_OK;
    hipLaunchKernelGGL(lerp_kernel, dim3(grid_for(n)), dim3(BLK), 0, (hipStream_t)stream, x, y, n, t, out);
    MPG_LAUNCH_CHECK("lerp_kernel");
}

extern "C" int mpg_pair_reduce(mpg_stream_t stream, const float* a, const float* b, size_t n, int mode, float* out) {
    MPG_REQUIRE(a && out, "mpg_pair_reduce: null pointer");
    MPG_REQUIRE(mode == 0 || mode == 1, "mpg_pair_reduce: mode %d", mode);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = mpg::zero_async(out, sizeof(float), s);
    if (e != hipSuccess) return mpg::hip_check(e, "mpg_pair_reduce: zero");
    if (n == 0) return MPG_OK;
    size_t blocks = (n + BLK * 8 - 1) / (BLK * 8);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(pair_reduce_kernel, dim3((unsigned)blocks), dim3(BLK), 0, s, a, b, n, mode, out);
    MPG_LAUNCH_CHECK("pair_reduce_kernel");
}

extern "C" int mpg_minibatch_stddev_bwd2(mpg_stream_t stream, const float* x, const float* dy, const float* ggx, int n, int h,
                                         int w, int c, int group_size, float* g_x, float* g_dy, float* partials,
                                         size_t partials_floats) {
    MPG_REQUIRE(x && dy && ggx && g_x && g_dy && partials, "mpg_minibatch_stddev_bwd2: null pointer");
    MPG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1 && group_size >= 1, "mpg_minibatch_stddev_bwd2: bad shape");
    const int g = group_size < n ? group_size : n;
    MPG_REQUIRE(n % g == 0, "mpg_minibatch_stddev_bwd2: batch %d is not divisible by the group size %d", n, g);
    const int m = n / g;
    MPG_REQUIRE(partials_floats >= (size_t)m * MBSTD2_FLOATS_PER_GROUP, "mpg_minibatch_stddev_bwd2: partials buffer too small");
    const size_t npix_per = (size_t)h * w, hwc = npix_per * c;
    hipStream_t s = (hipStream_t)stream;
    size_t span = hwc > (size_t)g * npix_per ? hwc : (size_t)g * npix_per;
    unsigned bx = (unsigned)((span + BLK * 4 - 1) / (BLK * 4));
    if (bx > MBSTD2_MAX_BLOCKS) bx = MBSTD2_MAX_BLOCKS;
    float* stats = partials + (size_t)m * 2 * MBSTD2_MAX_BLOCKS;
    hipLaunchKernelGGL(mbstd_bwd2_sum_kernel, dim3(bx, m), dim3(BLK), 0, s, x, dy, ggx, g, m, npix_per, c, partials);
    hipLaunchKernelGGL(mbstd_bwd2_finalize_kernel, dim3(m), dim3(BLK), 0, s, (const float*)partials, (int)bx,
                       1.f / ((float)hwc * (float)g), stats);
    hipLaunchKernelGGL(mbstd_bwd2_apply_kernel, dim3(grid_for(hwc), m), dim3(BLK), 0, s, x, ggx, (const float*)stats, g, m, hwc,
                       c, g_x, g_dy);
    MPG_LAUNCH_CHECK("mbstd backward-of-backward kernels");
}

extern "C" int mpg_logit_stats(mpg_stream_t stream, const float* logits, size_t n, float* out6) {
    MPG_REQUIRE(logits && out6, "mpg_logit_stats: null pointer");
    MPG_REQUIRE(n >= 1, "mpg_logit_stats: empty logit vector");
    hipLaunchKernelGGL(logit_stats_kernel, dim3(1), dim3(BLK), 0, (hipStream_t)stream, logits, n, 1.f / (float)n, out6);
    MPG_LAUNCH_CHECK("logit_stats_kernel");
}

extern "C" int mpg_tiles_to_gray8(mpg_stream_t stream, const float* tiles, int n_tiles, int th, int tw, int c, int channel,
                                  int rows, int cols, unsigned char* out) {
    MPG_REQUIRE(tiles && out, "mpg_tiles_to_gray8: null pointer");
    MPG_REQUIRE(n_tiles >= 1 && th >= 1 && tw >= 1 && c >= 1 && rows >= 1 && cols >= 1, "mpg_tiles_to_gray8: bad shape");
    MPG_REQUIRE(channel >= 0 && channel < c, "mpg_tiles_to_gray8: channel %d of %d", channel, c);
    MPG_REQUIRE(n_tiles % (rows * cols) == 0, "mpg_tiles_to_gray8: %d tiles do not fill %d x %d mosaics", n_tiles, rows, cols);
    const size_t bytes = (size_t)n_tiles * th * tw;
    hipStream_t s = (hipStream_t)stream;
    if ((tw % 4) == 0 && (((uintptr_t)out) & 3) == 0)
        hipLaunchKernelGGL((tiles_to_gray8_kernel<true>), dim3(grid_for(bytes / 4)), dim3(BLK), 0, s, tiles, bytes / 4, th, tw, c,
                           channel, rows, cols, out);
    else
        hipLaunchKernelGGL((tiles_to_gray8_kernel<false>), dim3(grid_for(bytes)), dim3(BLK), 0, s, tiles, bytes, th, tw, c,
                           channel, rows, cols, out);
    MPG_LAUNCH_CHECK("tiles_to_gray8_kernel");
}
