// Batch norm with batch statistics on the vector ALUs, fp32 NHWC: the shift and the per-channel sums over pixels (block
// sums kept and added in a fixed order, mpgan_valu.h), the normalisation with activation -- the same kernels serve the
// training forward, inference and held-out evaluation (mpg_bn_infer_act), which can write the G8 form of its output as
// well --, the backward pass and the backward of the backward pass (WGAN-GP through batch norm).
// Entries: mpg_channel_sum_ordered, mpg_bn_partials_floats, mpg_bn_train_fwd_ordered, mpg_bn_train_bwd_ordered,
// mpg_bn_train_bwd2_ordered, mpg_bn_infer_act.
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

// ---------------------------------------------------------------- per-channel sums over pixels
// MODE 0: sum x
// MODE 2: sum a, sum a*(x - mean)*invstd  (a = dy; two outputs)
// MODE 3: sum (x - k), sum (x - k)^2 with k = aux0[ch], the shift bn_shift_kernel took from the tensor: both batch moments
//         in ONE pass over x.  With k within a fraction of sigma of the mean, var = E[(x-k)^2] - E[x-k]^2 loses nothing to
//         cancellation.  k = the first pixel's value did (a border pixel can sit many sigma away, and the gradients through
//         the normalisation felt it); so did the mean of four pixels when all four were such pixels: the variance error
//         grows with 1 + ((k - mean) / sigma)^2.
// k[ch] = the channel's mean over BN_SHIFT_PIX pixels spread evenly through the batch (every pixel once when there are
// fewer), added in pixel order: a few outliers among them move k by a fraction of sigma only.  A block takes four
// channels: one thread per (pixel, channel) loads, so the 64 loads of a channel are in flight together (one thread
// per channel walking them cost 6 us a call), then one thread per channel adds them.
constexpr int BN_SHIFT_PIX = 64;
static_assert(BN_SHIFT_PIX * 4 == BLK, "bn_shift_kernel: one thread per (pixel, channel of four)");

__global__ __launch_bounds__(256) void bn_shift_kernel(const float* __restrict__ x, size_t npix, int c, float* __restrict__ k) {
    __shared__ float samp[BN_SHIFT_PIX][4];
    const int cl = threadIdx.x & 3, j = threadIdx.x >> 2;
    const int ch = blockIdx.x * 4 + cl;
    const int ns = npix < (size_t)BN_SHIFT_PIX ? (int)npix : BN_SHIFT_PIX;
    if (j < ns && ch < c) samp[j][cl] = x[((size_t)j * npix / ns) * c + ch];
    __syncthreads();
    if (j == 0 && ch < c) {
        float s = 0.f;
        for (int i = 0; i < ns; ++i) s += samp[i][cl];
        k[ch] = s / (float)ns;
    }
}

// V channels per thread on the grid of split_pixels.  V = 1 keeps one pixel in flight per thread and moves 1.7 TB/s on a
// 128-channel tensor, one 4-byte load per dependent iteration; V = 4 (c % 4 == 0, 16-byte loads) keeps UN pixels in flight.
// Either way a thread adds its pixels in pixel order, then the thread of row 0 adds the rows in order.
template <int MODE, int V>
__global__ __launch_bounds__(256) void chan_sum_kernel(const float* __restrict__ a, const float* __restrict__ x, size_t npix,
                                                       int c, int lanes, const float* __restrict__ aux0,
                                                       const float* __restrict__ aux1, float eps, size_t pix_per_block,
                                                       float* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float red[2][BLK * V];
    const int tid = threadIdx.x;
    const int ppi = BLK / lanes;                 // pixels per iteration
    const int lane = tid % lanes, row = tid / lanes;
    const int ch = (blockIdx.y * lanes + lane) * V;
    const size_t p_begin = (size_t)blockIdx.x * pix_per_block;
    const size_t p_end = min(npix, p_begin + pix_per_block);
    float s0[V], s1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s0[j] = s1[j] = 0.f;
    if (ch < c) {
        float m[V], is[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            m[j] = is[j] = 0.f;
            if (MODE == 2) { m[j] = aux0[ch + j]; is[j] = rsqrtf(aux1[ch + j] + eps); }
            if (MODE == 3) m[j] = aux0[ch + j];
        }
        auto take = [&](const float (&v)[V], const float (&xv)[V]) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (MODE == 0) s0[j] += v[j];
                if (MODE == 2) { s0[j] += v[j]; s1[j] = fmaf(v[j], (xv[j] - m[j]) * is[j], s1[j]); }
                if (MODE == 3) { const float d = v[j] - m[j]; s0[j] += d; s1[j] = fmaf(d, d, s1[j]); }
            }
        };
        constexpr int UN = V == 1 ? 1 : (MODE == 2 ? 4 : 8);      // pixels in flight per thread
        size_t p = p_begin + row;
        for (; p + (UN - 1) * (size_t)ppi < p_end; p += UN * (size_t)ppi) {
            float v[UN][V], xv[UN][V];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                ldv<V>(a + (p + (size_t)u * ppi) * c + ch, v[u]);
                if (MODE == 2) ldv<V>(x + (p + (size_t)u * ppi) * c + ch, xv[u]);
                else
#pragma unroll
                    for (int j = 0; j < V; ++j) xv[u][j] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) take(v[u], xv[u]);
        }
        if constexpr (UN > 1)
            for (; p < p_end; p += ppi) {
                float v[V], xv[V];
                ldv<V>(a + p * c + ch, v);
                if (MODE == 2) ldv<V>(x + p * c + ch, xv);
                else
#pragma unroll
                    for (int j = 0; j < V; ++j) xv[j] = 0.f;
                take(v, xv);
            }
    }
    stv<V>(&red[0][tid * V], s0);
    stv<V>(&red[1][tid * V], s1);
    __syncthreads();
    if (row == 0 && ch < c) {
        for (int r = 1; r < ppi; ++r) {
            float u0[V], u1[V];
            ldv<V>(&red[0][(r * lanes + lane) * V], u0);
            ldv<V>(&red[1][(r * lanes + lane) * V], u1);
#pragma unroll
            for (int j = 0; j < V; ++j) { s0[j] += u0[j]; s1[j] += u1[j]; }
        }
        // the block's sums are kept; sum_partials_kernel adds them in block order
        float* pp = partials + ((size_t)blockIdx.x * c + ch) * 2;
#pragma unroll
        for (int j = 0; j < V; ++j) { pp[2 * j] = s0[j]; pp[2 * j + 1] = s1[j]; }
    }
}

constexpr int CHAN_SUM_MAX_BLOCKS = 1024;       // pixel blocks of either form (the size of a `partials` buffer: blocks x c x 2)

// returns the number of pixel blocks, the rows of `partials` written
template <int MODE>
int launch_chan_sum(hipStream_t s, const float* a, const float* x, size_t npix, int c, const float* aux0,
                    const float* aux1, float eps, float* partials) {
    const bool v4 = c >= 16 && (c % 4) == 0 && (((uintptr_t)a) & 15) == 0 && (x == nullptr || (((uintptr_t)x) & 15) == 0);
    const PixelSplit sp = split_pixels(npix, v4 ? c / 4 : c, v4 ? 512 : CHAN_SUM_MAX_BLOCKS);
    const auto kernel = v4 ? chan_sum_kernel<MODE, 4> : chan_sum_kernel<MODE, 1>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)sp.blocks, sp.cblocks), dim3(BLK), 0, s, a, x, npix, c, sp.lanes, aux0, aux1,
                       eps, sp.ppb, partials);
    return (int)sp.blocks;
}

// The ordered form of the sums: the blocks' partial sums ([block][channel][2]) added in the fixed order of
// ordered_partials_sum.
// BN_FWD: the two sums are those of MODE 3 around the shift k that out0 holds on entry; the kernel leaves the batch mean
// (sum0 / n + k) and the biased variance (sum1 / n - (sum0 / n)^2) in out0 / out1 and advances the moving averages of
// tf.contrib batch_norm (moving = decay * moving + (1 - decay) * batch) when their pointers are given
template <bool BN_FWD>
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ partials, int nblocks, int c,
                                                           float* out0, float* __restrict__ out1, float inv_n,
                                                           float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                           float decay) {
    int ch;
    float S[2];
    if (!ordered_partials_sum<2>(partials, nblocks, c, ch, S)) return;
    float s0 = S[0], s1 = S[1];
    if (BN_FWD) {
        const float m = s0 * inv_n;
        s1 = fmaxf(s1 * inv_n - m * m, 0.f);
        s0 = m + out0[ch];
        if (moving_mean) moving_mean[ch] = decay * moving_mean[ch] + (1.f - decay) * s0;
        if (moving_var) moving_var[ch] = decay * moving_var[ch] + (1.f - decay) * s1;
    }
    out0[ch] = s0;
    out1[ch] = s1;
}

// mean, rsqrt(var + eps), gamma, beta of every channel in LDS (c <= BN4_CMAX)
__device__ __forceinline__ void stage_bn_vectors(float (&par)[4][BN4_CMAX], int c, const float* __restrict__ mean,
                                                 const float* __restrict__ var, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float eps) {
    stage_channel_vectors<4>(par, c, [&](int k, int i) {
        return k == 0 ? mean[i] : k == 1 ? rsqrtf(var[i] + eps) : k == 2 ? gamma[i] : beta[i];
    });
}

// y = act((x - mean) * rsqrt(var + eps) * gamma + beta).  V = 1: one thread per element.  V = 4 (c % 4 == 0, c <= BN4_CMAX):
// the per-channel vectors staged in LDS and every thread streams 16 bytes of x per step of a grid-stride loop
template <int V>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, size_t totalv, int c,
                                                       const float* __restrict__ mean, const float* __restrict__ var,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       int act, float leak, float* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) float par[V == 4 ? 4 : 1][V == 4 ? BN4_CMAX : 1];
    if constexpr (V == 4) stage_bn_vectors(par, c, mean, var, gamma, beta, eps);
    for (size_t iv = (size_t)blockIdx.x * BLK + threadIdx.x; iv < totalv; iv += (size_t)gridDim.x * BLK) {
        const size_t e = iv * V;
        const int ch = (int)(e % (size_t)c);
        float v[V], q[4][V], o[V];
        ldv<V>(x + e, v);
        if constexpr (V == 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ldv<V>(&par[k][ch], q[k]);
        } else {
            q[0][0] = mean[ch]; q[1][0] = rsqrtf(var[ch] + eps); q[2][0] = gamma[ch]; q[3][0] = beta[ch];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = mpg::apply_act((v[j] - q[0][j]) * q[1][j] * q[2][j] + q[3][j], act, leak);
        stv<V>(y + e, o);
    }
}

// the float4 form when the tensor allows it; what mpg_bn_train_fwd_ordered applies after its statistics and what
// mpg_bn_infer_act applies with given vectors
void launch_bn_apply(hipStream_t s, const float* x, size_t total, int c, const float* mean, const float* var,
                     const float* gamma, const float* beta, float eps, int act, float leak, float* y) {
    if ((c % 4) == 0 && c <= BN4_CMAX && ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0) {
        unsigned g = grid_for(total / 4);
        if (g > 4096) g = 4096;
        hipLaunchKernelGGL(bn_apply_kernel<4>, dim3(g), dim3(BLK), 0, s, x, total / 4, c, mean, var, gamma, beta, eps, act,
                           leak, y);
    }
    else
        hipLaunchKernelGGL(bn_apply_kernel<1>, dim3(grid_for(total)), dim3(BLK), 0, s, x, total, c, mean, var, gamma, beta,
                           eps, act, leak, y);
}

// dx = gamma * invstd * (dy - dbeta/N - xhat * dgamma/N)
__global__ void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, size_t total, int c,
                                    const float* __restrict__ mean, const float* __restrict__ var,
                                    const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                    const float* __restrict__ dbeta, float eps, float inv_n, float* __restrict__ dx,
                                    unsigned int* __restrict__ amax) {
    float m = 0.f;
    for (size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BLK) {
        const int ch = idx % c;
        const float is = rsqrtf(var[ch] + eps);
        const float xh = (x[idx] - mean[ch]) * is;
        const float v = gamma[ch] * is * (dy[idx] - dbeta[ch] * inv_n - xh * dgamma[ch] * inv_n);
        dx[idx] = v;
        m = fmaxf(m, fabsf(v));
    }
    if (amax != nullptr) block_absmax_to(m, amax);
}

// ---------------------------------------------------------------- second derivative (WGAN-GP through batch norm)
// Double backward of training-mode batch norm.  Per channel over the M pixels, x^ = (x - mean) r, r = rsqrt(var + eps):
// one reduction pass for the five sums Sdz, Sdzx (= dbeta, dgamma of the first backward), Sg, Sgx, Sgdz; the blocks' sums go
// to `partials` ([block][channel][5]) and bn_bwd2_finalize_kernel adds them in block order (no atomics), then folds them with
// gamma, gdgamma, gdbeta into eight per-channel coefficients of the elementwise pass and writes g_gamma.
constexpr int BN2_NS = 5;
constexpr int BN2_MAX_BLOCKS = 256;
constexpr int BN2_NCOEF = 9;                    // mean, r, then g_dz = a0 gdx + a1 + a2 x^, g_x = b0 x^ + b1 gdx + b2 dz + b3

// V channels per thread (V = 4: c % 4 == 0 and 16-byte aligned tensors); `lanes` threads across the channels, BLK / lanes
// pixel rows; block x = one slice of the pixel range, block y = one group of lanes * V channels
template <int V>
__global__ __launch_bounds__(256) void bn_bwd2_sum_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                          const float* __restrict__ gdx, size_t npix, int c, int lanes,
                                                          const float* __restrict__ mean, const float* __restrict__ var,
                                                          float eps, size_t pix_per_block, float* __restrict__ partials) {
    __shared__ float red[BN2_NS][BLK * V];
    const int tid = threadIdx.x;
    const int ppi = BLK / lanes;
    const int lane = tid % lanes, row = tid / lanes;
    const int ch = (blockIdx.y * lanes + lane) * V;
    const size_t p_begin = (size_t)blockIdx.x * pix_per_block;
    const size_t p_end = min(npix, p_begin + pix_per_block);
    float s[BN2_NS][V];
#pragma unroll
    for (int k = 0; k < BN2_NS; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) s[k][j] = 0.f;
    if (ch < c) {
        float m[V], r[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { m[j] = mean[ch + j]; r[j] = rsqrtf(var[ch + j] + eps); }
        for (size_t p = p_begin + row; p < p_end; p += ppi) {
            float d[V], xv[V], g[V];
            ldv<V>(dz + p * c + ch, d);
            ldv<V>(x + p * c + ch, xv);
            if (gdx != nullptr) ldv<V>(gdx + p * c + ch, g);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float xh = (xv[j] - m[j]) * r[j];
                s[0][j] += d[j];
                s[1][j] = fmaf(d[j], xh, s[1][j]);
                if (gdx != nullptr) {
                    s[2][j] += g[j];
                    s[3][j] = fmaf(g[j], xh, s[3][j]);
                    s[4][j] = fmaf(g[j], d[j], s[4][j]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < BN2_NS; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) red[k][tid * V + j] = s[k][j];
    __syncthreads();
    if (row == 0 && ch < c) {
        for (int rr = 1; rr < ppi; ++rr)            // rows added in order: the block's sums do not depend on timing
#pragma unroll
            for (int k = 0; k < BN2_NS; ++k)
#pragma unroll
                for (int j = 0; j < V; ++j) s[k][j] += red[k][(rr * lanes + lane) * V + j];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (ch + j >= c) break;
            float* pp = partials + ((size_t)blockIdx.x * c + ch + j) * BN2_NS;
#pragma unroll
            for (int k = 0; k < BN2_NS; ++k) pp[k] = s[k][j];
        }
    }
}

// the five sums in the fixed order of ordered_partials_sum, then the coefficients
__global__ __launch_bounds__(256) void bn_bwd2_finalize_kernel(const float* __restrict__ partials, int nblocks, int c,
                                                               float inv_n, const float* __restrict__ mean,
                                                               const float* __restrict__ var, float eps,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ gdgamma,
                                                               const float* __restrict__ gdbeta, float* __restrict__ coef,
                                                               float* __restrict__ g_gamma) {
    int ch;
    float S[BN2_NS];
    if (!ordered_partials_sum<BN2_NS>(partials, nblocks, c, ch, S)) return;
    const float sdz = S[0], sdzx = S[1], sg = S[2], sgx = S[3], sgdz = S[4];
    const float r = rsqrtf(var[ch] + eps), gm = gamma[ch];
    const float gdg = gdgamma != nullptr ? gdgamma[ch] : 0.f, gdb = gdbeta != nullptr ? gdbeta[ch] : 0.f;
    const float A = sgdz - sg * sdz * inv_n;
    const float gr = gm * r, k = gm * r * r * inv_n;
    g_gamma[ch] = r * (A - sgx * sdzx * inv_n);
    coef[0 * (size_t)c + ch] = mean[ch];
    coef[1 * (size_t)c + ch] = r;
    coef[2 * (size_t)c + ch] = gr;                                                   // a0
    coef[3 * (size_t)c + ch] = gdb - gr * sg * inv_n;                               // a1
    coef[4 * (size_t)c + ch] = gdg - gr * sgx * inv_n;                              // a2
    coef[5 * (size_t)c + ch] = k * (3.f * sgx * sdzx * inv_n - A) - gdg * r * sdzx * inv_n;   // b0
    coef[6 * (size_t)c + ch] = -k * sdzx;                                            // b1
    coef[7 * (size_t)c + ch] = gdg * r - k * sgx;                                    // b2
    coef[8 * (size_t)c + ch] = k * (sdzx * sg + sgx * sdz) * inv_n - gdg * r * sdz * inv_n;   // b3
}

// g_dz = a0 gdx + a1 + a2 x^,  g_x = b0 x^ + b1 gdx + b2 dz + b3.  V = 4: the coefficients staged in LDS (c <= BN4_CMAX)
template <int V>
__global__ __launch_bounds__(256) void bn_bwd2_apply_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                            const float* __restrict__ gdx, size_t totalv, int c,
                                                            const float* __restrict__ coef, float* __restrict__ g_dz,
                                                            float* __restrict__ g_x) {
    __shared__ __attribute__((aligned(16))) float par[V == 4 ? BN2_NCOEF : 1][V == 4 ? BN4_CMAX : 1];
    if constexpr (V == 4) stage_channel_vectors<BN2_NCOEF>(par, c, [&](int k, int i) { return coef[(size_t)k * c + i]; });
    for (size_t iv = (size_t)blockIdx.x * BLK + threadIdx.x; iv < totalv; iv += (size_t)gridDim.x * BLK) {
        const size_t e = iv * V;
        const int ch = (int)(e % (size_t)c);
        float d[V], xv[V], g[V], q[BN2_NCOEF][V];
        ldv<V>(dz + e, d);
        ldv<V>(x + e, xv);
        if (gdx != nullptr) ldv<V>(gdx + e, g);
        else
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] = 0.f;
#pragma unroll
        for (int k = 0; k < BN2_NCOEF; ++k) {
            if constexpr (V == 4) ldv<V>(&par[k][ch], q[k]);
            else q[k][0] = coef[(size_t)k * c + ch];
        }
        float od[V], ox[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float xh = (xv[j] - q[0][j]) * q[1][j];
            od[j] = fmaf(q[2][j], g[j], fmaf(q[4][j], xh, q[3][j]));
            ox[j] = fmaf(q[5][j], xh, fmaf(q[6][j], g[j], fmaf(q[7][j], d[j], q[8][j])));
        }
        stv<V>(g_dz + e, od);
        stv<V>(g_x + e, ox);
    }
}

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

// y = act((x - mean) * rsqrt(var + eps) * gamma + beta) with the G8 form of y written by the same thread from the same
// registers (the next convolution reads it; no mpg_f32_to_g8 pass over y).  One thread per (pixel, group of 8 channels),
// groups fastest: a pixel row is read as consecutive 32-byte pieces.  The per-channel vectors are staged in LDS as
// bn_apply_kernel<4> does (c <= BN4_CMAX; wider tensors read them from memory).  VEC: c % 4 == 0 and 16-byte aligned x / y.
template <bool VEC>
__global__ __launch_bounds__(256) void bn_infer_g8_kernel(const float* __restrict__ x, int n, size_t plane_px, int c,
                                                          const float* __restrict__ mean, const float* __restrict__ var,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, int act, float leak, float* __restrict__ y,
                                                          _Float16* __restrict__ g8) {
    __shared__ __attribute__((aligned(16))) float par[4][BN4_CMAX];
    const bool staged = c <= BN4_CMAX;
    if (staged) stage_bn_vectors(par, c, mean, var, gamma, beta, eps);
    const int cg_n = (c + 7) >> 3;
    const size_t total = (size_t)n * plane_px * cg_n;
    for (size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BLK) {
        const int cg = (int)(idx % cg_n);
        const size_t pix = idx / cg_n;                         // b * plane_px + px
        const size_t b = pix / plane_px, px = pix % plane_px;
        const int ch0 = cg * 8;
        const float* src = x + pix * c + ch0;
        float v[8];
        if (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(src);
            const float4 z = ch0 + 4 < c ? *reinterpret_cast<const float4*>(src + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = z.x; v[5] = z.y; v[6] = z.z; v[7] = z.w;
        }
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ch0 + j < c ? src[j] : 0.f;
        }
        float o[8];
        half8_t hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ch = ch0 + j;
            float r = 0.f;
            if (ch < c) {
                const float m = staged ? par[0][ch] : mean[ch], is = staged ? par[1][ch] : rsqrtf(var[ch] + eps);
                const float g = staged ? par[2][ch] : gamma[ch], bt = staged ? par[3][ch] : beta[ch];
                r = mpg::apply_act((v[j] - m) * is * g + bt, act, leak);
            }
            o[j] = r;
            hi[j] = (_Float16)r;
            lo[j] = (_Float16)(r - (float)hi[j]);
        }
        if (y != nullptr) {
            float* dst = y + pix * c + ch0;
            if (VEC) {
                *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
                if (ch0 + 4 < c) *reinterpret_cast<float4*>(dst + 4) = make_float4(o[4], o[5], o[6], o[7]);
            }
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (ch0 + j < c) dst[j] = o[j];
            }
        }
        _Float16* gd = g8 + (((b * cg_n + cg) * 2) * plane_px + px) * 8;
        *reinterpret_cast<half8_t*>(gd) = hi;
        *reinterpret_cast<half8_t*>(gd + plane_px * 8) = lo;
    }
}

}  // namespace

// One `partials` buffer serves every pass.  Floats per channel: the channel sums keep CHAN_SUM_MAX_BLOCKS x 2 block sums;
// the second derivative keeps BN2_MAX_BLOCKS x BN2_NS block sums and, behind them, its BN2_NCOEF coefficients.
constexpr int BN_PARTIALS_PER_CHANNEL = CHAN_SUM_MAX_BLOCKS * 2;
static_assert(BN2_MAX_BLOCKS * BN2_NS + BN2_NCOEF <= BN_PARTIALS_PER_CHANNEL,
              "mpg_bn_partials_floats: the buffer must hold the second derivative's block sums and coefficients");

extern "C" size_t mpg_bn_partials_floats(int c) { return c >= 1 ? (size_t)BN_PARTIALS_PER_CHANNEL * c : 0; }

// per-channel sum over pixels; the blocks' sums are kept in `partials` (mpg_bn_partials_floats(c) + c floats: the second
// float of a pair receives a copy) and added in a fixed order
extern "C" int mpg_channel_sum_ordered(mpg_stream_t stream, const float* x, size_t npix, int c, float* out, float* partials,
                                       size_t partials_floats) {
    MPG_REQUIRE(x && out && partials, "mpg_channel_sum_ordered: null pointer");
    MPG_REQUIRE(npix >= 1 && c >= 1, "mpg_channel_sum_ordered: bad shape");
    MPG_REQUIRE(partials_floats >= (size_t)BN_PARTIALS_PER_CHANNEL * c + (size_t)c, "mpg_channel_sum_ordered: partials buffer too small");
    hipStream_t s = (hipStream_t)stream;
    float* spare = partials + (size_t)BN_PARTIALS_PER_CHANNEL * c;      // sum_partials_kernel writes two vectors: the second goes here
    const int nb = launch_chan_sum<0>(s, x, nullptr, npix, c, nullptr, nullptr, 0.f, partials);
    hipLaunchKernelGGL(sum_partials_kernel<false>, dim3((c + 15) / 16), dim3(BLK), 0, s, (const float*)partials, nb, c, out, spare,
                       0.f, (float*)nullptr, (float*)nullptr, 0.f);
    MPG_LAUNCH_CHECK("chan_sum_kernel (ordered)");
}

extern "C" int mpg_bn_train_fwd_ordered(mpg_stream_t stream, const float* x, size_t npix, int c, const float* gamma,
                                        const float* beta, float eps, int act, float leak, float* y, float* batch_mean,
                                        float* batch_var, float* moving_mean, float* moving_var, float decay, float* partials,
                                        size_t partials_floats) {
    MPG_REQUIRE(x && gamma && beta && y && batch_mean && batch_var, "mpg_bn_train_fwd_ordered: null pointer");
    MPG_REQUIRE(npix >= 1 && c >= 1, "mpg_bn_train_fwd_ordered: bad shape");
    MPG_REQUIRE(act >= MPG_ACT_NONE && act <= MPG_ACT_TANH, "mpg_bn_train_fwd_ordered: bad activation %d", act);
    MPG_REQUIRE(partials != nullptr && partials_floats >= mpg_bn_partials_floats(c), "mpg_bn_train_fwd_ordered: partials buffer too small");
    hipStream_t s = (hipStream_t)stream;
    const float inv_n = 1.f / (float)npix;
    // the shift waits in batch_mean until sum_partials_kernel, which writes every sum (nothing to clear), replaces it
    hipLaunchKernelGGL(bn_shift_kernel, dim3((c + 3) / 4), dim3(BLK), 0, s, x, npix, c, batch_mean);
    const int nb = launch_chan_sum<3>(s, x, nullptr, npix, c, batch_mean, nullptr, 0.f, partials);
    hipLaunchKernelGGL(sum_partials_kernel<true>, dim3((c + 15) / 16), dim3(BLK), 0, s, (const float*)partials, nb, c, batch_mean,
                       batch_var, inv_n, moving_mean, moving_var, decay);
    launch_bn_apply(s, x, npix * c, c, batch_mean, batch_var, gamma, beta, eps, act, leak, y);
    MPG_LAUNCH_CHECK("bn_train_fwd_ordered");
}

extern "C" int mpg_bn_train_bwd_ordered(mpg_stream_t stream, const float* dy, const float* x, size_t npix, int c,
                                        const float* batch_mean, const float* batch_var, const float* gamma, float eps,
                                        float* dx, float* dgamma, float* dbeta, float* amax, float* partials,
                                        size_t partials_floats) {
    MPG_REQUIRE(dy && x && batch_mean && batch_var && gamma && dx && dgamma && dbeta,
                "mpg_bn_train_bwd_ordered: null pointer");
    MPG_REQUIRE(npix >= 1 && c >= 1, "mpg_bn_train_bwd_ordered: bad shape");
    MPG_REQUIRE(partials != nullptr && partials_floats >= mpg_bn_partials_floats(c), "mpg_bn_train_bwd_ordered: partials buffer too small");
    hipStream_t s = (hipStream_t)stream;
    // sum_partials_kernel writes every sum: only the abs-max (an atomic maximum) is cleared
    if (amax != nullptr) {
        hipError_t e = mpg::zero_async(amax, sizeof(float), s);
        if (e != hipSuccess) return mpg::hip_check(e, "mpg_bn_train_bwd_ordered: memset");
    }
    const int nb = launch_chan_sum<2>(s, dy, x, npix, c, batch_mean, batch_var, eps, partials);
    // the blocks' sums in a fixed order (and no atomics queueing on 2 c addresses)
    hipLaunchKernelGGL(sum_partials_kernel<false>, dim3((c + 15) / 16), dim3(BLK), 0, s, (const float*)partials, nb, c, dbeta, dgamma,
                       0.f, (float*)nullptr, (float*)nullptr, 0.f);
    const size_t total = npix * c;
    unsigned g = grid_for(total);
    if (amax != nullptr && g > AMAX_GRID) g = AMAX_GRID;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(g), dim3(BLK), 0, s, dy, x, total, c, batch_mean,
                       batch_var, gamma, dgamma, dbeta, eps, 1.f / (float)npix, dx, (unsigned int*)amax);
    MPG_LAUNCH_CHECK("bn_train_bwd_ordered");
}

extern "C" int mpg_bn_train_bwd2_ordered(mpg_stream_t stream, const float* dz, const float* x, size_t npix, int c,
                                         const float* batch_mean, const float* batch_var, const float* gamma, float eps,
                                         const float* gdx, const float* gdgamma, const float* gdbeta, float* g_dz, float* g_x,
                                         float* g_gamma, float* partials, size_t partials_floats) {
    MPG_REQUIRE(dz && x && batch_mean && batch_var && gamma && g_dz && g_x && g_gamma && partials,
                "mpg_bn_train_bwd2_ordered: null pointer");
    MPG_REQUIRE(npix >= 1 && c >= 1, "mpg_bn_train_bwd2_ordered: bad shape");
    MPG_REQUIRE(partials_floats >= mpg_bn_partials_floats(c), "mpg_bn_train_bwd2_ordered: partials buffer too small");
    hipStream_t s = (hipStream_t)stream;
    float* coef = partials + (size_t)BN2_MAX_BLOCKS * c * BN2_NS;       // BN2_NCOEF * c floats behind the block sums
    const uintptr_t al = (uintptr_t)dz | (uintptr_t)x | (uintptr_t)gdx | (uintptr_t)g_dz | (uintptr_t)g_x;
    const bool v4 = (c % 4) == 0 && (al & 15) == 0;
    const PixelSplit sp = split_pixels(npix, v4 ? c / 4 : c, BN2_MAX_BLOCKS);
    hipLaunchKernelGGL(v4 ? bn_bwd2_sum_kernel<4> : bn_bwd2_sum_kernel<1>, dim3((unsigned)sp.blocks, sp.cblocks), dim3(BLK), 0, s,
                       dz, x, gdx, npix, c, sp.lanes, batch_mean, batch_var, eps, sp.ppb, partials);
    hipLaunchKernelGGL(bn_bwd2_finalize_kernel, dim3((c + 15) / 16), dim3(BLK), 0, s, (const float*)partials, (int)sp.blocks, c,
                       1.f / (float)npix, batch_mean, batch_var, eps, gamma, gdgamma, gdbeta, coef, g_gamma);
    const size_t total = npix * c;
    if (v4 && c <= BN4_CMAX) {
        unsigned g = grid_for(total / 4);
        if (g > 4096) g = 4096;
        hipLaunchKernelGGL(bn_bwd2_apply_kernel<4>, dim3(g), dim3(BLK), 0, s, dz, x, gdx, total / 4, c, (const float*)coef,
                           g_dz, g_x);
    } else {
        unsigned g = grid_for(total);
        if (g > 8192) g = 8192;
        hipLaunchKernelGGL(bn_bwd2_apply_kernel<1>, dim3(g), dim3(BLK), 0, s, dz, x, gdx, total, c, (const float*)coef, g_dz,
                           g_x);
    }
    MPG_LAUNCH_CHECK("bn_train_bwd2");
}

extern "C" int mpg_bn_infer_act(mpg_stream_t stream, const float* x, int n, int h, int w, int c, const float* mean,
                                const float* var, const float* gamma, const float* beta, float eps, int act, float leak,
                                float* y, void* y_g8) {
    MPG_REQUIRE(x && mean && var && gamma && beta && (y || y_g8), "mpg_bn_infer_act: null pointer");
    MPG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1, "mpg_bn_infer_act: bad shape");
    MPG_REQUIRE(act >= MPG_ACT_NONE && act <= MPG_ACT_TANH, "mpg_bn_infer_act: bad activation %d", act);
    hipStream_t s = (hipStream_t)stream;
    const size_t plane_px = (size_t)h * w;
    const uintptr_t al = (uintptr_t)x | (uintptr_t)y;
    const bool vec = (c % 4) == 0 && (al & 15) == 0;
    if (y_g8 == nullptr) {
        // the normalisation with given vectors is what the training forward applies after its statistics: the same kernels
        launch_bn_apply(s, x, (size_t)n * plane_px * c, c, mean, var, gamma, beta, eps, act, leak, y);
        MPG_LAUNCH_CHECK("mpg_bn_infer_act");
    }
    MPG_REQUIRE((((uintptr_t)y_g8) & 15) == 0, "mpg_bn_infer_act: y_g8 must be 16-byte aligned");
    unsigned g = grid_for((size_t)n * plane_px * ((c + 7) / 8));
    if (g > 4096) g = 4096;
    if (vec)
        hipLaunchKernelGGL((bn_infer_g8_kernel<true>), dim3(g), dim3(BLK), 0, s, x, n, plane_px, c, mean, var, gamma, beta, eps,
                           act, leak, y, (_Float16*)y_g8);
    else
        hipLaunchKernelGGL((bn_infer_g8_kernel<false>), dim3(g), dim3(BLK), 0, s, x, n, plane_px, c, mean, var, gamma, beta, eps,
                           act, leak, y, (_Float16*)y_g8);
    MPG_LAUNCH_CHECK("bn_infer_g8_kernel");
}
