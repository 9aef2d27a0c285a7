// Training companions of the convolution on the vector ALUs, fp32 NHWC: the weight gradient (register-tiled contraction
// over pixels, split over the pixel range, accumulated with fp32 atomics), the data gradient for strided / even-sized
// filters, and the fully connected layer (one block per row and 64 outputs; split over K with atomics when the
// contraction is long and the rows are few).  Entries: mpg_conv2d_wgrad, mpg_conv2d_dgrad, mpg_fc_forward.
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

struct ConvGeom {
    int n, h, w, cin, oh, ow, cout, kh, kw, sh, sw, pt, pl;
};

// ---------------------------------------------------------------- weight gradient
// dw[ky][kx][ci][co] += wscale * sum_p x[p shifted by (ky,kx)][ci] * dy[p][co]
// block = one tap, a (16*MI) x (16*NI) tile of (ci, co), one slice of the pixel range.
template <int MI, int NI>
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                    float* __restrict__ dw, ConvGeom g, float wscale,
                                                    int ci_tiles, int co_tiles, size_t pix_per_split) {
    constexpr int TM = 16 * MI, TN = 16 * NI, TK = 8;
    __shared__ float xs[TK][TM + 4];
    __shared__ float ds[TK][TN + 4];
    __shared__ long long xoff[TK];
    __shared__ long long doff[TK];

    int bid = blockIdx.x;
    const int co_t = bid % co_tiles; bid /= co_tiles;
    const int ci_t = bid % ci_tiles; bid /= ci_tiles;
    const int tap = bid;
    const int ky = tap / g.kw, kx = tap % g.kw;
    const int ci0 = ci_t * TM, co0 = co_t * TN;
    const size_t P = (size_t)g.n * g.oh * g.ow;
    const size_t p_begin = (size_t)blockIdx.y * pix_per_split;
    const size_t p_end = min(P, p_begin + pix_per_split);
    const int tid = threadIdx.x;
    const int ty = tid / 16, tx = tid % 16;

    float acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = 0.f;

    for (size_t p0 = p_begin; p0 < p_end; p0 += TK) {
        if (tid < TK) {
            const size_t p = p0 + tid;
            long long xo = -1, dofs = -1;
            if (p < p_end) {
                const int ox = (int)(p % g.ow);
                const size_t r = p / g.ow;
                const int oy = (int)(r % g.oh);
                const int b = (int)(r / g.oh);
                const int iy = oy * g.sh + ky - g.pt, ix = ox * g.sw + kx - g.pl;
                dofs = (long long)p * g.cout;
                if (iy >= 0 && iy < g.h && ix >= 0 && ix < g.w) xo = (((long long)b * g.h + iy) * g.w + ix) * g.cin;
            }
            xoff[tid] = xo;
            doff[tid] = dofs;
        }
        __syncthreads();
        for (int e = tid; e < TK * TM; e += BLK) {
            const int pp = e / TM, c = e % TM;
            const long long o = xoff[pp];
            xs[pp][c] = (o >= 0 && ci0 + c < g.cin) ? x[o + ci0 + c] : 0.f;
        }
        for (int e = tid; e < TK * TN; e += BLK) {
            const int pp = e / TN, c = e % TN;
            const long long o = doff[pp];
            ds[pp][c] = (o >= 0 && xoff[pp] >= 0 && co0 + c < g.cout) ? dy[o + co0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TK; ++k) {
            float a[MI], bq[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) a[i] = xs[k][ty * MI + i];
#pragma unroll
            for (int j = 0; j < NI; ++j) bq[j] = ds[k][tx * NI + j];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) acc[i][j] = fmaf(a[i], bq[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int ci = ci0 + ty * MI + i;
        if (ci >= g.cin) continue;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int co = co0 + tx * NI + j;
            if (co < g.cout && acc[i][j] != 0.f)
                atomicAdd(dw + ((size_t)tap * g.cin + ci) * g.cout + co, acc[i][j] * wscale);
        }
    }
}

template <int MI, int NI>
int launch_wgrad(hipStream_t s, const float* x, const float* dy, float* dw, const ConvGeom& g, float wscale) {
    constexpr int TM = 16 * MI, TN = 16 * NI;
    const int ci_tiles = (g.cin + TM - 1) / TM, co_tiles = (g.cout + TN - 1) / TN;
    const size_t tiles = (size_t)g.kh * g.kw * ci_tiles * co_tiles;
    const size_t P = (size_t)g.n * g.oh * g.ow;
    size_t split = (2048 + tiles - 1) / tiles;
    const size_t max_split = (P + 127) / 128;
    if (split > max_split) split = max_split;
    if (split < 1) split = 1;
    if (split > 65535) split = 65535;
    size_t pps = (P + split - 1) / split;
    pps = (pps + 7) & ~(size_t)7;
    split = (P + pps - 1) / pps;
    hipLaunchKernelGGL((wgrad_kernel<MI, NI>), dim3((unsigned)tiles, (unsigned)split), dim3(BLK), 0, s, x, dy, dw, g,
                       wscale, ci_tiles, co_tiles, pps);
    return 0;
}

inline int micro(int c) { return c > 64 ? 8 : c > 32 ? 4 : c > 16 ? 2 : 1; }

// ---------------------------------------------------------------- data gradient (any stride / filter)
// dx[b,iy,ix,ci] = wscale * sum_{ky,kx,co} dy[b,oy,ox,co] * w[ky,kx,ci,co],  oy*sh + ky - pt == iy
// wt is the filter with the channel axes swapped, [kh,kw,cout,cin]: the lanes of a wave (adjacent ci)
// read adjacent weights while dy[co] is a broadcast
__global__ void dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ dx,
                             ConvGeom g, float wscale) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t total = (size_t)g.n * g.h * g.w * g.cin;
    if (idx >= total) return;
    const int ci = idx % g.cin;
    size_t p = idx / g.cin;
    const int ix = p % g.w; p /= g.w;
    const int iy = p % g.h;
    const int b = p / g.h;
    float acc = 0.f;
    for (int ky = 0; ky < g.kh; ++ky) {
        const int ny = iy + g.pt - ky;
        if (ny < 0 || ny % g.sh) continue;
        const int oy = ny / g.sh;
        if (oy >= g.oh) continue;
        for (int kx = 0; kx < g.kw; ++kx) {
            const int nx = ix + g.pl - kx;
            if (nx < 0 || nx % g.sw) continue;
            const int ox = nx / g.sw;
            if (ox >= g.ow) continue;
            const float* dp = dy + (((size_t)b * g.oh + oy) * g.ow + ox) * g.cout;
            const float* wp = wt + (size_t)(ky * g.kw + kx) * g.cout * g.cin + ci;
            for (int co = 0; co < g.cout; ++co) acc = fmaf(dp[co], wp[(size_t)co * g.cin], acc);
        }
    }
    dx[idx] = acc * wscale;
}

// long contractions (the discriminator's flatten -> 1: k = 262144 at 256^2 tiles) with one block per row leave the chip
// empty (16 blocks, 320 us): split K over blockIdx.z, partial sums by atomics into a zeroed y, bias + activation after
__global__ __launch_bounds__(256) void fc_splitk_kernel(const float* __restrict__ x, const float* __restrict__ w, int k, int cout,
                                                        int kchunk, float wscale, float* __restrict__ y) {
    __shared__ float red[1][BLK];
    const int row = blockIdx.x, o0 = blockIdx.y * 64, tid = threadIdx.x;
    const int no = min(64, cout - o0);
    const int k0 = blockIdx.z * kchunk, k1 = min(k, k0 + kchunk);
    const float* xr = x + (size_t)row * k;
    if (no == 1) {
        float s = 0.f;
        for (int i = k0 + tid; i < k1; i += BLK) s = fmaf(xr[i], w[(size_t)i * cout + o0], s);
        red[0][tid] = s;
        block_tree_sum(red);
        if (tid == 0) atomicAdd(y + (size_t)row * cout + o0, red[0][0] * wscale);
        return;
    }
    const int o = tid % 64, kl = tid / 64;
    float s = 0.f;
    if (o < no)
        for (int i = k0 + kl; i < k1; i += 4) s = fmaf(xr[i], w[(size_t)i * cout + o0 + o], s);
    red[0][tid] = s;
    __syncthreads();
    if (kl == 0 && o < no)
        atomicAdd(y + (size_t)row * cout + o0 + o, (red[0][o] + red[0][64 + o] + red[0][128 + o] + red[0][192 + o]) * wscale);
}

__global__ void fc_finish_kernel(float* __restrict__ y, const float* __restrict__ bias, size_t n, int cout, int act, float leak) {
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (idx >= n) return;
    y[idx] = mpg::apply_act(y[idx] + (bias ? bias[idx % cout] : 0.f), act, leak);
}

// fully connected layer: y[r][o] = act(wscale * sum_k x[r][k] * w[k][o] + b[o]); one block per (row, 64 outputs),
// the K range is strided over the block and reduced through LDS
__global__ __launch_bounds__(256) void fc_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, int k, int cout, float wscale,
                                                     int act, float leak, float* __restrict__ y) {
    __shared__ float red[1][BLK];
    const int row = blockIdx.x;
    const int o0 = blockIdx.y * 64;
    const int no = min(64, cout - o0);
    const int tid = threadIdx.x;
    const float* xr = x + (size_t)row * k;
    if (no == 1) {
        float s = 0.f;
        for (int i = tid; i < k; i += BLK) s = fmaf(xr[i], w[(size_t)i * cout + o0], s);
        red[0][tid] = s;
        block_tree_sum(red);
        if (tid == 0) y[(size_t)row * cout + o0] = mpg::apply_act(red[0][0] * wscale + (bias ? bias[o0] : 0.f), act, leak);
        return;
    }
    // 4 k-lanes x 64 outputs
    const int o = tid % 64, kl = tid / 64;
    float s = 0.f;
    if (o < no)
        for (int i = kl; i < k; i += 4) s = fmaf(xr[i], w[(size_t)i * cout + o0 + o], s);
    red[0][tid] = s;
    __syncthreads();
    if (kl == 0 && o < no) {
        s = red[0][o] + red[0][64 + o] + red[0][128 + o] + red[0][192 + o];
        y[(size_t)row * cout + o0 + o] = mpg::apply_act(s * wscale + (bias ? bias[o0 + o] : 0.f), act, leak);
    }
}

int fill_geom(ConvGeom& g, int n, int h, int w, int cin, int cout, int kh, int kw, int sh, int sw) {
    g.n = n; g.h = h; g.w = w; g.cin = cin; g.cout = cout; g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw;
    g.oh = (h + sh - 1) / sh;
    g.ow = (w + sw - 1) / sw;
    int ph = (g.oh - 1) * sh + kh - h; if (ph < 0) ph = 0;
    int pw = (g.ow - 1) * sw + kw - w; if (pw < 0) pw = 0;
    g.pt = ph / 2;
    g.pl = pw / 2;
    return 0;
}

}  // namespace

#define MPG_GEOM_CHECK(NAME)                                                                                  \
    MPG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && cin >= 1 && cout >= 1, NAME ": bad shape");                     \
    MPG_REQUIRE(kh >= 1 && kw >= 1 && kh <= 16 && kw <= 16, NAME ": bad filter %dx%d", kh, kw);               \
    MPG_REQUIRE(stride_h >= 1 && stride_w >= 1, NAME ": bad stride")

extern "C" int mpg_conv2d_wgrad(mpg_stream_t stream, const float* x, int n, int h, int w, int cin, const float* dy,
                                int cout, int kh, int kw, int stride_h, int stride_w, float wscale, float* dw) {
    MPG_REQUIRE(x && dy && dw, "mpg_conv2d_wgrad: null pointer");
    MPG_GEOM_CHECK("mpg_conv2d_wgrad");
    ConvGeom g;
    fill_geom(g, n, h, w, cin, cout, kh, kw, stride_h, stride_w);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = mpg::zero_async(dw, (size_t)kh * kw * cin * cout * sizeof(float), s);
    if (e != hipSuccess) return mpg::hip_check(e, "mpg_conv2d_wgrad: memset");
    const int mi = micro(cin), ni = micro(cout);
#define MPG_WG(M, N) if (mi == M && ni == N) launch_wgrad<M, N>(s, x, dy, dw, g, wscale)
    MPG_WG(1, 1); MPG_WG(1, 2); MPG_WG(1, 4); MPG_WG(1, 8);
    MPG_WG(2, 1); MPG_WG(2, 2); MPG_WG(2, 4); MPG_WG(2, 8);
    MPG_WG(4, 1); MPG_WG(4, 2); MPG_WG(4, 4); MPG_WG(4, 8);
    MPG_WG(8, 1); MPG_WG(8, 2); MPG_WG(8, 4); MPG_WG(8, 8);
#undef MPG_WG
    MPG_LAUNCH_CHECK("wgrad_kernel");
}

extern "C" int mpg_conv2d_dgrad(mpg_stream_t stream, const float* dy, int n, int h, int w, int cin,
                                const float* w_hwoi, int cout, int kh, int kw, int stride_h, int stride_w,
                                float wscale, float* dx) {
    MPG_REQUIRE(dy && w_hwoi && dx, "mpg_conv2d_dgrad: null pointer");
    MPG_GEOM_CHECK("mpg_conv2d_dgrad");
    ConvGeom g;
    fill_geom(g, n, h, w, cin, cout, kh, kw, stride_h, stride_w);
    const size_t total = (size_t)n * h * w * cin;
    hipLaunchKernelGGL(dgrad_kernel, dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, dy, w_hwoi, dx, g,
                       wscale);
    MPG_LAUNCH_CHECK("dgrad_kernel");
}

extern "C" int mpg_fc_forward(mpg_stream_t stream, const float* x, int rows, int k, const float* w, int cout,
                              float wscale, const float* bias, int act, float leak, float* y) {
    MPG_REQUIRE(x && w && y, "mpg_fc_forward: null pointer");
    MPG_REQUIRE(rows >= 1 && k >= 1 && cout >= 1, "mpg_fc_forward: bad shape");
    MPG_REQUIRE(act >= MPG_ACT_NONE && act <= MPG_ACT_TANH, "mpg_fc_forward: bad activation %d", act);
    const int ogroups = (cout + 63) / 64;
    if (k >= 16384 && (size_t)rows * ogroups < 512) {
        int splits = (int)(1024 / ((size_t)rows * ogroups));
        if (splits > k / 2048) splits = k / 2048;                       // at least 2048 terms per block
        if (splits > 1) {
            const int kchunk = ((k + splits - 1) / splits + 255) / 256 * 256;
            splits = (k + kchunk - 1) / kchunk;
            hipError_t e = mpg::zero_async(y, (size_t)rows * cout * sizeof(float), (hipStream_t)stream);
            if (e != hipSuccess) return mpg::hip_check(e, "mpg_fc_forward: zero");
            hipLaunchKernelGGL(fc_splitk_kernel, dim3(rows, ogroups, splits), dim3(BLK), 0, (hipStream_t)stream, x, w, k, cout,
                               kchunk, wscale, y);
            hipLaunchKernelGGL(fc_finish_kernel, dim3(grid_for((size_t)rows * cout)), dim3(BLK), 0, (hipStream_t)stream, y, bias,
                               (size_t)rows * cout, cout, act, leak);
            MPG_LAUNCH_CHECK("fc_splitk_kernel");
        }
    }
    hipLaunchKernelGGL(fc_fwd_kernel, dim3(rows, ogroups), dim3(BLK), 0, (hipStream_t)stream, x, w, bias, k,
                       cout, wscale, act, leak, y);
    MPG_LAUNCH_CHECK("fc_fwd_kernel");
}
