// The fused convolution for layers of at most 8 channels on either side: not matrix work (mpgan_conv.h).
#include "mpgan_conv.h"

using namespace mpg::conv;

namespace {

// extra bytes of dynamic LDS asked for by every conv_small_kernel launch (occupancy experiments)
#ifndef MPG_SM_PAD
#define MPG_SM_PAD 0
#endif

// ---------------------------------------------------------------------------------------------
// conv_small_kernel: fused convolution for layers with <= 8 input and <= 8 output channels per
// segment.  One thread per output pixel holds the 8 output channels; every tap is one 16-byte
// read per plane of the single G8 channel group (hi + lo -> fp32), the weights are wave-uniform
// scalar loads.  HBM / L1 bound, fp32 arithmetic on fp32-grade activations.
// ---------------------------------------------------------------------------------------------
struct SmallSeg {
    const char* x;
    const float* w;       // [tap][8][8]
    int cg_total, g_off, kh, kw, up, upy, pt, pl, hs, ws, cin;
};

struct SmallArgs {
    int n, h, w, cout, nseg;
    int tile_floats;      // floats of the halo tile of the largest segment; the weight table follows it in LDS
    SmallSeg seg[MPG_MAX_SEG];
    const float* bias;
    const float* in_amax;
    int act;
    float leak;
    float* y;
    char* y_g8;
};

__device__ __forceinline__ void g8_load8(const char* src, size_t plane_bytes, float (&v)[8]) {
    const half8 hi = *reinterpret_cast<const half8*>(src);
    const half8 lo = *reinterpret_cast<const half8*>(src + plane_bytes);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)hi[j] + (float)lo[j];
}

// block = 64 x 16 output pixels; a thread owns a COLUMN of four of them (rows 4 yg .. 4 yg + 3 at column lx), so that
// consecutive lanes read consecutive 16-byte LDS words (no bank conflicts) and the rows a thread reads for one filter
// column serve all of its pixels: (4 + kh - 1) pixel reads per kx instead of 4 kh, and every tap's weight block --
// LDS broadcasts of the dense [tap][CINB][COUT] table -- feeds four pixels.  Per segment the halo tile is converted to
// fp32 ONCE into LDS as planes of four channels ([plane][row][col] float4, zero outside the image).
#ifndef MPG_SM_RPT
#define MPG_SM_RPT 4
#endif
constexpr int SM_TW = 64, SM_RPT = MPG_SM_RPT, SM_TH = 4 * SM_RPT, SM_KMAX = 7;
#ifndef MPG_DIAG_SMALL
#define MPG_DIAG_SMALL 0
#endif
#ifndef MPG_SMALL_INV
#define MPG_SMALL_INV 0
#endif
#if MPG_DIAG_SMALL
__device__ unsigned g_small_diag[2];
#endif

// The <= 8 bias values of a small layer, read once per thread in front of every loop (uniform addresses; index clamped
// to the last channel instead of a branch per value: nothing at or beyond bias + cout is read, and channels beyond cout
// are never used).  Zeros without a bias.
template <int C>
__device__ __forceinline__ void small_bias(const float* bias, int cout, float (&bq)[C]) {
#pragma unroll
    for (int q = 0; q < C; ++q) bq[q] = 0.f;
    if (bias != nullptr) {
#pragma unroll
        for (int q = 0; q < C; ++q) bq[q] = bias[q < cout ? q : cout - 1];
    }
}
// run f(std::integral_constant<int, act>): one uniform switch around code that holds a single activation
template <class F>
__device__ __forceinline__ void with_act(int act, F&& f) {
    switch (act) {
        case MPG_ACT_RELU: f(std::integral_constant<int, MPG_ACT_RELU>{}); break;
        case MPG_ACT_LRELU: f(std::integral_constant<int, MPG_ACT_LRELU>{}); break;
        case MPG_ACT_TANH: f(std::integral_constant<int, MPG_ACT_TANH>{}); break;
        default: f(std::integral_constant<int, MPG_ACT_NONE>{}); break;
    }
}

// COUT / CINB: output channels / input channels per segment rounded up to 1, 2, 4, 8 (compile-time loop bounds: the
// weight table holds zeros beyond cin and cout, a G8 group holds zeros beyond its channels)
template <int COUT, int CINB>
__global__ __launch_bounds__(256) void conv_small_kernel(SmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    constexpr int PL = (CINB + 3) / 4;                 // planes of four channels
    constexpr int CP = CINB < 4 ? CINB : 4;            // channels used of a plane
    float4* tile = reinterpret_cast<float4*>(small_lds);
    float* wl = small_lds + a.tile_floats;
    const int tid = threadIdx.x;
    const int lx = tid % SM_TW, yg = tid / SM_TW;
    const int x0 = blockIdx.x * SM_TW, y0 = blockIdx.y * SM_TH, b = blockIdx.z;
#if MPG_SMALL_INV
    asm volatile("buffer_inv sc0 sc1" ::: "memory");
#endif
    float bq[COUT];
    small_bias(a.bias, a.cout, bq);
    const float amax = a.in_amax != nullptr ? *a.in_amax : 0.f;     // pow2_scale(0) == 1
    float acc[SM_RPT][COUT];
#pragma unroll
    for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[j][co] = 0.f;
    for (int s = 0; s < a.nseg; ++s) {
        const SmallSeg& g = a.seg[s];
        const size_t plane_bytes = (size_t)g.hs * g.ws * 16;
        const char* base = g.x + ((size_t)b * g.cg_total + g.g_off) * 2 * plane_bytes;
        const int tw = SM_TW + g.kw - 1, th = SM_TH + g.kh - 1;
        if (s > 0) __syncthreads();
        for (int p = tid; p < g.kh * g.kw * CINB * COUT; p += 256) {
            const int co = p % COUT, ci = (p / COUT) % CINB, tap = p / (COUT * CINB);
            wl[p] = g.w[tap * 64 + ci * 8 + co];
        }
        for (int p = tid; p < tw * th; p += 256) {
            const int hy = p / tw, hx = p - hy * tw;
            const int yy = y0 - g.pt + hy, xx = x0 - g.pl + hx;
            float v[8];
            if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
                g8_load8(base + ((size_t)(yy >> g.upy) * g.ws + (xx >> g.up)) * 16, plane_bytes, v);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = 0.f;
            }
            tile[p] = make_float4(v[0], v[1], v[2], v[3]);
            if (PL > 1) tile[th * tw + p] = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
        const int kh = g.kh;
        for (int kx = 0; kx < g.kw; ++kx) {
            // the rows this thread's four pixels see through filter column kx
            float rows[SM_RPT + SM_KMAX - 1][CINB];
#pragma unroll
            for (int r = 0; r < SM_RPT + SM_KMAX - 1; ++r) {
                if (r < SM_RPT + kh - 1) {
                    const float4* src = tile + (yg * SM_RPT + r) * tw + lx + kx;
                    const float4 p0 = src[0];
                    rows[r][0] = p0.x;
                    if constexpr (CP > 1) rows[r][1] = p0.y;
                    if constexpr (CP > 2) { rows[r][2] = p0.z; rows[r][3] = p0.w; }
                    if constexpr (PL > 1) {
                        const float4 p1 = src[th * tw];
                        rows[r][4] = p1.x; rows[r][5] = p1.y; rows[r][6] = p1.z; rows[r][7] = p1.w;
                    }
                }
            }
#pragma unroll
            for (int ky = 0; ky < SM_KMAX; ++ky) {
                if (ky < kh) {
                    const float* wt = wl + (ky * g.kw + kx) * (CINB * COUT);
#pragma unroll
                    for (int ci = 0; ci < CINB; ++ci) {
                        float wv[COUT];
                        if (COUT >= 4) {
#pragma unroll
                            for (int q = 0; q < COUT / 4; ++q) {
                                const float4 w4 = *reinterpret_cast<const float4*>(wt + ci * COUT + 4 * q);
                                wv[4 * q] = w4.x; wv[4 * q + 1] = w4.y; wv[4 * q + 2] = w4.z; wv[4 * q + 3] = w4.w;
                            }
                        } else if (COUT == 2) {
                            const float2 w2 = *reinterpret_cast<const float2*>(wt + ci * 2);
                            wv[0] = w2.x; wv[1] = w2.y;
                        } else {
                            wv[0] = wt[ci];
                        }
#pragma unroll
                        for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
                            for (int co = 0; co < COUT; ++co) acc[j][co] = fmaf(rows[j + ky][ci], wv[co], acc[j][co]);
                    }
                }
            }
        }
#if MPG_DIAG_SMALL
        {   // diagnostic: is this block's LDS still what it wrote?  (foreign writes into the allocation; checked for EVERY
            // segment right after its sums, before the next segment overwrites the table and the tile)
            __syncthreads();
            unsigned bad_w = 0, bad_t = 0;
            for (int p = tid; p < g.kh * g.kw * CINB * COUT; p += 256) {
                const int co = p % COUT, ci = (p / COUT) % CINB, tap = p / (COUT * CINB);
                if (wl[p] != g.w[tap * 64 + ci * 8 + co]) ++bad_w;
            }
            for (int p = tid; p < tw * th; p += 256) {
                const int hy = p / tw, hx = p - hy * tw;
                const int yy = y0 - g.pt + hy, xx = x0 - g.pl + hx;
                float v[8];
                if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
                    g8_load8(base + ((size_t)(yy >> g.upy) * g.ws + (xx >> g.up)) * 16, plane_bytes, v);
                } else {
                    for (int q = 0; q < 8; ++q) v[q] = 0.f;
                }
                const float4 t0 = tile[p];
                if (t0.x != v[0] || t0.y != v[1] || t0.z != v[2] || t0.w != v[3]) ++bad_t;
                if (PL > 1) {
                    const float4 t1 = tile[th * tw + p];
                    if (t1.x != v[4] || t1.y != v[5] || t1.z != v[6] || t1.w != v[7]) ++bad_t;
                }
            }
            if (bad_w) atomicAdd(&g_small_diag[0], bad_w);
            if (bad_t) atomicAdd(&g_small_diag[1], bad_t);
        }
#endif
    }
    const int x = x0 + lx;
    if (x >= a.w) return;
    const float unscale = 1.f / mpg::pow2_scale(amax);
    const size_t plane_px = (size_t)a.h * a.w;
    // the values of the thread's SM_RPT pixels under the launch's activation (the only code that differs between the
    // activations), then the stores
    float o[SM_RPT][8];
    with_act(a.act, [&](auto actc) {
        constexpr int ACT = decltype(actc)::value;
#pragma unroll
        for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q)
                o[j][q] = (q < COUT && q < a.cout) ? mpg::apply_act(acc[j][q < COUT ? q : 0] * unscale + bq[q < COUT ? q : 0], ACT, a.leak) : 0.f;
    });
#pragma unroll
    for (int j = 0; j < SM_RPT; ++j) {
        const int y = y0 + yg * SM_RPT + j;
        if (y >= a.h) break;
        const size_t pix = (size_t)y * a.w + x;
        if (a.y != nullptr) {
            float* dst = a.y + ((size_t)b * plane_px + pix) * a.cout;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < a.cout) dst[q] = o[j][q];
        }
        if (a.y_g8 != nullptr) {
            half8 hi, lo;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                hi[q] = (_Float16)o[j][q];
                lo[q] = (_Float16)(o[j][q] - (float)hi[q]);
            }
            char* dst = a.y_g8 + ((size_t)b * 2 * plane_px + pix) * 16;
            *reinterpret_cast<half8*>(dst) = hi;
            *reinterpret_cast<half8*>(dst + plane_px * 16) = lo;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// conv_small_pair_kernel: a residual block whose three convolutions all have <= 8 channels on either side -- the first
// and the last block of gen_resnet, relu(convB(relu(convA(x))) + conv1x1(x)) with 1 -> 2 -> 8 and 8 -> 2 -> 1 channels
// (GAN/multipassGAN-4x.py:505-526,560,564) -- as ONE launch.  The block's middle tensor never leaves the CU: stage A is
// evaluated on the output tile plus the halo of filter B (68 x 20 pixels for a 64 x 16 tile and a 5x5 filter) into LDS,
// stage B and the shortcut read it and the input tile from there.  As two launches the middle tensor made a round
// trip through HBM in the G8 layout (32 bytes per pixel written and read for two channels) and the second launch
// waited for the last block of the first.
// A thread owns a column of SM_RPT pixels in both stages (see conv_small_kernel).  Middle pixels outside the image
// are zero: filter B sees the SAME padding of a tensor of the image's size, not an extension of stage A.
// ---------------------------------------------------------------------------------------------
struct PairArgs {
    int n, h, w;
    const char* x;                 // G8 input, one channel group
    int cg_total, g_off, up, upy, hs, ws;
    const float *wa, *wb, *wsc;    // [tap][8][8] tables: stage A (cin -> cmid), stage B (cmid -> cout), shortcut (cin -> cout) or null
    int kha, kwa, pta, pla;        // filter A and its SAME padding before
    int khb, kwb, ptb, plb;
    int khs, kws, pts, pls;
    const float *bias_a, *bias_b;
    int act_a, act_b;
    float leak_a, leak_b;
    int cmid, cout;
    float* y;
    char* y_g8;
    int x_px, mid_px;              // pixels of the input tile / of the middle tile (LDS plane sizes)
};

// sums of one filter over a column of SM_RPT pixels: tile = planes of four channels [plane][row][col] (float4), the
// thread's first row is `row0`, its column `col` (both in tile coordinates of the first tap); wl = [tap][CINB][COUTB]
template <int CINB, int COUTB>
__device__ __forceinline__ void small_column(const float4* tile, int tw, int plane_px, int row0, int col, const float* wl,
                                             int kh, int kw, float (&acc)[SM_RPT][COUTB]) {
    constexpr int PL = (CINB + 3) / 4, CP = CINB < 4 ? CINB : 4;
    for (int kx = 0; kx < kw; ++kx) {
        float rows[SM_RPT + SM_KMAX - 1][CINB];
#pragma unroll
        for (int r = 0; r < SM_RPT + SM_KMAX - 1; ++r) {
            if (r < SM_RPT + kh - 1) {
                const float4* src = tile + (row0 + r) * tw + col + kx;
                const float4 p0 = src[0];
                rows[r][0] = p0.x;
                if constexpr (CP > 1) rows[r][1] = p0.y;
                if constexpr (CP > 2) { rows[r][2] = p0.z; rows[r][3] = p0.w; }
                if constexpr (PL > 1) {
                    const float4 p1 = src[plane_px];
                    rows[r][4] = p1.x; rows[r][5] = p1.y; rows[r][6] = p1.z; rows[r][7] = p1.w;
                }
            }
        }
#pragma unroll
        for (int ky = 0; ky < SM_KMAX; ++ky) {
            if (ky < kh) {
                const float* wt = wl + (ky * kw + kx) * (CINB * COUTB);
#pragma unroll
                for (int ci = 0; ci < CINB; ++ci) {
                    float wv[COUTB];
#pragma unroll
                    for (int co = 0; co < COUTB; ++co) wv[co] = wt[ci * COUTB + co];
#pragma unroll
                    for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
                        for (int co = 0; co < COUTB; ++co) acc[j][co] = fmaf(rows[j + ky][ci], wv[co], acc[j][co]);
                }
            }
        }
    }
}

template <int CINB, int CMIDB, int COUTB>
__global__ __launch_bounds__(256) void conv_small_pair_kernel(PairArgs a) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    constexpr int PLX = (CINB + 3) / 4, PLM = (CMIDB + 3) / 4;
    float4* xt = reinterpret_cast<float4*>(small_lds);               // input tile: PLX planes of x_px pixels
    float4* mt = xt + PLX * a.x_px;                                   // middle tile: PLM planes of mid_px pixels
    float* wla = reinterpret_cast<float*>(mt + PLM * a.mid_px);       // [tap][CINB][CMIDB]
    float* wlb = wla + a.kha * a.kwa * CINB * CMIDB;                  // [tap][CMIDB][COUTB]
    float* wls = wlb + a.khb * a.kwb * CMIDB * COUTB;                 // [tap][CINB][COUTB]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SM_TW, y0 = blockIdx.y * SM_TH, b = blockIdx.z;
    float bqa[CMIDB], bqb[COUTB];
    small_bias(a.bias_a, a.cmid, bqa);    // (middle channels beyond cmid meet zero weights in stage B)
    small_bias(a.bias_b, a.cout, bqb);
    const int mw = SM_TW + a.kwb - 1, mh = SM_TH + a.khb - 1;         // middle tile
    const int xw = mw + a.kwa - 1, xh = mh + a.kha - 1;               // input tile
    const int mx0 = x0 - a.plb, my0 = y0 - a.ptb;                     // image coordinates of the tiles' first pixels
    const int xx0 = mx0 - a.pla, xy0 = my0 - a.pta;
    for (int p = tid; p < a.kha * a.kwa * CINB * CMIDB; p += 256) {
        const int co = p % CMIDB, ci = (p / CMIDB) % CINB, tap = p / (CMIDB * CINB);
        wla[p] = a.wa[tap * 64 + ci * 8 + co];
    }
    for (int p = tid; p < a.khb * a.kwb * CMIDB * COUTB; p += 256) {
        const int co = p % COUTB, ci = (p / COUTB) % CMIDB, tap = p / (COUTB * CMIDB);
        wlb[p] = a.wb[tap * 64 + ci * 8 + co];
    }
    if (a.wsc != nullptr)
        for (int p = tid; p < a.khs * a.kws * CINB * COUTB; p += 256) {
            const int co = p % COUTB, ci = (p / COUTB) % CINB, tap = p / (COUTB * CINB);
            wls[p] = a.wsc[tap * 64 + ci * 8 + co];
        }
    {
        const size_t plane_bytes = (size_t)a.hs * a.ws * 16;
        const char* base = a.x + ((size_t)b * a.cg_total + a.g_off) * 2 * plane_bytes;
        for (int p = tid; p < xw * xh; p += 256) {
            const int hy = p / xw, hx = p - hy * xw;
            const int yy = xy0 + hy, xx = xx0 + hx;
            float v[8];
            if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
                g8_load8(base + ((size_t)(yy >> a.upy) * a.ws + (xx >> a.up)) * 16, plane_bytes, v);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = 0.f;
            }
            xt[p] = make_float4(v[0], v[1], v[2], v[3]);
            if (PLX > 1) xt[a.x_px + p] = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
    __syncthreads();
    // ---- stage A on the middle tile: columns of SM_RPT pixels, mw x ceil(mh / SM_RPT) of them ----
    const int mgroups = (mh + SM_RPT - 1) / SM_RPT;
    for (int t = tid; t < mw * mgroups; t += 256) {
        const int col = t % mw, rg = t / mw;
        float acc[SM_RPT][CMIDB];
#pragma unroll
        for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
            for (int c = 0; c < CMIDB; ++c) acc[j][c] = 0.f;
        small_column<CINB, CMIDB>(xt, xw, a.x_px, rg * SM_RPT, col, wla, a.kha, a.kwa, acc);
        float o[SM_RPT][8];
        with_act(a.act_a, [&](auto actc) {
            constexpr int ACT = decltype(actc)::value;
#pragma unroll
            for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    o[j][c] = c < CMIDB ? mpg::apply_act(acc[j][c < CMIDB ? c : 0] + bqa[c < CMIDB ? c : 0], ACT, a.leak_a) : 0.f;
        });
#pragma unroll
        for (int j = 0; j < SM_RPT; ++j) {
            const int row = rg * SM_RPT + j;
            if (row < mh) {
                const int yy = my0 + row, xx = mx0 + col;
                const bool in = yy >= 0 && yy < a.h && xx >= 0 && xx < a.w;
                mt[row * mw + col] = in ? make_float4(o[j][0], o[j][1], o[j][2], o[j][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (PLM > 1) mt[a.mid_px + row * mw + col] = in ? make_float4(o[j][4], o[j][5], o[j][6], o[j][7]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __syncthreads();
    // ---- stage B + shortcut on the output tile ----
    const int lx = tid % SM_TW, yg = tid / SM_TW;
    float acc[SM_RPT][COUTB];
#pragma unroll
    for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
        for (int c = 0; c < COUTB; ++c) acc[j][c] = 0.f;
    small_column<CMIDB, COUTB>(mt, mw, a.mid_px, yg * SM_RPT, lx, wlb, a.khb, a.kwb, acc);
    if (a.wsc != nullptr)     // the shortcut reads the input tile; its first tap sits at (ptb + pta - pts, plb + pla - pls) of it
        small_column<CINB, COUTB>(xt, xw, a.x_px, yg * SM_RPT + a.ptb + a.pta - a.pts, lx + a.plb + a.pla - a.pls, wls, a.khs, a.kws, acc);
    const int x = x0 + lx;
    if (x >= a.w) return;
    const size_t plane_px = (size_t)a.h * a.w;
    float o[SM_RPT][8];
    with_act(a.act_b, [&](auto actc) {
        constexpr int ACT = decltype(actc)::value;
#pragma unroll
        for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q)
                o[j][q] = (q < COUTB && q < a.cout) ? mpg::apply_act(acc[j][q < COUTB ? q : 0] + bqb[q < COUTB ? q : 0], ACT, a.leak_b) : 0.f;
    });
#pragma unroll
    for (int j = 0; j < SM_RPT; ++j) {
        const int y = y0 + yg * SM_RPT + j;
        if (y >= a.h) break;
        const size_t pix = (size_t)y * a.w + x;
        if (a.y != nullptr) {
            float* dst = a.y + ((size_t)b * plane_px + pix) * a.cout;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < a.cout) dst[q] = o[j][q];
        }
        if (a.y_g8 != nullptr) {
            half8 hi, lo;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                hi[q] = (_Float16)o[j][q];
                lo[q] = (_Float16)(o[j][q] - (float)hi[q]);
            }
            char* dst = a.y_g8 + ((size_t)b * 2 * plane_px + pix) * 16;
            *reinterpret_cast<half8*>(dst) = hi;
            *reinterpret_cast<half8*>(dst + plane_px * 16) = lo;
        }
    }
}

}  // namespace

// small-channel layers (every cin and cout <= 8, plain epilogue): conv_small_kernel
int mpg::conv::launch_small(hipStream_t stream, const mpg_conv_desc* d) {
    SmallArgs sa;
    sa.n = d->n; sa.h = d->h; sa.w = d->w; sa.cout = d->cout; sa.nseg = d->nseg;
    int cmax = 1, tmax = 1, tile_px = 0;
    for (int s = 0; s < d->nseg; ++s) {
        if (const int rc = check_segment(d, s)) return rc;
        const mpg_conv_seg& g = d->seg[s];
        SmallSeg& o = sa.seg[s];
        o.x = (const char*)g.x;
        o.w = (const float*)((const char*)g.wpack + pack_base_bytes(g.kh, g.kw, g.cin, d->cout, d->prec));
        o.cg_total = g.cgroups; o.g_off = g.g_off; o.kh = g.kh; o.kw = g.kw; o.up = g.up_log2; o.upy = g.up_x_only ? 0 : g.up_log2;
        o.pt = pad_before(g.kh, g.pad_hi); o.pl = pad_before(g.kw, g.pad_hi);
        o.hs = d->h >> o.upy; o.ws = d->w >> o.up; o.cin = g.cin;
        cmax = g.cin > cmax ? g.cin : cmax;
        tmax = g.kh * g.kw > tmax ? g.kh * g.kw : tmax;
        const int px = (SM_TH + g.kh - 1) * (SM_TW + g.kw - 1);
        tile_px = px > tile_px ? px : tile_px;
    }
    for (int s = d->nseg; s < MPG_MAX_SEG; ++s) sa.seg[s] = sa.seg[0];
    sa.bias = d->bias; sa.in_amax = d->in_amax; sa.act = d->act; sa.leak = d->leak;
    sa.y = d->y; sa.y_g8 = (char*)d->y_g8;
    MPG_REQUIRE((((uintptr_t)d->y_g8) & 15) == 0, "mpg_conv2d_fused: misaligned output");
    const dim3 grid((unsigned)((d->w + SM_TW - 1) / SM_TW), (unsigned)((d->h + SM_TH - 1) / SM_TH), (unsigned)d->n);
    const int cob = d->cout == 1 ? 1 : d->cout == 2 ? 2 : d->cout <= 4 ? 4 : 8;
    const int cib = cmax == 1 ? 1 : cmax == 2 ? 2 : cmax <= 4 ? 4 : 8;
    sa.tile_floats = tile_px * 4 * ((cib + 3) / 4);       // one or two planes of four channels
    const size_t lds = ((size_t)sa.tile_floats + (size_t)tmax * cib * cob) * sizeof(float) + MPG_SM_PAD;
    switch (cob * 16 + cib) {
#define MPG_SMALL(CO, CI) \
    case CO * 16 + CI: hipLaunchKernelGGL((conv_small_kernel<CO, CI>), grid, dim3(256), lds, stream, sa); break;
        MPG_SMALL(1, 1) MPG_SMALL(1, 2) MPG_SMALL(1, 4) MPG_SMALL(1, 8)
        MPG_SMALL(2, 1) MPG_SMALL(2, 2) MPG_SMALL(2, 4) MPG_SMALL(2, 8)
        MPG_SMALL(4, 1) MPG_SMALL(4, 2) MPG_SMALL(4, 4) MPG_SMALL(4, 8)
        MPG_SMALL(8, 1) MPG_SMALL(8, 2) MPG_SMALL(8, 4) MPG_SMALL(8, 8)
#undef MPG_SMALL
        default: break;
    }
    MPG_LAUNCH_CHECK("conv_small_kernel");
}

// One residual block of <= 8-channel convolutions as a single launch (conv_small_pair_kernel).
extern "C" int mpg_conv2d_small_pair(mpg_stream_t stream, const mpg_small_pair_desc* d) {
    MPG_REQUIRE(d != nullptr, "mpg_conv2d_small_pair: null desc");
    MPG_REQUIRE(d->n >= 1 && d->h >= 1 && d->w >= 1 && d->n <= 65535, "mpg_conv2d_small_pair: bad shape %d x %d x %d", d->n, d->h, d->w);
    MPG_REQUIRE(d->cin >= 1 && d->cin <= 8 && d->cmid >= 1 && d->cmid <= 8 && d->cout >= 1 && d->cout <= 8,
                "mpg_conv2d_small_pair: %d -> %d -> %d channels (1..8 each)", d->cin, d->cmid, d->cout);
    MPG_REQUIRE(d->x && d->wpack_a && d->wpack_b, "mpg_conv2d_small_pair: null pointer");
    MPG_REQUIRE(d->y != nullptr || d->y_g8 != nullptr, "mpg_conv2d_small_pair: no output requested");
    MPG_REQUIRE(d->kh_a >= 1 && d->kh_a <= 7 && d->kw_a >= 1 && d->kw_a <= 7 && d->kh_b >= 1 && d->kh_b <= 7 && d->kw_b >= 1 && d->kw_b <= 7,
                "mpg_conv2d_small_pair: kernel sizes 1..7");
    MPG_REQUIRE((d->kh_a & 1) && (d->kw_a & 1) && (d->kh_b & 1) && (d->kw_b & 1), "mpg_conv2d_small_pair: odd filters only");
    MPG_REQUIRE(d->wpack_s == nullptr || (d->kh_s >= 1 && d->kh_s <= d->kh_a + d->kh_b - 1 && d->kw_s >= 1 && d->kw_s <= d->kw_a + d->kw_b - 1 &&
                                          (d->kh_s & 1) && (d->kw_s & 1) && ((d->kh_a + d->kh_b) & 1) == 0 && ((d->kw_a + d->kw_b) & 1) == 0),
                "mpg_conv2d_small_pair: the shortcut filter must be odd and fit inside the input tile of two odd filters");
    MPG_REQUIRE(d->g_off >= 0 && d->g_off < d->cgroups, "mpg_conv2d_small_pair: channel-group range");
    MPG_REQUIRE(d->up_x_only == 0 || d->up_x_only == 1, "mpg_conv2d_small_pair: up_x_only %d (0 or 1)", d->up_x_only);
    MPG_REQUIRE(d->up_log2 >= 0 && d->up_log2 <= 4 && (d->up_x_only || (d->h % (1 << d->up_log2)) == 0) && (d->w % (1 << d->up_log2)) == 0,
                "mpg_conv2d_small_pair: upsample %d", d->up_log2);
    MPG_REQUIRE(d->act_a >= MPG_ACT_NONE && d->act_a <= MPG_ACT_TANH && d->act_b >= MPG_ACT_NONE && d->act_b <= MPG_ACT_TANH, "mpg_conv2d_small_pair: bad act");
    MPG_REQUIRE(d->prec == MPG_PREC_F16X1 || d->prec == MPG_PREC_F16X3 || d->prec == MPG_PREC_F16F6, "mpg_conv2d_small_pair: bad prec %d", d->prec);
    MPG_REQUIRE((((uintptr_t)d->x) & 15) == 0 && (((uintptr_t)d->y_g8) & 15) == 0, "mpg_conv2d_small_pair: misaligned tensor");
    PairArgs a;
    a.n = d->n; a.h = d->h; a.w = d->w;
    a.x = (const char*)d->x; a.cg_total = d->cgroups; a.g_off = d->g_off; a.up = d->up_log2; a.upy = d->up_x_only ? 0 : d->up_log2;
    a.hs = d->h >> a.upy; a.ws = d->w >> a.up;
    a.wa = (const float*)((const char*)d->wpack_a + pack_base_bytes(d->kh_a, d->kw_a, d->cin, d->cmid, d->prec));
    a.wb = (const float*)((const char*)d->wpack_b + pack_base_bytes(d->kh_b, d->kw_b, d->cmid, d->cout, d->prec));
    a.wsc = d->wpack_s ? (const float*)((const char*)d->wpack_s + pack_base_bytes(d->kh_s, d->kw_s, d->cin, d->cout, d->prec)) : nullptr;
    a.kha = d->kh_a; a.kwa = d->kw_a; a.pta = pad_before(d->kh_a, 0); a.pla = pad_before(d->kw_a, 0);
    a.khb = d->kh_b; a.kwb = d->kw_b; a.ptb = pad_before(d->kh_b, 0); a.plb = pad_before(d->kw_b, 0);
    a.khs = d->wpack_s ? d->kh_s : 1; a.kws = d->wpack_s ? d->kw_s : 1; a.pts = pad_before(a.khs, 0); a.pls = pad_before(a.kws, 0);
    a.bias_a = d->bias_a; a.bias_b = d->bias_b; a.act_a = d->act_a; a.act_b = d->act_b; a.leak_a = d->leak_a; a.leak_b = d->leak_b;
    a.cmid = d->cmid; a.cout = d->cout; a.y = d->y; a.y_g8 = (char*)d->y_g8;
    const int mw = SM_TW + a.kwb - 1, mh = SM_TH + a.khb - 1;
    const int mgroups = (mh + SM_RPT - 1) / SM_RPT;
    const int xw = mw + a.kwa - 1, xh = mgroups * SM_RPT + a.kha - 1;      // rows past the middle tile are read, never used
    a.x_px = xw * xh;
    a.mid_px = mw * (mgroups * SM_RPT + a.khb - 1);
    // compile-time channel bounds: cin in {1, 4, 8}, cmid in {2, 8}, cout in {1, 8}
    const int ci = d->cin == 1 ? 1 : d->cin <= 4 ? 4 : 8, cm = d->cmid <= 2 ? 2 : 8, co = d->cout == 1 ? 1 : 8;
    const size_t lds = ((size_t)((ci + 3) / 4) * a.x_px + (size_t)((cm + 3) / 4) * a.mid_px) * 16 +
                       ((size_t)a.kha * a.kwa * ci * cm + (size_t)a.khb * a.kwb * cm * co + (size_t)a.khs * a.kws * ci * co) * sizeof(float);
    MPG_REQUIRE(lds <= LDS_MAX, "mpg_conv2d_small_pair: LDS budget %zu exceeds 160 KiB", lds);
    const dim3 grid((unsigned)((d->w + SM_TW - 1) / SM_TW), (unsigned)((d->h + SM_TH - 1) / SM_TH), (unsigned)d->n);
    hipError_t le = hipSuccess;
    switch (ci * 100 + cm * 10 + co) {
#define MPG_PAIR(CI, CM, CO) case CI * 100 + CM * 10 + CO: \
        le = mpg::launch_dyn_lds<conv_small_pair_kernel<CI, CM, CO>>(grid, dim3(256), lds, (hipStream_t)stream, a); break;
        MPG_PAIR(1, 2, 1) MPG_PAIR(1, 2, 8) MPG_PAIR(1, 8, 1) MPG_PAIR(1, 8, 8)
        MPG_PAIR(4, 2, 1) MPG_PAIR(4, 2, 8) MPG_PAIR(4, 8, 1) MPG_PAIR(4, 8, 8)
        MPG_PAIR(8, 2, 1) MPG_PAIR(8, 2, 8) MPG_PAIR(8, 8, 1) MPG_PAIR(8, 8, 8)
#undef MPG_PAIR
        default: break;
    }
    if (le != hipSuccess) return mpg::hip_check(le, "mpg_conv2d_small_pair: hipFuncSetAttribute(dynamic LDS)");
    MPG_LAUNCH_CHECK("conv_small_pair_kernel");
}

#if MPG_DIAG_SMALL
extern "C" int mpg_debug_small_diag(unsigned* out2) {
    return hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_small_diag), 8) == hipSuccess ? 0 : 1;
}
#endif
