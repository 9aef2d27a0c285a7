// The fused convolution for layers of at most 8 channels on either side: not matrix work (mpgan_conv.h).
#include "mpgan_conv.h"

using namespace mpg::conv;

namespace {

// ---------------------------------------------------------------------------------------------
// conv_small_kernel: fused convolution for layers with <= 8 input and <= 8 output channels per
// segment.  One thread holds the output channels of a column of SM_RPT output pixels.  Per segment
// the block converts its halo tile (hi + lo -> fp32) and the segment's dense weight table into LDS
// once; every filter column then costs SM_RPT + kh - 1 pixel reads from LDS per thread, and the
// weights are LDS broadcasts.  fp32 arithmetic on fp32-grade activations.
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

// block = 64 x 16 output pixels; a thread owns a COLUMN of four of them (rows 4 yg .. 4 yg + 3 at column lx), so that
// consecutive lanes read consecutive LDS words (no bank conflicts) and the rows a thread reads for one filter
// column serve all of its pixels: (4 + kh - 1) pixel reads per kx instead of 4 kh, and every tap's weight block --
// LDS broadcasts of the dense [tap][CS][COUT] table -- feeds four pixels.  Per segment the halo tile is converted to
// fp32 ONCE into LDS, zero outside the image, CS = the segment's channels rounded up to 1, 2, 4 or 8 per pixel:
// [row][col] of float, float2 or float4, and two such planes of float4 for 8 channels.
#ifndef MPG_SM_RPT
#define MPG_SM_RPT 4
#endif
constexpr int SM_TW = 64, SM_RPT = MPG_SM_RPT, SM_TH = 4 * SM_RPT, SM_KMAX = 7;
// Every global load of a block -- halo tile and weight tables -- is issued before the first of them is waited for, in
// loops whose trip counts are known to the compiler: the passes of 256 threads over the largest tile and table.
constexpr int passes(int n) { return (n + 255) / 256; }
constexpr int SM_TILE_PASSES = passes((SM_TW + SM_KMAX - 1) * (SM_TH + SM_KMAX - 1));
constexpr int SM_PAIR_PASSES = passes((SM_TW + 2 * (SM_KMAX - 1)) * (SM_TH + 2 * (SM_KMAX - 1)));   // input tile of two filters
constexpr int SM_TAPS = SM_KMAX * SM_KMAX;
// tables and tiles start on 16 bytes in LDS
__host__ __device__ constexpr int up4(int n) { return (n + 3) & ~3; }
// channels rounded up to 1, 2, 4, 8
__host__ __device__ constexpr int chan_bound(int c) { return c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : 8; }

// A value that every thread of the launch reads and that was written before the launch: a scalar load.  Such a load is
// no vector-memory operation, so a register that waits for it does not stand between the tile loads further down.
__device__ __forceinline__ float uniform_load(const float* p) {
    return *reinterpret_cast<const __attribute__((address_space(4))) float*>(reinterpret_cast<uintptr_t>(p));
}
// The <= 8 bias values of a small layer, read once per wave in front of every loop (index clamped to the last channel
// instead of a branch per value: nothing at or beyond bias + cout is read, and channels beyond cout are never used).
// Zeros without a bias.
template <int C>
__device__ __forceinline__ void small_bias(const float* bias, int cout, float (&bq)[C]) {
#pragma unroll
    for (int q = 0; q < C; ++q) bq[q] = 0.f;
    if (bias != nullptr) {
#pragma unroll
        for (int q = 0; q < C; ++q) bq[q] = uniform_load(bias + (q < cout ? q : cout - 1));
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
// run f(std::integral_constant<int, chan_bound(cin)>) for cin <= CMAX (1, 2, 4 or 8): one uniform switch per segment
template <int CMAX, class F>
__device__ __forceinline__ void with_chan_bound(int cin, F&& f) {
    if (CMAX >= 8 && cin > 4) f(std::integral_constant<int, CMAX >= 8 ? 8 : CMAX>{});
    else if (CMAX >= 4 && cin > 2) f(std::integral_constant<int, CMAX >= 4 ? 4 : CMAX>{});
    else if (CMAX >= 2 && cin > 1) f(std::integral_constant<int, CMAX >= 2 ? 2 : CMAX>{});
    else f(std::integral_constant<int, 1>{});
}

// ---- weight tables: [tap][8][8] in memory -> dense [tap][CI][CO] in LDS ----
template <int CI, int CO>
struct TableLoads {
    static constexpr int NPASS = passes(SM_TAPS * CI * CO);
    float v[NPASS];
};
template <int CI, int CO>
__device__ __forceinline__ float table_word(const float* w, int p) {
    const int co = p % CO, ci = (p / CO) % CI, tap = p / (CO * CI);
    return w[tap * 64 + ci * 8 + co];
}
template <int CI, int CO>
__device__ __forceinline__ void table_issue(TableLoads<CI, CO>& t, const float* w, int n, int tid) {
#pragma unroll
    for (int i = 0; i < TableLoads<CI, CO>::NPASS; ++i) {
        const int p = tid + 256 * i;
        t.v[i] = 0.f;
        if (p < n) t.v[i] = table_word<CI, CO>(w, p);
    }
}
// (no table has more than SM_TAPS taps: the host code refuses larger filters, the shortcut of a pair included)
template <int CI, int CO>
__device__ __forceinline__ void table_store(const TableLoads<CI, CO>& t, float* wl, int n, int tid) {
#pragma unroll
    for (int i = 0; i < TableLoads<CI, CO>::NPASS; ++i) {
        const int p = tid + 256 * i;
        if (p < n) wl[p] = t.v[i];
    }
}

// ---- halo tiles: G8 in memory -> fp32 in LDS ----
// The words of a thread's pixels p = tid + 256 i of a tile: the first LC channels of the hi and of the lo plane.
template <int LC, int NPASS>
struct TileLoads {
    typedef _Float16 hv __attribute__((ext_vector_type(LC)));
    hv hi[NPASS], lo[NPASS];
    unsigned inside;      // bit i: pixel i lies in the image (every other pixel of the tile is zero)
};
// tile of tw columns and npx pixels whose first pixel is (ty0, tx0) of the h x w image; the source is the image
// shrunk by (upy, up) bits, ws pixels wide.  A pixel outside the image loads the nearest one inside (so every address
// is one of the tensor) and is replaced by zero in tile_store; pixels at and beyond npx load nothing.
template <int LC, int NPASS>
__device__ __forceinline__ void tile_issue(TileLoads<LC, NPASS>& t, const char* base, size_t plane_bytes, int ws, int up, int upy,
                                           int h, int w, int ty0, int tx0, int tw, int npx, int tid) {
    typedef typename TileLoads<LC, NPASS>::hv hv;
    const int qs = 256 / tw, rs = 256 - qs * tw;     // 256 pixels further: qs rows and rs columns
    int hy = tid / tw, hx = tid - hy * tw;
    t.inside = 0;
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
        const int yy = ty0 + hy, xx = tx0 + hx;
        const bool live = tid + 256 * i < npx;
        if (live && yy >= 0 && yy < h && xx >= 0 && xx < w) t.inside |= 1u << i;
        const int yc = min(max(yy, 0), h - 1), xc = min(max(xx, 0), w - 1);
        const char* src = base + ((size_t)(yc >> upy) * ws + (xc >> up)) * 16;
        t.hi[i] = hv{};
        t.lo[i] = hv{};
        if (live) {
            t.hi[i] = *reinterpret_cast<const hv*>(src);
            t.lo[i] = *reinterpret_cast<const hv*>(src + plane_bytes);
        }
        hx += rs;
        hy += qs;
        if (hx >= tw) { hx -= tw; ++hy; }
    }
}
// hi + lo -> fp32, CS channels per pixel (CS <= LC) into the tile of plane_px pixels per plane
template <int CS, int LC, int NPASS>
__device__ __forceinline__ void tile_store(const TileLoads<LC, NPASS>& t, float* tile, int plane_px, int npx, int tid) {
    static_assert(CS <= LC, "a tile pixel holds no more channels than were loaded");
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
        const int p = tid + 256 * i;
        if (p < npx) {
            const bool in = (t.inside >> i) & 1;
            float v[CS];
#pragma unroll
            for (int j = 0; j < CS; ++j) v[j] = in ? (float)t.hi[i][j] + (float)t.lo[i][j] : 0.f;
            if constexpr (CS == 1) tile[p] = v[0];
            if constexpr (CS == 2) reinterpret_cast<float2*>(tile)[p] = make_float2(v[0], v[1]);
            if constexpr (CS >= 4) reinterpret_cast<float4*>(tile)[p] = make_float4(v[0], v[1], v[2], v[3]);
            if constexpr (CS == 8) reinterpret_cast<float4*>(tile)[plane_px + p] = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
}
// the CS channels of tile pixel idx
template <int CS>
__device__ __forceinline__ void tile_pixel(const float* tile, int plane_px, int idx, float (&r)[CS]) {
    if constexpr (CS == 1) r[0] = tile[idx];
    if constexpr (CS == 2) {
        const float2 p = reinterpret_cast<const float2*>(tile)[idx];
        r[0] = p.x; r[1] = p.y;
    }
    if constexpr (CS >= 4) {
        const float4 p = reinterpret_cast<const float4*>(tile)[idx];
        r[0] = p.x; r[1] = p.y; r[2] = p.z; r[3] = p.w;
    }
    if constexpr (CS == 8) {
        const float4 p = reinterpret_cast<const float4*>(tile)[plane_px + idx];
        r[4] = p.x; r[5] = p.y; r[6] = p.z; r[7] = p.w;
    }
}
// CS channels of a pixel into the tile (the middle tile of a pair)
template <int CS>
__device__ __forceinline__ void tile_put(float* tile, int plane_px, int idx, const float (&v)[8]) {
    if constexpr (CS == 1) tile[idx] = v[0];
    if constexpr (CS == 2) reinterpret_cast<float2*>(tile)[idx] = make_float2(v[0], v[1]);
    if constexpr (CS >= 4) reinterpret_cast<float4*>(tile)[idx] = make_float4(v[0], v[1], v[2], v[3]);
    if constexpr (CS == 8) reinterpret_cast<float4*>(tile)[plane_px + idx] = make_float4(v[4], v[5], v[6], v[7]);
}

// Sums of one filter over a column of SM_RPT pixels: the thread's first row of the tile is `row0`, its column `col`
// (both in tile coordinates of the first tap); wl = [tap][CS][COUTB].  KH, KW > 0: the filter's size, known to the
// compiler (no branch in the sums); KH == 0: kh x kw <= SM_KMAX x SM_KMAX, decided while running.  Either way an output
// is the same chain of fmaf: kx outer, then ky, then ci.
template <int CS, int COUTB, int KH, int KW>
__device__ __forceinline__ void small_column(const float* tile, int tw, int plane_px, int row0, int col, const float* wl,
                                             int kh_run, int kw_run, float (&acc)[SM_RPT][COUTB]) {
    constexpr int KHM = KH > 0 ? KH : SM_KMAX, NW = CS * COUTB;
    const int kh = KH > 0 ? KH : kh_run, kw = KW > 0 ? KW : kw_run;
    // a filter column of a small block is unrolled into the next, so that its pixel reads run under these sums
    constexpr int UNROLL_KX = KW > 0 && NW <= 16 ? KW : 1;
#pragma unroll UNROLL_KX
    for (int kx = 0; kx < kw; ++kx) {
        // the rows this thread's pixels see through filter column kx
        float rows[SM_RPT + KHM - 1][CS];
#pragma unroll
        for (int r = 0; r < SM_RPT + KHM - 1; ++r)
            if (KH > 0 || r < SM_RPT + kh - 1) tile_pixel<CS>(tile, plane_px, (row0 + r) * tw + col + kx, rows[r]);
#pragma unroll
        for (int ky = 0; ky < KHM; ++ky) {
            if (KH > 0 || ky < kh) {
                // the tap's [CS][COUTB] block: up to 16 weights at once in the widest reads their number allows (one
                // ds_read_b128 is two input channels of a 2-channel output), a larger block one input channel at a time
                const float* wt = wl + (ky * kw + kx) * NW;
                constexpr int WG = NW <= 16 ? NW : COUTB;
                constexpr int WQ = WG % 4 == 0 ? 4 : WG % 2 == 0 ? 2 : 1;
#pragma unroll
                for (int g0 = 0; g0 < NW; g0 += WG) {
                    float wv[WG];
#pragma unroll
                    for (int q = 0; q < WG / WQ; ++q) {
                        if constexpr (WQ == 4) {
                            const float4 w4 = *reinterpret_cast<const float4*>(wt + g0 + 4 * q);
                            wv[4 * q] = w4.x; wv[4 * q + 1] = w4.y; wv[4 * q + 2] = w4.z; wv[4 * q + 3] = w4.w;
                        } else if constexpr (WQ == 2) {
                            const float2 w2 = *reinterpret_cast<const float2*>(wt + g0 + 2 * q);
                            wv[2 * q] = w2.x; wv[2 * q + 1] = w2.y;
                        } else {
                            wv[q] = wt[g0 + q];
                        }
                    }
#pragma unroll
                    for (int c = 0; c < WG / COUTB; ++c)
#pragma unroll
                        for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
                            for (int co = 0; co < COUTB; ++co)
                                acc[j][co] = fmaf(rows[j + ky][g0 / COUTB + c], wv[c * COUTB + co], acc[j][co]);
                }
            }
        }
    }
}
// the filter sizes of both generators' small layers are instantiated, every other size takes the run-time form
template <int CS, int COUTB>
__device__ __forceinline__ void small_filter(const float* tile, int tw, int plane_px, int row0, int col, const float* wl, int kh, int kw,
                                             float (&acc)[SM_RPT][COUTB]) {
    // (not for 8 -> 8 channels: with 64 weights per tap the instantiated sizes would cost a wave per SIMD in registers)
    constexpr bool SIZES = CS * COUTB < 64;
    if (SIZES && kh == 5 && kw == 5) small_column<CS, COUTB, SIZES ? 5 : 0, SIZES ? 5 : 0>(tile, tw, plane_px, row0, col, wl, kh, kw, acc);
    else if (SIZES && kh == 1 && kw == 1) small_column<CS, COUTB, SIZES ? 1 : 0, SIZES ? 1 : 0>(tile, tw, plane_px, row0, col, wl, kh, kw, acc);
    else small_column<CS, COUTB, 0, 0>(tile, tw, plane_px, row0, col, wl, kh, kw, acc);
}

// the thread's SM_RPT pixels of column x (rows y0 ..): fp32 NHWC and / or G8
__device__ __forceinline__ void small_store(const float (&o)[SM_RPT][8], float* y, char* y_g8, int b, int h, int w, int cout, int y0, int x) {
    const size_t plane_px = (size_t)h * w;
#pragma unroll
    for (int j = 0; j < SM_RPT; ++j) {
        const int yy = y0 + j;
        if (yy >= h) break;
        const size_t pix = (size_t)yy * w + x;
        if (y != nullptr) {
            float* dst = y + ((size_t)b * plane_px + pix) * cout;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < cout) dst[q] = o[j][q];
        }
        if (y_g8 != nullptr) {
            half8 hi, lo;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                hi[q] = (_Float16)o[j][q];
                lo[q] = (_Float16)(o[j][q] - (float)hi[q]);
            }
            char* dst = y_g8 + ((size_t)b * 2 * plane_px + pix) * 16;
            *reinterpret_cast<half8*>(dst) = hi;
            *reinterpret_cast<half8*>(dst + plane_px * 16) = lo;
        }
    }
}

// COUT: output channels rounded up to 1, 2, 4, 8; CINB: the same of the launch's widest segment, which sizes the LDS.
// A segment works on its own channels rounded up (CS): the weight table holds zeros beyond cin and cout and a G8 group
// holds zeros beyond its channels, so the terms left out of a narrow segment are fmaf(0, 0, acc) = acc (acc starts at
// +0 and a sum of products that reaches zero from +0 is +0 in round-to-nearest, never -0).
template <int COUT, int CINB>
__global__ __launch_bounds__(256) void conv_small_kernel(SmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    float* tile = small_lds;
    float* wl = small_lds + a.tile_floats;
    const int tid = threadIdx.x;
    const int lx = tid % SM_TW, yg = tid / SM_TW;
    const int x0 = blockIdx.x * SM_TW, y0 = blockIdx.y * SM_TH, b = blockIdx.z;
    float bq[COUT];
    small_bias(a.bias, a.cout, bq);
    const float amax = a.in_amax != nullptr ? uniform_load(a.in_amax) : 0.f;     // pow2_scale(0) == 1
    float acc[SM_RPT][COUT];
#pragma unroll
    for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[j][co] = 0.f;
    for (int s = 0; s < a.nseg; ++s) {
        const SmallSeg& g = a.seg[s];
        with_chan_bound<CINB>(g.cin, [&](auto csc) {
            constexpr int CS = decltype(csc)::value;
            constexpr int LC = CS < 2 ? 2 : CS;      // channels loaded per pixel and plane: 4, 8 or 16 bytes
            const size_t plane_bytes = (size_t)g.hs * g.ws * 16;
            const char* base = g.x + ((size_t)b * g.cg_total + g.g_off) * 2 * plane_bytes;
            const int tw = SM_TW + g.kw - 1, th = SM_TH + g.kh - 1;
            const int nw = g.kh * g.kw * CS * COUT;
            TableLoads<CS, COUT> tab;
            TileLoads<LC, SM_TILE_PASSES> px;
            tile_issue(px, base, plane_bytes, g.ws, g.up, g.upy, a.h, a.w, y0 - g.pt, x0 - g.pl, tw, tw * th, tid);
            table_issue(tab, g.w, nw, tid);
            if (s > 0) __syncthreads();      // the sums of the segment before this one have read the tile and the table
            table_store(tab, wl, nw, tid);
            tile_store<CS>(px, tile, tw * th, tw * th, tid);
            __syncthreads();
            small_filter<CS, COUT>(tile, tw, tw * th, yg * SM_RPT, lx, wl, g.kh, g.kw, acc);
        });
    }
    const int x = x0 + lx;
    if (x >= a.w) return;
    const float unscale = 1.f / mpg::pow2_scale(amax);
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
    small_store(o, a.y, a.y_g8, b, a.h, a.w, a.cout, y0 + yg * SM_RPT, x);
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

template <int CINB, int CMIDB, int COUTB>
__global__ __launch_bounds__(256) void conv_small_pair_kernel(PairArgs a) {
    extern __shared__ __attribute__((aligned(16))) float small_lds[];
    const int na = a.kha * a.kwa * CINB * CMIDB, nb = a.khb * a.kwb * CMIDB * COUTB, ns = a.wsc != nullptr ? a.khs * a.kws * CINB * COUTB : 0;
    float* xt = small_lds;                             // input tile: x_px pixels of CINB channels
    float* mt = xt + up4(a.x_px * CINB);               // middle tile: mid_px pixels of CMIDB channels
    float* wla = mt + up4(a.mid_px * CMIDB);           // [tap][CINB][CMIDB]
    float* wlb = wla + up4(na);                        // [tap][CMIDB][COUTB]
    float* wls = wlb + up4(nb);                        // [tap][CINB][COUTB]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SM_TW, y0 = blockIdx.y * SM_TH, b = blockIdx.z;
    float bqa[CMIDB], bqb[COUTB];
    small_bias(a.bias_a, a.cmid, bqa);    // (middle channels beyond cmid meet zero weights in stage B)
    small_bias(a.bias_b, a.cout, bqb);
    const int mw = SM_TW + a.kwb - 1, mh = SM_TH + a.khb - 1;         // middle tile
    const int xw = mw + a.kwa - 1, xh = mh + a.kha - 1;               // input tile
    const int mx0 = x0 - a.plb, my0 = y0 - a.ptb;                     // image coordinates of the tiles' first pixels
    const int xx0 = mx0 - a.pla, xy0 = my0 - a.pta;
    {
        constexpr int LC = CINB < 2 ? 2 : CINB;
        const size_t plane_bytes = (size_t)a.hs * a.ws * 16;
        const char* base = a.x + ((size_t)b * a.cg_total + a.g_off) * 2 * plane_bytes;
        TableLoads<CINB, CMIDB> ta;
        TableLoads<CMIDB, COUTB> tb;
        TableLoads<CINB, COUTB> ts;
        TileLoads<LC, SM_PAIR_PASSES> px;
        table_issue(ta, a.wa, na, tid);
        table_issue(tb, a.wb, nb, tid);
        table_issue(ts, a.wsc, ns, tid);
        tile_issue(px, base, plane_bytes, a.ws, a.up, a.upy, a.h, a.w, xy0, xx0, xw, xw * xh, tid);
        table_store(ta, wla, na, tid);
        table_store(tb, wlb, nb, tid);
        table_store(ts, wls, ns, tid);
        tile_store<CINB>(px, xt, a.x_px, xw * xh, tid);
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
        small_filter<CINB, CMIDB>(xt, xw, a.x_px, rg * SM_RPT, col, wla, a.kha, a.kwa, acc);
        float o[SM_RPT][8];
        with_act(a.act_a, [&](auto actc) {
            constexpr int ACT = decltype(actc)::value;
#pragma unroll
            for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    o[j][c] = c < CMIDB ? mpg::apply_act(acc[j][c < CMIDB ? c : 0] + bqa[c < CMIDB ? c : 0], ACT, a.leak_a) : 0.f;
        });
        const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < SM_RPT; ++j) {
            const int row = rg * SM_RPT + j;
            if (row < mh) {
                const int yy = my0 + row, xx = mx0 + col;
                const bool in = yy >= 0 && yy < a.h && xx >= 0 && xx < a.w;
                if (in) tile_put<CMIDB>(mt, a.mid_px, row * mw + col, o[j]);
                else tile_put<CMIDB>(mt, a.mid_px, row * mw + col, zero);
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
    small_filter<CMIDB, COUTB>(mt, mw, a.mid_px, yg * SM_RPT, lx, wlb, a.khb, a.kwb, acc);
    if (a.wsc != nullptr)     // the shortcut reads the input tile; its first tap sits at (ptb + pta - pts, plb + pla - pls) of it
        small_filter<CINB, COUTB>(xt, xw, a.x_px, yg * SM_RPT + a.ptb + a.pta - a.pts, lx + a.plb + a.pla - a.pls, wls, a.khs, a.kws, acc);
    const int x = x0 + lx;
    if (x >= a.w) return;
    float o[SM_RPT][8];
    with_act(a.act_b, [&](auto actc) {
        constexpr int ACT = decltype(actc)::value;
#pragma unroll
        for (int j = 0; j < SM_RPT; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q)
                o[j][q] = (q < COUTB && q < a.cout) ? mpg::apply_act(acc[j][q < COUTB ? q : 0] + bqb[q < COUTB ? q : 0], ACT, a.leak_b) : 0.f;
    });
    small_store(o, a.y, a.y_g8, b, a.h, a.w, a.cout, y0 + yg * SM_RPT, x);
}

}  // namespace

// small-channel layers (every cin and cout <= 8, plain epilogue): conv_small_kernel
int mpg::conv::launch_small(hipStream_t stream, const mpg_conv_desc* d) {
    SmallArgs sa;
    sa.n = d->n; sa.h = d->h; sa.w = d->w; sa.cout = d->cout; sa.nseg = d->nseg;
    const int cob = chan_bound(d->cout);
    int cmax = 1, tile_floats = 0, table_floats = 0;
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
        tile_floats = std::max(tile_floats, (SM_TH + g.kh - 1) * (SM_TW + g.kw - 1));
        table_floats = std::max(table_floats, g.kh * g.kw);
    }
    for (int s = d->nseg; s < MPG_MAX_SEG; ++s) sa.seg[s] = sa.seg[0];
    sa.bias = d->bias; sa.in_amax = d->in_amax; sa.act = d->act; sa.leak = d->leak;
    sa.y = d->y; sa.y_g8 = (char*)d->y_g8;
    MPG_REQUIRE((((uintptr_t)d->y_g8) & 15) == 0, "mpg_conv2d_fused: misaligned output");
    const dim3 grid((unsigned)((d->w + SM_TW - 1) / SM_TW), (unsigned)((d->h + SM_TH - 1) / SM_TH), (unsigned)d->n);
    // the LDS holds the largest tile and the largest table at the widest segment's channel bound
    const int cib = chan_bound(cmax);
    sa.tile_floats = up4(tile_floats * cib);
    const size_t lds = ((size_t)sa.tile_floats + (size_t)table_floats * cib * cob) * sizeof(float);
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
    // (no larger filter can be packed, and the sums run over at most SM_KMAX filter rows)
    MPG_REQUIRE(d->wpack_s == nullptr || (d->kh_s <= SM_KMAX && d->kw_s <= SM_KMAX), "mpg_conv2d_small_pair: shortcut filter %d x %d (1..7)",
                d->kh_s, d->kw_s);
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
    // the kernel's carving of the LDS: two tiles, three tables, each rounded up to 16 bytes
    const size_t lds = ((size_t)up4(a.x_px * ci) + up4(a.mid_px * cm) + up4(a.kha * a.kwa * ci * cm) + up4(a.khb * a.kwb * cm * co) +
                        up4(d->wpack_s ? a.khs * a.kws * ci * co : 0)) * sizeof(float);
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
