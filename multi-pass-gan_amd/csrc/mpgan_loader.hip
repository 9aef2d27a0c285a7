// Device side of the training-set loader's slice mode (the half next to mpgan_tiles.hip): what
// tools_wscale/fluiddataloader.py:387-544 does to every entry with numpy / scipy on one host thread -- the slice-axis view
// with the velocity components following it (:416-431), scipy.ndimage.zoom(order=1) of the whole array (:497-510), the
// per-slice density means of removeSlices (:295-313), addAdjSlices (:315-336) and the row selection -- on a source that was
// uploaded once, WITHOUT the zoomed array ever existing: the means are taken over the virtual zoomed array, and only the
// slices the host then keeps are interpolated.
//
// The virtual array of both entries: V = zoom(transpose(src, perm + (3,)), factors), src [d0,d1,d2,c] fp32, V [o0,o1,o2,c].
// Along V's axis k (n = d[perm[k]] source points, o_k output points) output index o reads source coordinate
// o * ((n - 1) / (o_k - 1)) -- the ratio first, then the product, both in float64, as scipy forms them; o * 1.0 where
// o_k == 1 -- and, like scipy's mode 'constant', is 0 where that coordinate rounds above n - 1 (see resample_kernel of
// mpgan_tiles.hip).  Order 1, separable: x, then y, then z, fp32 weights w = frac(coordinate) and 1 - w.  An axis whose
// weight is 0 (factor 1, integer coordinates) takes no blend and its upper neighbour is not read, so such values are the
// source's bits.  Channels are never interpolated.
// HBM-bound gather work, one thread per output unit (V channels), channels fastest.
// Entries: mpg_slice_zoom_means, mpg_slice_zoom_gather.
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

constexpr int LOADER_CMAX = 16;              // mapped channels of one gather (three packed frames of d,vx,vy,vz are 12)
constexpr int MEANS_MAX_BLOCKS = 64;         // pixel blocks per slice: the workspace is MEANS_MAX_BLOCKS * o0 floats

struct ZoomArgs {
    int n[3];                   // source points along V's axes: n[k] = d[perm[k]]
    int o[3];                   // V's spatial size
    size_t stride[3];           // distance in floats between neighbours along V's axis k in src
    double ratio[3];            // source coordinate = index * ratio
};

// one axis of one output element: the two source offsets, the upper weight, and whether scipy writes 0 there
struct AxisPos {
    size_t lo, hi;
    float w;
    bool zero;
};

__device__ __forceinline__ AxisPos axis_pos(const ZoomArgs& a, int k, int o) {
    const double cc = (double)o * a.ratio[k];
    const double fl = floor(cc);
    int i0 = (int)fl;
    i0 = max(0, min(i0, a.n[k] - 1));
    const int i1 = min(i0 + 1, a.n[k] - 1);
    AxisPos p;
    p.lo = (size_t)i0 * a.stride[k];
    p.hi = (size_t)i1 * a.stride[k];
    p.w = (float)(cc - fl);
    p.zero = cc < 0.0 || cc > (double)(a.n[k] - 1);
    return p;
}

template <int V>
__device__ __forceinline__ void blend(float (&a)[V], const float (&b)[V], float w) {
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = (1.f - w) * a[j] + w * b[j];
}

// V consecutive channels, the first one `ch`, of V at the position (p0, p1, p2)
template <int V>
__device__ __forceinline__ void zoom_fetch(const float* __restrict__ src, const AxisPos& p0, const AxisPos& p1, const AxisPos& p2,
                                           int ch, float (&out)[V]) {
    if (p0.zero || p1.zero || p2.zero) {
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = 0.f;
        return;
    }
    float vz[2][V];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (a == 1 && p0.w == 0.f) break;
        float vy[2][V];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b == 1 && p1.w == 0.f) break;
            const float* p = src + (a ? p0.hi : p0.lo) + (b ? p1.hi : p1.lo) + ch;
            ldv<V>(p + p2.lo, vy[b]);
            if (p2.w != 0.f) {
                float t[V];
                ldv<V>(p + p2.hi, t);
                blend<V>(vy[b], t, p2.w);
            }
        }
        if (p1.w != 0.f) blend<V>(vy[0], vy[1], p1.w);
#pragma unroll
        for (int j = 0; j < V; ++j) vz[a][j] = vy[0][j];
    }
    if (p0.w != 0.f) blend<V>(vz[0], vz[1], p0.w);
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = vz[0][j];
}

// grid (blocks, o0): block x adds the pixels [x * ppb, (x + 1) * ppb) of slice y -- a thread its own in pixel order, then the
// fixed tree over the threads -- into partials[x * o0 + y]
__global__ __launch_bounds__(256) void slice_means_partial_kernel(const float* __restrict__ src, ZoomArgs a, int chan, size_t ppb,
                                                                  float* __restrict__ partials) {
    __shared__ float red[1][BLK];
    const int s = blockIdx.y;
    const size_t npix = (size_t)a.o[1] * a.o[2];
    const size_t p_begin = (size_t)blockIdx.x * ppb;
    const size_t p_end = min(npix, p_begin + ppb);
    const AxisPos p0 = axis_pos(a, 0, s);
    float sum = 0.f;
    for (size_t p = p_begin + threadIdx.x; p < p_end; p += BLK) {
        const int j = (int)(p % a.o[2]);
        const int i = (int)(p / a.o[2]);
        float v[1];
        zoom_fetch<1>(src, p0, axis_pos(a, 1, i), axis_pos(a, 2, j), chan, v);
        sum += v[0];
    }
    red[0][threadIdx.x] = sum;
    block_tree_sum<1>(red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * a.o[0] + s] = red[0][0];
}

// the blocks' sums of a slice in THE order of mpgan_valu.h (a slice takes the place of a channel), divided by the pixels
__global__ __launch_bounds__(256) void slice_means_final_kernel(const float* __restrict__ partials, int nblocks, int o0, float npix,
                                                                float* __restrict__ means) {
    int s;
    float S[1];
    if (ordered_partials_sum<1>(partials, nblocks, o0, s, S)) means[s] = S[0] / npix;
}

struct GatherArgs {
    int n_slices, nq, adj, out_c, c_off;
    int cmap[LOADER_CMAX];
};

// V == 4: a unit is four output channels that come from ONE aligned group of four source channels (the velocity exchange
// stays inside a packed frame), read with one 16-byte access per corner and put in place in registers.
// V == 1: one output channel; with adj the channels of a frame are followed by channel 0 of that frame in V[s-1] and V[s+1].
template <int V>
__global__ __launch_bounds__(256) void slice_gather_kernel(const float* __restrict__ src, ZoomArgs a, GatherArgs g,
                                                           const int* __restrict__ slices, float* __restrict__ out) {
    const int oc_n = g.nq + (g.adj ? 6 : 0);           // channels this launch writes per pixel
    const int units = oc_n / V;
    const size_t npix = (size_t)a.o[1] * a.o[2];
    const size_t total = (size_t)g.n_slices * npix * units;
    const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (idx >= total) return;
    const int u = (int)(idx % units);
    size_t r = idx / units;
    const int j = (int)(r % a.o[2]); r /= a.o[2];
    const int i = (int)(r % a.o[1]);
    const int row = (int)(r / a.o[1]);
    int s = slices[row];
    float* d = out + ((size_t)row * npix + (size_t)i * a.o[2] + j) * g.out_c + g.c_off + u * V;
    float v[V];
    int ch;
    if constexpr (V == 4) {
        ch = g.cmap[4 * u] & ~3;
    } else if (g.adj) {
        const int cf = g.nq / 3, f = u / (cf + 2), k = u - f * (cf + 2);
        ch = g.cmap[f * cf + (k < cf ? k : 0)];
        if (k == cf) s -= 1;
        if (k == cf + 1) s += 1;
    } else {
        ch = g.cmap[u];
    }
    if (s < 0 || s >= a.o[0]) {               // beyond the ends (addAdjSlices); a bad table entry reads nothing either
#pragma unroll
        for (int q = 0; q < V; ++q) v[q] = 0.f;
    } else {
        zoom_fetch<V>(src, axis_pos(a, 0, s), axis_pos(a, 1, i), axis_pos(a, 2, j), ch, v);
    }
    if constexpr (V == 4) {
        float w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = g.cmap[4 * u + q] & 3;
            w[q] = m == 0 ? v[0] : m == 1 ? v[1] : m == 2 ? v[2] : v[3];
        }
        stv<4>(d, w);
    } else {
        d[0] = v[0];
    }
}

// shapes of both entries -> ZoomArgs; the message names the entry
int zoom_args(const char* who, const int* dims3, int c, const int* perm3, const int* out3, ZoomArgs* a) {
    MPG_REQUIRE(dims3 && out3, "%s: null shape", who);
    MPG_REQUIRE(dims3[0] >= 1 && dims3[1] >= 1 && dims3[2] >= 1 && c >= 1, "%s: bad source shape", who);
    const size_t st[3] = {(size_t)dims3[1] * dims3[2] * c, (size_t)dims3[2] * c, (size_t)c};
    int seen = 0;
    for (int k = 0; k < 3; ++k) {
        const int ax = perm3 ? perm3[k] : k;
        MPG_REQUIRE(ax >= 0 && ax < 3, "%s: perm", who);
        seen |= 1 << ax;
        MPG_REQUIRE(out3[k] >= 1, "%s: bad output shape", who);
        a->n[k] = dims3[ax];
        a->o[k] = out3[k];
        a->stride[k] = st[ax];
        a->ratio[k] = out3[k] > 1 ? (double)(dims3[ax] - 1) / (double)(out3[k] - 1) : 1.0;
    }
    MPG_REQUIRE(seen == 7, "%s: perm is not a permutation", who);
    return MPG_OK;
}

}  // namespace

extern "C" int mpg_slice_zoom_means(mpg_stream_t stream, const float* src, const int* dims3, int c, const int* perm3,
                                    const int* out3, int chan, float* means, float* workspace, size_t workspace_floats) {
    MPG_REQUIRE(src && means && workspace, "mpg_slice_zoom_means: null pointer");
    ZoomArgs a;
    const int rc = zoom_args("mpg_slice_zoom_means", dims3, c, perm3, out3, &a);
    if (rc != MPG_OK) return rc;
    MPG_REQUIRE(chan >= 0 && chan < c, "mpg_slice_zoom_means: channel %d of %d", chan, c);
    MPG_REQUIRE(a.o[0] <= 65535, "mpg_slice_zoom_means: more than 65535 slices");
    const size_t npix = (size_t)a.o[1] * a.o[2];
    const PixelSplit sp = split_pixels(npix, 1, MEANS_MAX_BLOCKS);
    MPG_REQUIRE(workspace_floats >= sp.blocks * (size_t)a.o[0], "mpg_slice_zoom_means: workspace of %zu floats, %zu needed",
                workspace_floats, sp.blocks * (size_t)a.o[0]);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(slice_means_partial_kernel, dim3((unsigned)sp.blocks, a.o[0]), dim3(BLK), 0, s, src, a, chan, sp.ppb,
                       workspace);
    hipLaunchKernelGGL(slice_means_final_kernel, dim3((a.o[0] + 15) / 16), dim3(BLK), 0, s, workspace, (int)sp.blocks, a.o[0],
                       (float)npix, means);
    MPG_LAUNCH_CHECK("slice means kernels");
}

extern "C" int mpg_slice_zoom_gather(mpg_stream_t stream, const float* src, const int* dims3, int c, const int* perm3,
                                     const int* out3, const int* slices, int n_slices, const int* chan_map, int n_chan, int adj,
                                     float* out, int out_c, int c_off) {
    MPG_REQUIRE(src && slices && out, "mpg_slice_zoom_gather: null pointer");
    ZoomArgs a;
    const int rc = zoom_args("mpg_slice_zoom_gather", dims3, c, perm3, out3, &a);
    if (rc != MPG_OK) return rc;
    GatherArgs g;
    g.n_slices = n_slices; g.nq = n_chan; g.adj = adj != 0; g.out_c = out_c; g.c_off = c_off;
    MPG_REQUIRE(n_slices >= 1, "mpg_slice_zoom_gather: no slices");
    MPG_REQUIRE(n_chan >= 1 && n_chan <= LOADER_CMAX, "mpg_slice_zoom_gather: 1..%d channels", LOADER_CMAX);
    MPG_REQUIRE(!g.adj || n_chan % 3 == 0, "mpg_slice_zoom_gather: adj needs three packed frames, %d channels", n_chan);
    const int oc_n = n_chan + (g.adj ? 6 : 0);
    MPG_REQUIRE(c_off >= 0 && out_c >= 1 && c_off + oc_n <= out_c, "mpg_slice_zoom_gather: channels [%d, %d) of %d", c_off,
                c_off + oc_n, out_c);
    bool wide = !g.adj && c % 4 == 0 && n_chan % 4 == 0 && out_c % 4 == 0 && c_off % 4 == 0 &&
                ((size_t)src | (size_t)out) % 16 == 0;
    for (int q = 0; q < LOADER_CMAX; ++q) {
        g.cmap[q] = q < n_chan ? (chan_map ? chan_map[q] : q) : 0;
        MPG_REQUIRE(g.cmap[q] >= 0 && g.cmap[q] < c, "mpg_slice_zoom_gather: chan_map[%d]", q);
        if (q < n_chan && g.cmap[q] / 4 != g.cmap[q & ~3] / 4) wide = false;
    }
    const size_t total = (size_t)n_slices * a.o[1] * a.o[2] * (wide ? oc_n / 4 : oc_n);
    MPG_REQUIRE(total / BLK < 0x7fffffffu, "mpg_slice_zoom_gather: too many elements for one launch");
    if (wide)
        hipLaunchKernelGGL(slice_gather_kernel<4>, dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, src, a, g, slices, out);
    else
        hipLaunchKernelGGL(slice_gather_kernel<1>, dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, src, a, g, slices, out);
    MPG_LAUNCH_CHECK("slice_gather_kernel");
}
