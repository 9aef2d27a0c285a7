// Preview images of the inference drivers, made where the pass volumes live: the three axis sums of save_img_3d
// (multipassGAN-out.py:208-210, called :461,523,585; -4x.py:1134,1146; -8x.py:1718), the planes of the slice loop
// (-out.py:592-604) and the 8-bit quantisation of save_img (:204-206).  Only bytes leave the device.
//
// mpg_volume_projections reads the volume once.  A wave owns a tile of PI x PJ x (64 V) elements, lanes along k, V
// consecutive k per lane.  Per lane it keeps the sums over the tile's i for its PJ x V columns (axis 0), the sum over the
// tile's j for the current i (axis 1), and per (i, j) the sum over the tile's k, folded across the lanes by a butterfly
// (axis 2).  The four waves of a block take four consecutive i ranges and add their axis-0 sums through LDS in wave order,
// so a block covers 4 PI planes.  Every tile writes its sums as partials [chunk][plane]; sum_partials_kernel adds the chunks
// of a plane element in ascending order.  No atomics: the same volume gives the same bits on every run.
#include "mpgan_valu.h"

using namespace mpg::valu;

namespace {

constexpr int PI = 8;             // i per wave
constexpr int PJ = 16;            // j per tile
constexpr int WAVES = BLK / 64;
constexpr int PBI = PI * WAVES;   // i per block

inline size_t chunks(int n, int per) { return ((size_t)n + per - 1) / per; }

template <int V>
__global__ __launch_bounds__(BLK) void volume_projections_kernel(const float* __restrict__ vol, int a, int b, int c, float divisor,
                                                                  float* __restrict__ part0, float* __restrict__ part1,
                                                                  float* __restrict__ part2) {
    constexpr int TK = 64 * V;
    __shared__ float red[WAVES][4][TK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k0 = blockIdx.x * TK, j0 = blockIdx.y * PJ, i0 = blockIdx.z * PBI + w * PI;
    const int k = k0 + lane * V;
    const bool live = k < c;                                   // V == 4: c % 4 == 0, so k + 3 < c as well
    const int i1 = min(i0 + PI, a);
    float acc0[PJ][V];
#pragma unroll
    for (int jj = 0; jj < PJ; ++jj)
#pragma unroll
        for (int v = 0; v < V; ++v) acc0[jj][v] = 0.f;
    for (int i = i0; i < i1; ++i) {
        float acc1[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc1[v] = 0.f;
        float keep = 0.f;
#pragma unroll
        for (int jj = 0; jj < PJ; ++jj) {
            const int j = j0 + jj;
            if (j >= b) continue;                              // wave-uniform
            float d[V];
#pragma unroll
            for (int v = 0; v < V; ++v) d[v] = 0.f;
            if (live) {
                ldv<V>(vol + ((size_t)i * b + j) * c + k, d);
#pragma unroll
                for (int v = 0; v < V; ++v) d[v] = d[v] / divisor;
            }
            float s = d[0];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                acc0[jj][v] += d[v];
                acc1[v] += d[v];
                if (v > 0) s += d[v];
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == jj) keep = s;
        }
        if (live) stv<V>(part1 + ((size_t)blockIdx.y * a + i) * c + k, acc1);
        if (lane < PJ && j0 + lane < b) part2[((size_t)blockIdx.x * a + i) * b + j0 + lane] = keep;
    }
    // axis 0: the four waves' sums, added in wave order, four j rows per round
#pragma unroll
    for (int r = 0; r < PJ / 4; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int v = 0; v < V; ++v) red[w][q][lane * V + v] = acc0[4 * r + q][v];
        __syncthreads();
        for (int e = threadIdx.x; e < 4 * TK; e += BLK) {
            const int q = e / TK, col = e % TK;
            const int j = j0 + 4 * r + q, kk = k0 + col;
            if (j < b && kk < c) {
                float s = red[0][q][col];
#pragma unroll
                for (int u = 1; u < WAVES; ++u) s += red[u][q][col];
                part0[((size_t)blockIdx.z * b + j) * c + kk] = s;
            }
        }
        __syncthreads();
    }
}

// out[e] = part[0][e] + part[1][e] + ... in that order, for the three planes of one call
__global__ void sum_partials_kernel(const float* __restrict__ part0, size_t n0, size_t e0, float* __restrict__ p0,
                                    const float* __restrict__ part1, size_t n1, size_t e1, float* __restrict__ p1,
                                    const float* __restrict__ part2, size_t n2, size_t e2, float* __restrict__ p2) {
    size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
    const float* part;
    float* out;
    size_t n, per;
    if (idx < e0) {
        part = part0; out = p0; n = n0; per = e0;
    } else if (idx < e0 + e1) {
        idx -= e0; part = part1; out = p1; n = n1; per = e1;
    } else if (idx < e0 + e1 + e2) {
        idx -= e0 + e1; part = part2; out = p2; n = n2; per = e2;
    } else {
        return;
    }
    float s = part[idx];
    for (size_t p = 1; p < n; ++p) s += part[p * per + idx];
    out[idx] = s;
}

// save_img's quantisation: a float32 product, clipped, truncated
__device__ __forceinline__ unsigned gray255(float v) { return (unsigned)fminf(fmaxf(v * 255.f, 0.f), 255.f); }

// four values per thread: one 16-byte load and one 32-bit store where QUAD (both pointers aligned), the tail by bytes
template <bool QUAD>
__global__ void gray8_kernel(const float* __restrict__ img, size_t n, unsigned char* __restrict__ out) {
    const size_t o = ((size_t)blockIdx.x * BLK + threadIdx.x) * 4;
    if (o >= n) return;
    if (QUAD && o + 4 <= n) {
        float t[4];
        ldv<4>(img + o, t);
        *reinterpret_cast<unsigned*>(out + o) = gray255(t[0]) | (gray255(t[1]) << 8) | (gray255(t[2]) << 16) | (gray255(t[3]) << 24);
    } else {
        for (size_t e = o; e < n && e < o + 4; ++e) out[e] = (unsigned char)gray255(img[e]);
    }
}

constexpr int PLANE_BATCH = 256;
struct PlaneArgs {
    size_t sr, ss, st;            // strides of the plane's first and second axis (array order) and of the sliced axis
    int nr, ns;                   // their sizes
    int n_idx, transposed;
    int idx[PLANE_BATCH];
};

// one thread per output byte: image t, row y, column x = plane element (y, x), or (x, y) when transposed
__global__ void planes_gray8_kernel(const float* __restrict__ vol, PlaneArgs p, unsigned char* __restrict__ gray) {
    const size_t o = (size_t)blockIdx.x * BLK + threadIdx.x;
    const size_t per = (size_t)p.nr * p.ns;
    if (o >= per * p.n_idx) return;
    const int t = o / per;
    const size_t e = o - (size_t)t * per;
    const int cols = p.transposed ? p.nr : p.ns;
    const size_t y = e / cols, x = e % cols;
    const size_t r = p.transposed ? x : y, s = p.transposed ? y : x;
    gray[o] = (unsigned char)gray255(vol[(size_t)p.idx[t] * p.st + r * p.sr + s * p.ss]);
}

// mean of plane blockIdx.x: a thread adds its elements e = tid, tid + 256, ... in that order, then the block's fixed tree
__global__ void plane_means_kernel(const float* __restrict__ vol, PlaneArgs p, float* __restrict__ mean) {
    __shared__ float red[1][BLK];
    const size_t per = (size_t)p.nr * p.ns;
    const float* base = vol + (size_t)p.idx[blockIdx.x] * p.st;
    float s = 0.f;
    for (size_t e = threadIdx.x; e < per; e += BLK) s += base[(e / p.ns) * p.sr + (e % p.ns) * p.ss];
    red[0][threadIdx.x] = s;
    block_tree_sum(red);
    if (threadIdx.x == 0) mean[blockIdx.x] = red[0][0] / (float)per;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" size_t mpg_volume_projections_ws_bytes(int a, int b, int c) {
    if (a < 1 || b < 1 || c < 1) return 0;
    // the partials of the scalar kernel (the most k chunks); each of the three arrays rounded up to 16 bytes
    const size_t f0 = chunks(a, PBI) * b * c, f1 = chunks(b, PJ) * a * c, f2 = chunks(c, 64) * a * b;
    return (((f0 + 3) & ~(size_t)3) + ((f1 + 3) & ~(size_t)3) + ((f2 + 3) & ~(size_t)3)) * sizeof(float);
}

extern "C" int mpg_volume_projections(mpg_stream_t stream, const float* vol, int a, int b, int c, float divisor, float* p0, float* p1,
                                      float* p2, void* ws) {
    MPG_REQUIRE(vol && p0 && p1 && p2 && ws, "mpg_volume_projections: null pointer");
    MPG_REQUIRE(a >= 1 && b >= 1 && c >= 1, "mpg_volume_projections: bad shape %d x %d x %d", a, b, c);
    MPG_REQUIRE(divisor != 0.f, "mpg_volume_projections: divisor 0");
    MPG_REQUIRE(aligned16(ws), "mpg_volume_projections: workspace not 16-byte aligned");
    const bool quad = c % 4 == 0 && aligned16(vol);
    const size_t n0 = chunks(a, PBI), n1 = chunks(b, PJ), n2 = chunks(c, quad ? 256 : 64);
    MPG_REQUIRE(n0 <= 65535 && n1 <= 65535, "mpg_volume_projections: volume too large for one launch");
    const size_t e0 = (size_t)b * c, e1 = (size_t)a * c, e2 = (size_t)a * b;
    float* part0 = static_cast<float*>(ws);
    float* part1 = part0 + ((n0 * e0 + 3) & ~(size_t)3);
    float* part2 = part1 + ((n1 * e1 + 3) & ~(size_t)3);
    const dim3 grid((unsigned)n2, (unsigned)n1, (unsigned)n0);
    hipStream_t s = (hipStream_t)stream;
    if (quad)
        hipLaunchKernelGGL((volume_projections_kernel<4>), grid, dim3(BLK), 0, s, vol, a, b, c, divisor, part0, part1, part2);
    else
        hipLaunchKernelGGL((volume_projections_kernel<1>), grid, dim3(BLK), 0, s, vol, a, b, c, divisor, part0, part1, part2);
    const int rc = mpg::hip_check(hipGetLastError(), "volume_projections_kernel");
    if (rc != MPG_OK) return rc;
    hipLaunchKernelGGL(sum_partials_kernel, dim3(grid_for(e0 + e1 + e2)), dim3(BLK), 0, s, part0, n0, e0, p0, part1, n1, e1, p1,
                       part2, n2, e2, p2);
    MPG_LAUNCH_CHECK("sum_partials_kernel");
}

extern "C" int mpg_gray8(mpg_stream_t stream, const float* img, size_t n, unsigned char* out) {
    MPG_REQUIRE(img && out, "mpg_gray8: null pointer");
    if (n == 0) return MPG_OK;
    const unsigned grid = grid_for((n + 3) / 4);
    if (aligned16(img) && (reinterpret_cast<uintptr_t>(out) & 3) == 0)
        hipLaunchKernelGGL((gray8_kernel<true>), dim3(grid), dim3(BLK), 0, (hipStream_t)stream, img, n, out);
    else
        hipLaunchKernelGGL((gray8_kernel<false>), dim3(grid), dim3(BLK), 0, (hipStream_t)stream, img, n, out);
    MPG_LAUNCH_CHECK("gray8_kernel");
}

extern "C" int mpg_volume_planes_gray8(mpg_stream_t stream, const float* vol, int a, int b, int c, int axis, const int* idx, int n_idx,
                                       int transposed, unsigned char* gray, float* mean) {
    MPG_REQUIRE(vol && idx && gray, "mpg_volume_planes_gray8: null pointer");
    MPG_REQUIRE(a >= 1 && b >= 1 && c >= 1, "mpg_volume_planes_gray8: bad shape %d x %d x %d", a, b, c);
    MPG_REQUIRE(axis >= 0 && axis <= 2, "mpg_volume_planes_gray8: axis %d (0..2)", axis);
    MPG_REQUIRE(n_idx >= 1, "mpg_volume_planes_gray8: no plane asked for");
    const int dims[3] = {a, b, c};
    const size_t strides[3] = {(size_t)b * c, (size_t)c, 1};
    for (int t = 0; t < n_idx; ++t)
        MPG_REQUIRE(idx[t] >= 0 && idx[t] < dims[axis], "mpg_volume_planes_gray8: index %d leaves axis %d of size %d", idx[t], axis,
                    dims[axis]);
    const int ar = axis == 0 ? 1 : 0, as = axis == 2 ? 1 : 2;
    PlaneArgs p;
    p.sr = strides[ar]; p.ss = strides[as]; p.st = strides[axis];
    p.nr = dims[ar]; p.ns = dims[as];
    p.transposed = transposed != 0;
    const size_t per = (size_t)p.nr * p.ns;
    for (int t0 = 0; t0 < n_idx; t0 += PLANE_BATCH) {
        p.n_idx = n_idx - t0 < PLANE_BATCH ? n_idx - t0 : PLANE_BATCH;
        for (int t = 0; t < PLANE_BATCH; ++t) p.idx[t] = t < p.n_idx ? idx[t0 + t] : 0;
        hipLaunchKernelGGL(planes_gray8_kernel, dim3(grid_for(per * p.n_idx)), dim3(BLK), 0, (hipStream_t)stream, vol, p,
                           gray + (size_t)t0 * per);
        int rc = mpg::hip_check(hipGetLastError(), "planes_gray8_kernel");
        if (rc != MPG_OK) return rc;
        if (mean != nullptr) {
            hipLaunchKernelGGL(plane_means_kernel, dim3(p.n_idx), dim3(BLK), 0, (hipStream_t)stream, vol, p, mean + t0);
            rc = mpg::hip_check(hipGetLastError(), "plane_means_kernel");
            if (rc != MPG_OK) return rc;
        }
    }
    return MPG_OK;
}
