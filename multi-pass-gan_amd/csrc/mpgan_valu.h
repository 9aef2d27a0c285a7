// What the vector-ALU translation units (mpgan_elem.hip, mpgan_tiles.hip, mpgan_bn.hip, mpgan_train_conv.hip,
// mpgan_train_elem.hip, mpgan_advect.hip, mpgan_optim.hip, mpgan_tempo.hip, mpgan_loader.hip, mpgan_preview.hip, mpgan_vorticity.hip) share: the block size and the one-thread-per-element grid,
// V-wide loads and stores, the block abs-max, and the three pieces the reproducible sums rest on -- the split of a pixel
// range over blocks, the ordered sum of the blocks' results and the fixed tree over a block's threads.
#pragma once
#include "mpgan_internal.h"

namespace mpg::valu {

constexpr int BLK = 256;

inline unsigned grid_for(size_t n) { return (unsigned)((n + BLK - 1) / BLK); }

// V consecutive floats: one 16-byte access when V == 4 (p 16-byte aligned), scalar accesses otherwise
template <int V>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&o)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = p[j];
    }
}

template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&o)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] = o[j];
    }
}

// max |v| of a block into *out (float bits of a non-negative value order like unsigned ints): wave shuffles, LDS across the
// waves, ONE atomic per block.  The kernels that use it run grid-stride with a capped grid, so a tensor costs a few
// thousand atomics (one per wave on a single address made bn_bwd_apply_kernel 9x slower: measured, round 2).
constexpr unsigned AMAX_GRID = 2048;

__device__ __forceinline__ void block_absmax_to(float m, unsigned int* __restrict__ out) {
    __shared__ float wave_max[BLK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = wave_max[0];
#pragma unroll
        for (int w = 1; w < BLK / 64; ++w) b = fmaxf(b, wave_max[w]);
        atomicMax(out, __float_as_uint(b));
    }
}

// The per-channel sums over pixels run on a (blocks, cblocks) grid: `lanes` threads (a power of two) across the cv channel
// units of a pixel -- a unit is V channels -- and ppi = BLK / lanes pixel rows, so a block takes ppi pixels per iteration;
// block x covers ppb consecutive pixels, block y one group of `lanes` units.  16 iterations a block unless that asks for
// more than max_blocks blocks.
struct PixelSplit {
    int lanes, cblocks, ppi;
    size_t blocks, ppb;
};

inline PixelSplit split_pixels(size_t npix, int cv, size_t max_blocks) {
    PixelSplit s;
    s.lanes = 1;
    while (s.lanes < cv && s.lanes < BLK) s.lanes <<= 1;
    s.cblocks = (cv + s.lanes - 1) / s.lanes;
    s.ppi = BLK / s.lanes;
    s.blocks = (npix + (size_t)s.ppi * 16 - 1) / ((size_t)s.ppi * 16);
    if (s.blocks > max_blocks) s.blocks = max_blocks;
    if (s.blocks < 1) s.blocks = 1;
    s.ppb = (npix + s.blocks - 1) / s.blocks;
    s.blocks = (npix + s.ppb - 1) / s.ppb;
    return s;
}

// THE order in which the blocks' sums ([block][channel][NS]) become a channel's sums, so that the result does not depend on
// the order the blocks ran in (atomics: it does, at 1e-7 relative, enough to flip a ReLU mask element next to zero now and
// then).  A block of 256 threads takes 16 channels: thread (run = tid / 16, channel = tid % 16) adds the blocks run,
// run + 16, run + 32, ... in that order (eight loads in flight, added in block order), then the thread of run 0 adds the
// runs 1 .. 15 in sequence through LDS.  Returns true in the threads that then hold their channel `ch`'s sums in S.
template <int NS>
__device__ __forceinline__ bool ordered_partials_sum(const float* __restrict__ partials, int nblocks, int c, int& ch,
                                                     float (&S)[NS]) {
    __shared__ float red[NS][BLK];
    const int tid = threadIdx.x, cl = tid & 15, run = tid >> 4;
    ch = blockIdx.x * 16 + cl;
#pragma unroll
    for (int k = 0; k < NS; ++k) S[k] = 0.f;
    if (ch < c) {
        int b = run;
        for (; b + 7 * 16 < nblocks; b += 8 * 16) {
            float p[8][NS];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int k = 0; k < NS; ++k) p[u][k] = partials[((size_t)(b + 16 * u) * c + ch) * NS + k];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int k = 0; k < NS; ++k) S[k] += p[u][k];
        }
        for (; b < nblocks; b += 16)
#pragma unroll
            for (int k = 0; k < NS; ++k) S[k] += partials[((size_t)b * c + ch) * NS + k];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][tid] = S[k];
    __syncthreads();
    if (run != 0 || ch >= c) return false;
    for (int r = 1; r < 16; ++r)
#pragma unroll
        for (int k = 0; k < NS; ++k) S[k] += red[k][r * 16 + cl];
    return true;
}

// The fixed tree over a block's threads: every thread has written red[k][threadIdx.x]; afterwards red[k][0] holds row k's
// sum, formed as (t + t+128), (t + t+64), ... whatever the timing.  One barrier before the tree and one after every level.
template <int ROWS>
__device__ __forceinline__ void block_tree_sum(float (&red)[ROWS][BLK]) {
    __syncthreads();
    for (int st = BLK / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
#pragma unroll
            for (int k = 0; k < ROWS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
        }
        __syncthreads();
    }
}

// K per-channel vectors staged in LDS once per block (c <= BN4_CMAX), par[k][i] = value(k, i): the vectors may be unaligned
// views into a flat parameter buffer, and 4 K scalar parameter loads per thread made the float4 kernels slower than the
// one-element ones.  Ends with the barrier.
constexpr int BN4_CMAX = 512;

template <int K, class F>
__device__ __forceinline__ void stage_channel_vectors(float (&par)[K][BN4_CMAX], int c, F value) {
    for (int i = threadIdx.x; i < c; i += BLK)
#pragma unroll
        for (int k = 0; k < K; ++k) par[k][i] = value(k, i);
    __syncthreads();
}

}  // namespace mpg::valu
