// Fused implicit-GEMM convolution on the gfx950 matrix cores.
//
// Data layout.  Activations travel between fused convolutions as "G8" tensors:
//     [N][CG = ceil(C/8)][2 planes: hi, lo][H][W][8 x fp16]
// (value = hi + lo, both fp16, exact to 2^-22; channels beyond C are zero).  A channel group of
// a tile row is therefore a contiguous run of 16-byte pixels, so the input tile with its halo AND
// the pre-packed weights both stream into LDS by LDS-DMA (global_load_lds_dwordx4): no VALU, no
// staging registers, deep prefetch.  fp32 NHWC enters / leaves through mpg_f32_to_g8 and the
// optional fp32 output of the epilogue.
//
// Replaces tf.nn.conv2d + bias + batch_norm + activation (+ residual 1x1 conv, + pixel_norm,
// + nearest upsample, + channel concat) of tools_wscale/GAN.py:80-119,472-474,501-541 and
// GAN/multipassGAN-4x.py:505-526, GAN/multipassGAN-out.py:220-237,357 (reference tree).
//
// This header is what the host decomposition (mpgan_conv_mfma.hip) and the kernel families agree on: the argument
// blocks, the pipeline traits, the epilogue both K loops end in, and one launch function per family (F16X1 / F16X3:
// mpgan_conv_f16.hip, F16F6: mpgan_conv_f6.hip, small channel counts: mpgan_conv_small.hip; the weight images they read
// are made in mpgan_conv_pack.hip).
#pragma once
#include "mpgan_internal.h"
#include "mpgan_mfma_dev.h"

namespace mpg::conv {

using namespace mpg::dev;

constexpr int TW = 32;              // tile cols == MFMA N dimension
constexpr int TAPOFF_BYTES = 1024;  // 256 tap offsets
// floats per pixel row of conv_epilogue's staging area (32 rows per wave, behind the tap table): NT * 32 channels + pad
constexpr int epi_rowf(int nt) { return nt * 32 + 4; }

struct SegArgs {
    const char* x;        // G8 tensor
    const char* w;        // packed weights
    int cg_seg;           // channel groups consumed
    int cg_total, g_off;  // groups of the tensor, first group consumed
    int kh, kw;
    int up, upy;          // source pixel = (y >> upy, x >> up): upy == up, or 0 for a column-only upsample (up_x_only)
    int cgc, nchunks, sc; // groups per chunk, chunks, weight stages per chunk
    int ih, iw;           // LDS image: (TH + kh - 1) x (TW + kw - 1) pixels
    int pt, pl;           // SAME padding before
    int hs, ws;           // source height / width (h >> upy, w >> up)
    int np;               // pixels per image plane, padded to a multiple of 64
    int ni_img;           // image DMA instructions per thread per chunk
    int direct;           // F16F6, 1x1 over >= 2 groups: B fragments straight from memory, K runs over groups
    int tp;               // F16F6: tap slots per channel group (kh*kw, or rounded up to 8 when below 16)
    int pref;             // F16F6: the B fragments of stage st + 1 may be read during stage st (seg_shape)
};

struct ConvArgs {
    int n, h, w, cout, nseg;
    SegArgs seg[MPG_MAX_SEG];
    const float* bias;
    int act;
    float leak;
    int pn;
    float pn_eps;
    const float* post_add;
    int pa_stride, pa_coff;
    // The outputs may be a channel window of wider tensors (mpg_conv2d_fused_window): the host folds the window's first
    // channel into y and y_g8, and what the stores still need of the whole tensor are these two strides (cout and
    // ceil(cout / 8) in a launch of mpg_conv2d_fused).  Kernel arguments like the rest: they stay in SGPRs.
    int y_stride;         // floats per pixel of the fp32 output
    int cg_img;           // channel groups per image of the G8 output
    float* y;             // fp32 NHWC output or null (channel 0 of the launch)
    char* y_g8;           // G8 output (planes hi16, lo16) or null (group 0 of the launch)
    const float* in_amax; // inputs were multiplied by pow2_scale(*in_amax): the accumulators are divided by it
    const char* zeros;    // >= 16 zero bytes (source of out-of-image pixels)
    int img_bytes;        // bytes of one LDS image buffer (max over segments)
    int tap_bytes;        // F16F6: bytes of the tap-offset table at the start of LDS
    int tiles_x, tiles_y;
    int dbg;              // development probes: 1 skip K loop, 2 skip stores
};

typedef const __attribute__((address_space(4))) ConvArgs* KArgs;

// mpg_conv2d_fused_d2s: the launch's arguments followed by the geometry of the depth-to-space output (block size 2,
// tf.depth_to_space of GAN.pixel_shuffle, GAN.py:554-560).  Only the D2S instantiations take this larger argument
// block; the kernels of mpg_conv2d_fused keep theirs.
struct ConvArgsD2S {
    ConvArgs a;
    int cs;               // channels of the shuffled tensor (c_total / 4)
    int coff;             // pre-shuffle channel of this launch's output channel 0
    int cg;               // G8 groups of the shuffled tensor (cs / 8)
};
typedef const __attribute__((address_space(4))) ConvArgsD2S* KArgsD2S;

template <bool D2S>
struct KernelArgs { typedef ConvArgs type; };
template <>
struct KernelArgs<true> { typedef ConvArgsD2S type; };

// pre-shuffle channel coff + c of pixel (py, px) -> channel cc of pixel `pix` (row-major in the 2H x 2W image) of the
// shuffled tensor: coff + c = (2 i + j) cs + cc, pix = (2 py + i) 2W + 2 px + j
struct D2SPos {
    int cc;
    size_t pix;
};
__device__ __forceinline__ D2SPos d2s_pos(const KArgsD2S dp, int py, int px, int c) {
    const int gc = dp->coff + c;
    const int k = gc / dp->cs;
    D2SPos p;
    p.cc = gc - k * dp->cs;
    p.pix = (size_t)(2 * py + (k >> 1)) * (2 * dp->a.w) + 2 * px + (k & 1);
    return p;
}

// Per (NT, PREC) pipeline shape (the host reads it through shape_of()).
template <int NT, int PREC>
struct Pipe {
    static constexpr int WAVES = 4;
    static constexpr int NPL = (PREC == 3) ? 2 : 1;
    static constexpr int PT = (NT >= 3) ? 2 : 4;       // pixel tiles (tile rows) per wave
    static constexpr int TH = 4 * PT;                  // tile rows per workgroup
    static constexpr int KS = (PREC == 3) ? ((NT == 4 || NT == 2) ? 1 : 2) : ((NT == 4 || NT == 2) ? 2 : 4);
    static constexpr int R = (NT == 3) ? 3 : 4;
    static constexpr int D = R - 1;
    static constexpr int WPLANE = KS * NT * 1024;
    static constexpr int WSTAGE = WPLANE * NPL;
    static constexpr int NI = WSTAGE / 4096;
    static constexpr int ROWF = epi_rowf(NT);
    static_assert(WSTAGE % 4096 == 0, "stage must be a whole number of 256 x 16-byte pieces");
};

template <int NT>
struct Pipe6 {
    static constexpr int WAVES = 8;
    static constexpr int OCC = (NT == 1) ? 4 : 2;          // waves per SIMD the kernel is compiled for (256 or 128 registers)
    static constexpr int PT = 16 / WAVES;                  // tile rows per wave
    static constexpr int TH = 16;
    static constexpr int KS = 4;                           // fp16 k-steps per stage: 8 tap slots
    static constexpr int WF16 = KS * NT * 1024;
    static constexpr int WF6 = NT * 2048;                  // one bf6 plane: NT x [2 halves][64 lanes][16 B]: 24 B of codes, scales, pad
    static constexpr int WSTAGE = WF16 + 2 * WF6;          // 8 * NT KiB
    static constexpr int R = 3;
    static constexpr int D = R - 1;
    static constexpr int NI = WSTAGE / (WAVES * 1024);
    static constexpr int ROWF = epi_rowf(NT);
    static_assert(WSTAGE % (WAVES * 1024) == 0, "stage must be a whole number of per-wave pieces");
};

// What conv_epilogue reads from memory besides post_add, fetched once per block IN FRONT of the K loop (the K loop's
// drain covers the loads, so no wave waits for memory between its last MFMA and its stores): thread c < cout holds
// bias[c], every other thread (and every thread of a launch without bias) zero; cout <= 128 <= threads of a block.
struct EpiPre {
    float bias;
    float amax;   // *in_amax, or 0 (pow2_scale(0) == 1)
};
__device__ __forceinline__ EpiPre epilogue_prefetch(const KArgs ap, int tid) {
    const auto& a = *ap;
    EpiPre pre;
    pre.bias = (a.bias != nullptr && tid < a.cout) ? a.bias[tid] : 0.f;
    pre.amax = a.in_amax != nullptr ? *a.in_amax : 0.f;
    return pre;
}

// One tile row: acc = act(acc * unscale + bias), zero beyond cout.  bl: the block's 128 staged bias values in LDS, one
// ds_read_b128 per quad (read again for every tile row: a wave has no registers to keep them in).
// tanh (the last layer of a network at most) has a branch per element, and unrolled over a tile row its results would
// not fit beside the accumulators: the row's linear part goes to this lane's slots of the wave's staging rows, tanhf runs
// over them in a rolled loop, and the row comes back.
template <int ACT, int NT>
__device__ __forceinline__ void epilogue_bias_act(f32x16 (&acc)[NT], const float* bl, float* stg_lane, float unscale, float leak, int cout,
                                                  int hh) {
    if constexpr (ACT == MPG_ACT_TANH) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int co0 = nt * 32 + 8 * q4 + 4 * hh;
                const float4 bq = *reinterpret_cast<const float4*>(bl + co0);
                *reinterpret_cast<float4*>(stg_lane + co0) =
                    make_float4(acc[nt][4 * q4] * unscale + bq.x, acc[nt][4 * q4 + 1] * unscale + bq.y,
                                acc[nt][4 * q4 + 2] * unscale + bq.z, acc[nt][4 * q4 + 3] * unscale + bq.w);
            }
#pragma nounroll
        for (int k = 0; k < NT * 16; ++k) {
            const int c = (k >> 2) * 8 + 4 * hh + (k & 3);
            stg_lane[c] = c < cout ? tanhf(stg_lane[c]) : 0.f;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 v = *reinterpret_cast<const float4*>(stg_lane + nt * 32 + 8 * q4 + 4 * hh);
                acc[nt][4 * q4] = v.x;
                acc[nt][4 * q4 + 1] = v.y;
                acc[nt][4 * q4 + 2] = v.z;
                acc[nt][4 * q4 + 3] = v.w;
            }
        return;
    }
    // the bias quads of cout tile nt + 1 are read while tile nt is worked on and no further ahead (the scheduling barriers):
    // 8 registers per lane in flight instead of the 16 NT an unbounded look-ahead may take beside the accumulators
    float4 bq[2][4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) bq[0][q4] = *reinterpret_cast<const float4*>(bl + 8 * q4 + 4 * hh);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (nt + 1 < NT) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) bq[(nt + 1) & 1][q4] = *reinterpret_cast<const float4*>(bl + (nt + 1) * 32 + 8 * q4 + 4 * hh);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int co0 = nt * 32 + 8 * q4 + 4 * hh;
            const float b4[4] = {bq[nt & 1][q4].x, bq[nt & 1][q4].y, bq[nt & 1][q4].z, bq[nt & 1][q4].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = mpg::apply_act(acc[nt][4 * q4 + i] * unscale + b4[i], ACT, leak);
                if (co0 + i >= cout) v = 0.f;
                acc[nt][4 * q4 + i] = v;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The values of one tile row: bias and activation (one uniform switch per tile row around code that holds a single
// activation), then pixel norm (per-pixel sum over the lane's values + one __shfl_xor 32)
template <int NT>
__device__ __forceinline__ void epilogue_row_values(f32x16 (&acc)[NT], const KArgs ap, const float* bl, float* stg_lane, float unscale,
                                                    int hh) {
    const auto& a = *ap;
    switch (a.act) {
        case MPG_ACT_RELU: epilogue_bias_act<MPG_ACT_RELU>(acc, bl, stg_lane, unscale, a.leak, a.cout, hh); break;
        case MPG_ACT_LRELU: epilogue_bias_act<MPG_ACT_LRELU>(acc, bl, stg_lane, unscale, a.leak, a.cout, hh); break;
        case MPG_ACT_TANH: epilogue_bias_act<MPG_ACT_TANH>(acc, bl, stg_lane, unscale, a.leak, a.cout, hh); break;
        default: epilogue_bias_act<MPG_ACT_NONE>(acc, bl, stg_lane, unscale, a.leak, a.cout, hh); break;
    }
    if (a.pn) {
        float ss = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) ss += acc[nt][i] * acc[nt][i];
        ss += __shfl_xor(ss, 32);
        const float sc = rsqrtf(ss / (float)a.cout + a.pn_eps);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nt][i] *= sc;
    }
}

// D2S: every output goes to its depth-to-space position (ConvArgsD2S; no pixel norm, no post-add); only the store
// addresses differ.  Both K loops end behind `s_waitcnt vmcnt(0)` + barrier (a launch that skips them, dbg & 1, has not
// touched LDS at all), so the tap table at the start of LDS is dead: the bias (EpiPre, one value per thread) is staged
// there for the block.  The launch's output kind is decided once, in front of the tile rows: the G8-only rows and the
// LDS-staged rows are two loops, so that no load of the staged path (post_add) is pending, as far as the compiler can
// tell, where the G8-only path writes registers or stores.
template <int NT, int PT, bool D2S = false>
__device__ __forceinline__ void conv_epilogue(f32x16 (&acc)[PT][NT], const KArgs ap, char* smem, int n, int y0, int x0,
                                              int wave, int lane, const EpiPre pre) {
    const auto& a = *ap;
    const KArgsD2S dp = reinterpret_cast<KArgsD2S>(ap);
    const int r = lane & 31;
    const int hh = lane >> 5;
    // accumulator element i of n-tile nt: output channel nt*32 + 8*(i>>2) + 4*hh + (i&3), pixel r.
    constexpr int ROWF = epi_rowf(NT);
    static_assert(128 * sizeof(float) <= TAPOFF_BYTES, "the staged bias must fit in front of the staging rows");
    float* bl = reinterpret_cast<float*>(smem);
    float* stg = reinterpret_cast<float*>(smem + TAPOFF_BYTES) + wave * (32 * ROWF);
    const int cg_out = (a.cout + 7) >> 3;
    const float unscale = 1.f / mpg::pow2_scale(pre.amax);
    {
        // every thread takes its prefetched value here: behind the drain the counter is at zero, and a register the
        // compiler still believed to be waiting for its load would cost a wait wherever it is written next
        float bv = pre.bias;
        asm volatile("" : "+v"(bv));
        if (wave < 2) bl[wave * 64 + lane] = bv;
    }
    __syncthreads();
    const int npx = min(32, a.w - x0);
    const size_t plane_px = (size_t)a.h * a.w;
    if (a.y == nullptr && a.post_add == nullptr) {
        // G8 output only (every launch between two fused convolutions): no LDS staging and no load from memory, so
        // nothing waits between the tile rows and their stores leave back to back.  An accumulator quad holds
        // channels 8 q + 4 hh .. + 3 of pixel r, i.e. the two lanes (r, hh = 0 / 1) share every 8-channel group.
        // v_permlane32_swap trades the upper half-wave of one quad register with the lower half-wave of another:
        // after four swaps lane (r, 0) holds all 8 channels of group gA and lane (r, 1) all 8 of group gB, ready
        // to be split into the hi / lo planes and stored as 512-byte runs per plane and half-wave.
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            const int py = y0 + PT * wave + pt;
            epilogue_row_values<NT>(acc[pt], ap, bl, stg + r * ROWF, unscale, hh);
            if (py < a.h && r < npx && !(a.dbg & 2)) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int qp = 0; qp < 2; ++qp) {
                        float v[8];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            typedef unsigned v2u_t __attribute__((ext_vector_type(2)));
                            const v2u_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[pt][nt][8 * qp + i]),
                                                                              __float_as_uint(acc[pt][nt][8 * qp + 4 + i]), false, false);
                            v[i] = __uint_as_float(sw[0]);
                            v[4 + i] = __uint_as_float(sw[1]);
                        }
                        const int cg = nt * 4 + 2 * qp + hh;
                        if (cg < cg_out) {
                            char* dst;
                            size_t plane_out = plane_px;
                            if constexpr (D2S) {
                                const D2SPos q = d2s_pos(dp, py, x0 + r, 8 * cg);
                                plane_out = 4 * plane_px;
                                dst = a.y_g8 + ((((size_t)n * dp->cg + (q.cc >> 3)) * 2) * plane_out + q.pix) * 16;
                            } else {
                                dst = a.y_g8 + ((((size_t)n * a.cg_img + cg) * 2) * plane_px + (size_t)py * a.w + x0 + r) * 16;
                            }
                            half8 hi, lo;
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                hi[j] = (_Float16)v[j];
                                lo[j] = (_Float16)(v[j] - (float)hi[j]);
                            }
                            __builtin_nontemporal_store(hi, reinterpret_cast<half8*>(dst));
                            __builtin_nontemporal_store(lo, reinterpret_cast<half8*>(dst + plane_out * 16));
                        }
                    }
            }
        }
        return;
    }
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int py = y0 + PT * wave + pt;
        epilogue_row_values<NT>(acc[pt], ap, bl, stg + r * ROWF, unscale, hh);
        // stage this wave's 32 pixels x cout through LDS ([pixel][cout] rows padded by 16 B); the 32
        // pixels of a tile row are contiguous in every output layout, so all stores are whole runs
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int co0 = nt * 32 + 8 * q4 + 4 * hh;
                *reinterpret_cast<float4*>(stg + r * ROWF + co0) =
                    make_float4(acc[pt][nt][4 * q4], acc[pt][nt][4 * q4 + 1], acc[pt][nt][4 * q4 + 2], acc[pt][nt][4 * q4 + 3]);
            }
        if (py < a.h && !(a.dbg & 2)) {
            const size_t pix0 = ((size_t)n * a.h + py) * a.w + x0;
            if (a.post_add != nullptr) {
                // add into the staged tile first, so both output formats carry it
                const float* pa = a.post_add + pix0 * a.pa_stride + a.pa_coff;
                // four loads in flight per lane; an index past the tile re-reads the tile's last element and adds nothing
                const int total = npx * a.cout;
                for (int f0 = lane; f0 < total; f0 += 256) {
                    float pv[4];
                    int so[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int f = min(f0 + 64 * j, total - 1);
                        const int p = f / a.cout;
                        const int c = f - p * a.cout;
                        so[j] = p * ROWF + c;
                        pv[j] = pa[(size_t)p * a.pa_stride + c];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        asm volatile("" : "+v"(pv[j]));      // all four are taken here: none stays pending behind the loop
                        if (f0 + 64 * j < total) stg[so[j]] += pv[j];
                    }
                }
            }
            if (D2S && a.y != nullptr) {
                // runs of up to cs channels per shuffled pixel; float4 when no run boundary splits a quad
                float* img = a.y + (size_t)n * 4 * a.h * a.w * dp->cs;
                const int total = npx * a.cout;
                if (((dp->cs | dp->coff | a.cout) & 3) == 0) {
                    for (int f = lane * 4; f < total; f += 256) {
                        const int p = f / a.cout;
                        const int c = f - p * a.cout;
                        const D2SPos q = d2s_pos(dp, py, x0 + p, c);
                        *reinterpret_cast<float4*>(img + q.pix * dp->cs + q.cc) = *reinterpret_cast<const float4*>(stg + p * ROWF + c);
                    }
                } else {
                    for (int f = lane; f < total; f += 64) {
                        const int p = f / a.cout;
                        const int c = f - p * a.cout;
                        const D2SPos q = d2s_pos(dp, py, x0 + p, c);
                        img[q.pix * dp->cs + q.cc] = stg[p * ROWF + c];
                    }
                }
            } else if (a.y != nullptr) {
                // runs of cout channels per pixel, y_stride floats apart (one run of npx * cout where the launch owns the
                // whole tensor); float4 when every run starts and ends on 16 bytes
                float* dst = a.y + pix0 * a.y_stride;
                const int total = npx * a.cout;
                if (((a.cout | a.y_stride) & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0) {
                    for (int f = lane * 4; f < total; f += 256) {
                        const int p = f / a.cout;
                        const int c = f - p * a.cout;
                        *reinterpret_cast<float4*>(dst + p * a.y_stride + c) = *reinterpret_cast<const float4*>(stg + p * ROWF + c);
                    }
                } else {
                    for (int f = lane; f < total; f += 64) {
                        const int p = f / a.cout;
                        const int c = f - p * a.cout;
                        dst[p * a.y_stride + c] = stg[p * ROWF + c];
                    }
                }
            }
            if (a.y_g8 != nullptr) {
                // lane (pixel r, half hh) converts channel group 2 i + hh and writes BOTH of its planes (hi16, lo16): no
                // divergence between the halves, 512-byte runs per plane and half-wave; streamed (read once or twice by
                // the next launch), so the stores do not push the weights out of L2
                if (r < npx) {
                    for (int cg = hh; cg < cg_out; cg += 2) {
                        const float4 v0 = *reinterpret_cast<const float4*>(stg + r * ROWF + cg * 8);
                        const float4 v1 = *reinterpret_cast<const float4*>(stg + r * ROWF + cg * 8 + 4);
                        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                        char* dst;
                        size_t plane_out = plane_px;
                        if constexpr (D2S) {
                            const D2SPos q = d2s_pos(dp, py, x0 + r, 8 * cg);
                            plane_out = 4 * plane_px;
                            dst = a.y_g8 + ((((size_t)n * dp->cg + (q.cc >> 3)) * 2) * plane_out + q.pix) * 16;
                        } else {
                            dst = a.y_g8 + ((((size_t)n * a.cg_img + cg) * 2) * plane_px + (size_t)py * a.w + x0 + r) * 16;
                        }
                        half8 hi, lo;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            hi[j] = (_Float16)v[j];
                            lo[j] = (_Float16)(v[j] - (float)hi[j]);
                        }
                        __builtin_nontemporal_store(hi, reinterpret_cast<half8*>(dst));
                        __builtin_nontemporal_store(lo, reinterpret_cast<half8*>(dst + plane_out * 16));
                    }
                }
            }
        }
    }
}

// ---- host side ----
// What the host needs of a kernel's pipeline; every field is read from Pipe<NT, PREC> / Pipe6<NT>.
struct Shape {
    int th;        // tile rows per workgroup
    int ks;        // k-steps (two tap slots each) per weight stage
    int waves;
    int wstage;    // bytes of a weight stage
    int ring;      // bytes of the weight ring
    int rowf;      // floats per staging row of conv_epilogue
};
// prec one of MPG_PREC_*, nt = ceil(cout / 32) in 1..4: the callers have checked both
const Shape& pipe_shape(int nt, int prec);

struct SegShape {
    int cgc, nchunks, sc, np, ni_img, img_bytes, direct, tp, pref;
    int slots;     // entries of the tap-offset table
    int stages;    // weight stages of the packed segment
};
// The K decomposition of one segment at `prec`
SegShape seg_shape(int kh, int kw, int cin, int nt, int prec);

constexpr size_t LDS_MAX = 160 * 1024;     // of a CU, so the most a workgroup can have

// bytes of the packed MFMA weight image of a layer, 0 where the layer is not available at `prec`
size_t pack_base_bytes(int kh, int kw, int cin, int cout, int prec);
// Layers with at most 8 input and 8 output channels (the first and last residual blocks of gen_resnet:
// 1->2->8 and 8->2->1) are not matrix work: they run on conv_small_kernel, which reads a plain fp32
// table [tap][ci 8][co 8] appended to the packed weights.
inline bool small_layer(int cin, int cout) { return cin <= 8 && cout <= 8; }
// SAME padding in front of a k-wide filter; pad_hi moves the odd pixel of an even filter to the front
inline int pad_before(int k, int pad_hi) { return pad_hi ? k / 2 : (k - 1) / 2; }
// the checks of segment s that do not depend on the kernel it runs on
int check_segment(const mpg_conv_desc* d, int s);

// One launch of the fused convolution per kernel family; nt = cout tiles picks the instantiation.  The MFMA ones return
// the error of raising the dynamic-LDS limit and leave the launch's own in hipGetLastError().
hipError_t launch_conv_f16(int prec, int nt, dim3 grid, size_t lds, hipStream_t st, const ConvArgs& a);
hipError_t launch_conv_f16(int prec, int nt, dim3 grid, size_t lds, hipStream_t st, const ConvArgsD2S& a);
hipError_t launch_conv_f6(int nt, dim3 grid, size_t lds, hipStream_t st, const ConvArgs& a);
// small-channel layers (every cin and cout <= 8, plain epilogue): conv_small_kernel
int launch_small(hipStream_t stream, const mpg_conv_desc* d);

}  // namespace mpg::conv
