// conv_mfma_kernel: the fused convolution at MPG_PREC_F16X1 / MPG_PREC_F16X3 (what training runs), see mpgan_conv.h.
//
// Work decomposition.  One workgroup = 4 waves = (4*PT) x 32 output pixels x all NT*32 output
// channels; wave w owns tile rows [PT*w, PT*w+PT) (PT pixel tiles of 32 pixels) x NT cout tiles.
// v_mfma_f32_32x32x16_f16 computes D[cout][pixel] += W[cout][k] * X[k][pixel] (weights = A operand,
// pixels = B operand), so a lane ends with 4 consecutive channels of one pixel per accumulator quad.
// K runs over (segment, chunk of CGC channel groups, tap, group): per chunk the halo image of the
// tile is DMA'd once ([group][plane][pixel][16 B], conflict-free ds_read_b128) and double-buffered,
// the kh*kw taps are shifted windows of that image (im2col-free); weight stages (KS k-steps of 16)
// stream through a ring of R LDS slots, D = R-1 stages ahead of the MFMAs, one barrier per stage.
#include "mpgan_conv.h"

using namespace mpg::conv;

namespace {

// D2S: the launch of mpg_conv2d_fused_d2s (ConvArgsD2S, depth-to-space store); the instantiations with D2S false are
// those of mpg_conv2d_fused
template <int NT, int PREC, bool D2S = false>
__global__ __launch_bounds__(256, (NT >= 2 ? 2 : 3)) void conv_mfma_kernel(const typename KernelArgs<D2S>::type a_unused) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KArgs ap = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const auto& a = *ap;
    using P = Pipe<NT, PREC>;
    constexpr int PT = P::PT, TH = P::TH, KS = P::KS, WPLANE = P::WPLANE, WSTAGE = P::WSTAGE;
    constexpr int NI = P::NI, R = P::R, D = P::D;

    int* tapoff = reinterpret_cast<int*>(smem);
    char* img_lds = smem + TAPOFF_BYTES;              // two image buffers
    char* w_lds = img_lds + 2 * a.img_bytes;          // ring of R stage slots

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int r = lane & 31;
    const int hh = lane >> 5;

    // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so give each XCD
    // a contiguous run of tiles => neighbouring halos hit the same L2.
    int bid = blockIdx.x;
    const int nblk = gridDim.x;
    if ((nblk & 7) == 0) bid = (bid & 7) * (nblk >> 3) + (bid >> 3);
    const int tx = bid % a.tiles_x;
    const int t2 = bid / a.tiles_x;
    const int ty = t2 % a.tiles_y;
    const int n = t2 / a.tiles_y;
    const int y0 = ty * TH, x0 = tx * TW;

    f32x16 acc[PT][NT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[pt][nt][i] = 0.f;

    const EpiPre pre = epilogue_prefetch(ap, tid);   // bias and input scale of the epilogue: landed long before it runs
    for (int s = 0; s < ((a.dbg & 1) ? 0 : a.nseg); ++s) {
        const auto& sg = ap->seg[s];
        const int CGC = sg.cgc;
        const int TG = sg.kh * sg.kw * CGC;
        const int plane_b = sg.np * 16;             // bytes of one image plane
        const int group_b = plane_b * 2;            // hi + lo
        const int ppg = sg.np >> 6;                 // 1-KiB pieces per plane

        // tap/group -> LDS byte offset inside an image buffer
        for (int q = tid; q < sg.sc * KS * 2; q += 256) {
            int off = 0;
            if (q < TG) {
                const int tap = q / CGC;
                const int g = q - tap * CGC;
                const int dy = tap / sg.kw;
                const int dx = tap - dy * sg.kw;
                off = (dy * sg.iw + dx) * 16 + g * group_b;
            }
            tapoff[q] = off;
        }
        int pixb[PT];
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) pixb[pt] = ((PT * wave + pt) * sg.iw + r) * 16;

        // ---- image DMA: piece pc = 4*i + wave covers 64 pixels of one plane of one group ----
        const size_t plane_px = (size_t)sg.hs * sg.ws;
        auto dma_image = [&](int chunk) {
            char* buf = img_lds + (chunk & 1) * a.img_bytes;
            for (int i = 0; i < sg.ni_img; ++i) {
                const int pc = 4 * i + wave_u;                 // piece of this wave
                const int g = pc / (2 * ppg);                  // group within the chunk
                const int rem = pc - g * 2 * ppg;
                const int pl = rem / ppg;                      // plane: 0 hi, 1 lo
                const int p = (rem - pl * ppg) * 64 + lane;    // pixel of the halo image
                const int hy = p / sg.iw;
                const int hx = p - hy * sg.iw;
                const int yy = y0 - sg.pt + hy;
                const int xx = x0 - sg.pl + hx;
                const int grp = chunk * CGC + g;
                const char* src = a.zeros;
                if (g < CGC && grp < sg.cg_seg && hy < sg.ih && yy >= 0 && yy < a.h && xx >= 0 && xx < a.w &&
                    (PREC == 3 || pl == 0))
                    src = sg.x + ((((size_t)n * sg.cg_total + sg.g_off + grp) * 2 + pl) * plane_px +
                                  (size_t)(yy >> sg.upy) * sg.ws + (xx >> sg.up)) * 16;
                dma16(src, buf + pc * 1024);
            }
        };
        // ---- weight DMA: stage -> ring slot, linear copy ----
        const int total_stages = sg.nchunks * sg.sc;
        auto dma_stage = [&](int stage) {
            const int sidx = stage < total_stages ? stage : total_stages - 1;   // tail: harmless re-read
            const char* src = sg.w + (size_t)sidx * WSTAGE + tid * 16;
            char* dst = w_lds + (stage % R) * WSTAGE + wave_u * 1024;
#pragma unroll
            for (int i = 0; i < NI; ++i) dma16(src + i * 4096, dst + i * 4096);
        };

        dma_image(0);
#pragma unroll
        for (int d = 0; d < D; ++d) dma_stage(d);

        for (int ch = 0; ch < sg.nchunks; ++ch) {
            // short chunks: the image of this chunk was issued fewer than D-1 stages ago
            if (sg.sc < D) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const char* img = img_lds + (ch & 1) * a.img_bytes;
            for (int st = 0; st < sg.sc; ++st) {
                const int gst = ch * sg.sc + st;
                // stage gst (and everything older, incl. this chunk's image) has landed; all waves are
                // done with stage gst-1 and, at st == 0, with the previous chunk's image
                wait_dma_and_barrier<(D - 1) * NI>();
                if (st == 0 && ch + 1 < sg.nchunks) dma_image(ch + 1);
                dma_stage(gst + D);
                const char* wb = w_lds + (gst % R) * WSTAGE;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int toff = tapoff[2 * (st * KS + ks) + hh];
                    half8 b_hi[PT], b_lo[PT], a_hi[NT], a_lo[NT];
#pragma unroll
                    for (int pt = 0; pt < PT; ++pt) {
                        b_hi[pt] = *reinterpret_cast<const half8*>(img + pixb[pt] + toff);
                        if (PREC == 3) b_lo[pt] = *reinterpret_cast<const half8*>(img + plane_b + pixb[pt] + toff);
                    }
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        a_hi[nt] = *reinterpret_cast<const half8*>(wb + ((ks * NT + nt) * 64 + lane) * 16);
                        if (PREC == 3)
                            a_lo[nt] = *reinterpret_cast<const half8*>(wb + WPLANE + ((ks * NT + nt) * 64 + lane) * 16);
                    }
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int pt = 0; pt < PT; ++pt) {
                            acc[pt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[nt], b_hi[pt], acc[pt][nt], 0, 0, 0);
                            if (PREC == 3) {
                                acc[pt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo[nt], b_hi[pt], acc[pt][nt], 0, 0, 0);
                                acc[pt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[nt], b_lo[pt], acc[pt][nt], 0, 0, 0);
                            }
                        }
                }
            }
        }
        // drain the tail re-reads before the buffers (or the epilogue staging) are reused
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    conv_epilogue<NT, PT, D2S>(acc, ap, smem, n, y0, x0, wave, lane, pre);
}

template <bool D2S>
hipError_t launch(int prec, int nt, dim3 grid, size_t lds, hipStream_t st, const typename KernelArgs<D2S>::type& a) {
    const dim3 block(256);
    if (prec == MPG_PREC_F16X3) {
        switch (nt) {
            case 1: return mpg::launch_dyn_lds<conv_mfma_kernel<1, 3, D2S>>(grid, block, lds, st, a);
            case 2: return mpg::launch_dyn_lds<conv_mfma_kernel<2, 3, D2S>>(grid, block, lds, st, a);
            case 3: return mpg::launch_dyn_lds<conv_mfma_kernel<3, 3, D2S>>(grid, block, lds, st, a);
            default: return mpg::launch_dyn_lds<conv_mfma_kernel<4, 3, D2S>>(grid, block, lds, st, a);
        }
    }
    switch (nt) {
        case 1: return mpg::launch_dyn_lds<conv_mfma_kernel<1, 1, D2S>>(grid, block, lds, st, a);
        case 2: return mpg::launch_dyn_lds<conv_mfma_kernel<2, 1, D2S>>(grid, block, lds, st, a);
        case 3: return mpg::launch_dyn_lds<conv_mfma_kernel<3, 1, D2S>>(grid, block, lds, st, a);
        default: return mpg::launch_dyn_lds<conv_mfma_kernel<4, 1, D2S>>(grid, block, lds, st, a);
    }
}

}  // namespace

hipError_t mpg::conv::launch_conv_f16(int prec, int nt, dim3 grid, size_t lds, hipStream_t st, const ConvArgs& a) {
    return launch<false>(prec, nt, grid, lds, st, a);
}
hipError_t mpg::conv::launch_conv_f16(int prec, int nt, dim3 grid, size_t lds, hipStream_t st, const ConvArgsD2S& a) {
    return launch<true>(prec, nt, grid, lds, st, a);
}
