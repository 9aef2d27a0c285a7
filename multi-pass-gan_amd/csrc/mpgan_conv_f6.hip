// ---------------------------------------------------------------------------------------------
// MPG_PREC_F16F6: one fp16 product a_hi*w_hi plus the two correction products a_lo*w_hi and a_hi*w_lo as
// block-scaled bf6 (e3m2) products: v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = blgp = 3 runs K = 64 in the
// 32 cycles of ONE fp16 32x32x16 (K = 16), so the two corrections cost half an fp16 product together:
// 1.5 fp16-equivalent matrix units per MAC (the fp8 form of round 1-2 cost 2: a mixed or fp8 operand pair
// runs at half this rate; tools/probes/probe_bf6.hip).
//
// Activations are read in the exact G8 flavour (hi16, lo16).  The bf6 operands of a lane -- the 32 K values
// (4 tap slots x 8 channels) it holds for the K = 64 instruction -- are made in registers from the very fp16
// fragments the fp16 products use: v_cvt_scalef32_pk32_bf6_f16 converts 32 values in one instruction with a
// power-of-two block scale, which is PER LANE here: 2^-18 times the binade of the largest |a_hi| among the
// lane's 32 values (three-input packed max / min trees), and 2^-12 of that for the a_lo block.  The E8M0
// bytes of both go to the MFMA's scale operand: true MX block scaling, no per-tensor exponent, nothing the
// producer has to know -- an activation tensor of any range and any mix of channel scales keeps the
// corrections (the fixed exponents of the fp8 flavour lost them outside |v| in 1e-2..112).
// Weights: bf6 planes packed per stage with one E8M0 byte per (output channel, K block of 32) and plane.
//
// One workgroup = 8 waves = 16 tile rows x 32 pixels, two tile rows per wave; a weight stage is one macro-step of 8 tap
// slots (K = 64): [4 fp16 k-steps][w_hi6][w_lo6].  The slots of a segment form one stream over its channel groups
// (slot = group * tp + tap), so a stage may end one group and begin the next; every group has its own LDS image.
// ---------------------------------------------------------------------------------------------
#include "mpgan_conv.h"

using namespace mpg::conv;

namespace {

#ifndef MPG_AH
#define MPG_AH 2
#endif
// development switches of the F16F6 K loop (tools/build_variants.sh builds one library per setting, tools/probe_variants.py
// times them against each other on one box):
//   MPG_WD          bf6 weight planes read MPG_WD correction steps ahead of their MFMAs (MPG_WD + 1 register buffers)
//   MPG_DIAG6       timing-only builds (results are garbage): 1 = no correction phase at all, 2 = no block-scale / conversion
//                   VALU work (the bf6 operands are whatever the fp16 fragments hold), 4 = no image copies in the K loop,
//                   8 = no weight copies in the K loop
#ifndef MPG_WD
#define MPG_WD 1
#endif
// (measured and dropped in round 3, like in round 2: four cout tiles as 4 waves x (4 tile rows x 4 cout tiles), one wave per
// SIMD with the 256 accumulators in AccVGPRs: hipcc allocates 142 VGPRs + 256 AGPRs but keeps 1088 bytes of scratch per lane
// in the K loop -- 15.8 ms against 0.64 ms; that shape needs hand-allocated registers: profiles/r03/kloop_variants.md)
#ifndef MPG_DIAG6
#define MPG_DIAG6 0
#endif
//   MPG_W0 0        the weight planes of correction step 0 are read at the head of the correction phase, not in front of the
//                   last fp16 group
#ifndef MPG_W0
#define MPG_W0 1
#endif
//   MPG_PIECES_AFTER 0   the LDS-DMA pieces of an fp16 group are issued in front of the group's operand wait (rounds 2-3)
#ifndef MPG_PIECES_AFTER
#define MPG_PIECES_AFTER 1
#endif
// (measured and dropped: the NT steps `w_lo6 x a_hi6` riding in the last NT fp16 groups of the stage, operands prefetched like
// the fp16 ones, only `w_hi6 x a_lo6` left as a separate phase: b1.B 650 us against 639, profiles/r03/kloop_variants.md;
// the second half of the waves running a stage's corrections BEFORE its fp16 groups: 265 spilled registers at four cout
// tiles, same file)
//   MPG_STAMPS 1    diagnostic build only: every wave accumulates, over the barrier intervals of its K loop, the s_memtime
//                   cycles (0) from the barrier release to its first MFMA wait satisfied, (1) in the fp16 groups, (2) in the
//                   correction steps, (3) waiting for the next barrier, and writes the four sums to
//                   y[(block * WAVES + wave) * 4 ..] when desc.reserved has bit 3 set (tools/probe_stamps.py).  With the
//                   barrier in mid-stage an interval is [head, corr(st), fp16(st + 1), wait], else [head, fp16, corr, wait]
#ifndef MPG_STAMPS
#define MPG_STAMPS 0
#endif
#if MPG_STAMPS
#define MPG_STAMP(v) asm volatile("s_memtime %0" : "=s"(v))
#else
#define MPG_STAMP(v)
#endif
// the a_hi correction step (0 .. NT-1) behind whose MFMAs the a_lo codes of tile row pt are made
constexpr int lo_step(int pt, int nt, int ptn) {
    const int s = nt - ptn + pt - 1;
    return s < 0 ? 0 : (s > nt - 1 ? nt - 1 : s);
}

typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v6i __attribute__((ext_vector_type(6)));
typedef _Float16 half32 __attribute__((ext_vector_type(32)));
typedef _Float16 half16 __attribute__((ext_vector_type(16)));

// 32 bytes of LDS as two 16-byte reads ([half][lane][16 B]: consecutive lanes read consecutive 16-byte words,
// which ds_read_b128 serves without bank conflicts; a [lane][32 B] layout is 2-way conflicted)
__device__ __forceinline__ v8i lds_read32(const char* p) {
    const v4i lo = *reinterpret_cast<const v4i*>(p);
    const v4i hi = *reinterpret_cast<const v4i*>(p + 1024);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The reads and waits are volatile asm: they stay in program order, which is what the counted waits count.
template <int OFF, class T>
__device__ __forceinline__ void ds_read16(T& dst, unsigned addr) {
    static_assert(sizeof(T) == 16 && OFF >= 0 && OFF < 65536, "one ds_read_b128");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}

// bookkeeping of the explicit schedule (all compile-time): fp16 group h = (k-step h / NT, cout tile h % NT) issues
// [PT B fragments when h % NT == 0] + 1 A fragment
constexpr int kx_cum(int h, int NT, int PT) { return h + PT * ((h + NT - 1) / NT); }
// reads that may still be outstanding when group g's MFMAs start: everything issued after group g's own fragments
constexpr int kx_allowed(int g, int NT, int PT, int AH) {
    const int G16 = 4 * NT;
    const int hi = g + AH + 1 < G16 ? g + AH + 1 : G16;
    return kx_cum(hi, NT, PT) - kx_cum(g + 1, NT, PT);
}

__device__ __forceinline__ half32 cat32(const half8& a, const half8& b, const half8& c, const half8& d) {
    const half16 lo = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    const half16 hi = __builtin_shufflevector(c, d, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23,
                                   24, 25, 26, 27, 28, 29, 30, 31);
}

// biased fp16 exponent (0..30) of the largest |x| among the 32 halves of a lane: packed three-input max and min
// trees (8 + 8 instructions; v_pk_maximum3_f16 has no |x| modifier), max(max, -min), the larger half, its exponent
__device__ __forceinline__ int block_exp16(const half32& v) {
    const v16i r = __builtin_bit_cast(v16i, v);
    int a0, a1, a2, a3, a4, a5, a6, a7, b0, b1, b2, b3, b4, b5, b6, b7, m2, m1;
#define MPG_MAX3(d, x, y, z) asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(y), "v"(z))
#define MPG_MIN3(d, x, y, z) asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(y), "v"(z))
    MPG_MAX3(a0, r[0], r[1], r[2]); MPG_MAX3(a1, r[3], r[4], r[5]); MPG_MAX3(a2, r[6], r[7], r[8]); MPG_MAX3(a3, r[9], r[10], r[11]);
    MPG_MAX3(a4, r[12], r[13], r[14]); MPG_MAX3(a5, a0, a1, r[15]); MPG_MAX3(a6, a2, a3, a4); MPG_MAX3(a7, a5, a6, a6);
    MPG_MIN3(b0, r[0], r[1], r[2]); MPG_MIN3(b1, r[3], r[4], r[5]); MPG_MIN3(b2, r[6], r[7], r[8]); MPG_MIN3(b3, r[9], r[10], r[11]);
    MPG_MIN3(b4, r[12], r[13], r[14]); MPG_MIN3(b5, b0, b1, r[15]); MPG_MIN3(b6, b2, b3, b4); MPG_MIN3(b7, b5, b6, b6);
#undef MPG_MAX3
#undef MPG_MIN3
    asm("v_pk_max_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(m2) : "v"(a7), "v"(b7));
    asm("v_pk_max_f16 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(m1) : "v"(m2));
    return (m1 >> 10) & 31;
}

// bf6 operands of a lane's 32 activation values.  With e = block_exp16 (every |a_hi| < 2^(e-14)):
//   hi block: codes of a_hi * 2^(18-e)  (< 16; the e3m2 range ends at 28), E8M0 byte e + 109
//   lo block: codes of a_lo * 2^(30-e)  (|a_lo| <= half an ulp of a_hi <= 2^(e-26)), E8M0 byte e + 97
// v_cvt_scalef32_pk32_bf6_f16 divides by its f32 scale operand (a power of two), rounds to nearest even and saturates.
#ifndef MPG_CVT_DIVIDES
#define MPG_CVT_DIVIDES 1
#endif
__device__ __forceinline__ float pow2_from_byte(int e8m0) {
#if MPG_CVT_DIVIDES
    return __builtin_bit_cast(float, e8m0 << 23);
#else
    return __builtin_bit_cast(float, (254 - e8m0) << 23);
#endif
}
__device__ __forceinline__ v8i widen6(const v6i& v) {
    return __builtin_shufflevector(v, v, 0, 1, 2, 3, 4, 5, -1, -1);
}
__device__ __forceinline__ v8i bf6_of(const half32& v, int e8m0) {
    return widen6(__builtin_amdgcn_cvt_scalef32_pk32_bf6_f16(v, pow2_from_byte(e8m0)));
}
constexpr int BF6 = 3;     // cbsz / blgp code of e3m2

// Two blocks share a CU.  With two to four cout tiles the 64 to 128 accumulator registers of a wave leave room for two waves
// per SIMD; with ONE cout tile a wave has 32, and the kernel is compiled for 128 registers (Pipe6<1>::OCC = 4): four waves
// per SIMD, so that the in-order chain of a wave's stage (fragment reads, fp16 MFMAs, block maxima and conversions, a_lo
// reads, bf6 MFMAs, barrier) runs under the MFMAs of three other waves instead of one.
template <int NT>
__global__ __launch_bounds__(Pipe6<NT>::WAVES * 64, Pipe6<NT>::OCC) void conv_mfma_f6_kernel(const ConvArgs a_unused) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KArgs ap = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const auto& a = *ap;
    using P = Pipe6<NT>;
    constexpr int WAVES = P::WAVES, PT = P::PT, TH = P::TH, WF16 = P::WF16, WF6 = P::WF6, WSTAGE = P::WSTAGE;
    constexpr int NI = P::NI, R = P::R, D = P::D, THREADS = WAVES * 64;
    constexpr bool FLAT = NT == 1;      // the 128-register kernel: one tile row at a time in the direct path, no if / else below

    int* tap16 = reinterpret_cast<int*>(smem);
    char* img_lds = smem + a.tap_bytes;
    char* w_lds = img_lds + 2 * a.img_bytes;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);

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
    // The K segments are independent partial sums.  Blocks that share a CU (workgroups go round-robin over the 8
    // XCDs, then over the 32 CUs of an XCD: co-resident blocks differ in bit 8 of the id) walk them in opposite
    // orders, so one block's HBM-bound direct 1x1 segment runs under the other's LDS / MFMA-bound 5x5 segment.
    const int seg_flip = (NT == 1 && a.nseg > 1) ? ((int)(blockIdx.x >> 8) & 1) : 0;
    for (int s0 = 0; s0 < ((a.dbg & 1) ? 0 : a.nseg); ++s0) {
        const int s = seg_flip ? a.nseg - 1 - s0 : s0;
        const auto& sg = ap->seg[s];
        // The lane's indices are derived again in every segment from an id the compiler cannot see through: lane-only
        // terms of the addresses below would else be hoisted out of the segment loop and held in registers across both
        // stage loops (the 128-register kernel has none to spare: they went to scratch).
        int tid_seg = threadIdx.x;
        asm volatile("" : "+v"(tid_seg));
        const int tid = tid_seg, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
        if (NT <= 2 && sg.direct) {
            // 1x1 segment over cg_seg >= 2 channel groups: no halo, so no LDS image.  The G8 rows are already
            // fragment-shaped (16 B per pixel and group): lane (pixel r, half hh) loads its B operands from
            // memory, a weight stage is one macro-step of 8 GROUPS (K = 64) instead of 8 taps.  Rows / columns
            // past the image edge re-read the last valid pixel; their outputs are never stored.
            const unsigned plane_bytes = (unsigned)(sg.hs * sg.ws) * 16u;   // host: 16 planes < 2^31 bytes
            const unsigned gstride = 2u * plane_bytes;
            const char* xb = sg.x + ((size_t)n * sg.cg_total + sg.g_off) * gstride;   // uniform
            unsigned pixo[PT];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
                int yy = y0 + PT * wave + pt, xx = x0 + r;
                yy = (yy < a.h ? yy : a.h - 1) >> sg.upy;
                xx = (xx < a.w ? xx : a.w - 1) >> sg.up;
                pixo[pt] = (unsigned)(yy * sg.ws + xx) * 16u;
            }
            const int glast = sg.cg_seg - 1;
            auto dma_stage_d = [&](int stage) {
                const int sidx = stage < sg.sc ? stage : sg.sc - 1;
                const char* src = sg.w + (size_t)sidx * WSTAGE + tid * 16;
                char* dst = w_lds + (stage % R) * WSTAGE + wave_u * 1024;
#pragma unroll
                for (int i = 0; i < NI; ++i) dma16(src + i * (THREADS * 16), dst + i * (THREADS * 16));
            };
#pragma unroll
            for (int d = 0; d < D; ++d) dma_stage_d(d);
            for (int st = 0; st < sg.sc; ++st) {
                wait_dma_and_barrier<(D - 1) * NI>();
                dma_stage_d(st + D);
                const char* wb = w_lds + (st % R) * WSTAGE;
                const char* xs = xb + (size_t)st * 8 * gstride;   // uniform: first group of this macro-step
                const int grem = glast - st * 8;
                if constexpr (FLAT) {
                    // One tile row at a time, on the explicit reads and counted waits of the image path: the weight fragments
                    // of a row are read again for the next one and live in eight registers, both planes of a pixel share
                    // the lane's offset.  LDS reads in order: A(0) A(1) | A(2) | A(3) | w_lo6 | w_hi6, each group behind
                    // the MFMA that frees its registers.
                    const unsigned a_base = lds_off(wb) + (unsigned)lane * 16u;
                    // (opaque, so that they stay the scalar bases of the loads: folded into the lanes' offsets they would
                    // cost a 64-bit address per load)
                    const char* xs_hi = xs;
                    const char* xs_lo = xs + plane_bytes;
                    asm volatile("" : "+s"(xs_hi), "+s"(xs_lo));
                    static_for<0, PT>([&](auto qc) {
                        constexpr int q = decltype(qc)::value;
                        half8 b_hi[4], b_lo[4], aq[2];
                        v4i wl[2], wh[2];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            int g = 2 * j + hh;
                            g = g < grem ? g : grem;                 // groups past the segment: zero weights
                            const unsigned vo = pixo[q] + g * gstride;
                            typedef const __attribute__((address_space(1))) half8* gmem;     // (the asm hid where they point)
                            b_hi[j] = __builtin_nontemporal_load((gmem)(xs_hi + vo));   // read once
                            b_lo[j] = __builtin_nontemporal_load((gmem)(xs_lo + vo));
                        }
                        ds_read16<0>(aq[0], a_base);
                        ds_read16<1024>(aq[1], a_base);
                        static_for<0, 4>([&](auto jc) {
                            constexpr int j = decltype(jc)::value;
                            lgkm_wait<(j < 3 ? 1 : 2)>();           // behind A(j): A(j + 1), or the two halves of w_lo6
                            tie(aq[j & 1]);
                            acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq[j & 1], b_hi[j], acc[q][0], 0, 0, 0);
                            if constexpr (j < 2) {
                                ds_read16<(j + 2) * 1024>(aq[j & 1], a_base);
                            } else if constexpr (j == 2) {
                                ds_read16<WF16 + WF6>(wl[0], a_base);
                                ds_read16<WF16 + WF6 + 1024>(wl[1], a_base);
                            } else {
                                ds_read16<WF16>(wh[0], a_base);
                                ds_read16<WF16 + 1024>(wh[1], a_base);
                            }
                        });
                        const half32 bh = cat32(b_hi[0], b_hi[1], b_hi[2], b_hi[3]);
                        const int e = block_exp16(bh);
                        const v8i hi6 = bf6_of(bh, e + 109);
                        const v8i lo6 = bf6_of(cat32(b_lo[0], b_lo[1], b_lo[2], b_lo[3]), e + 97);
                        const int sb = (e + 109) | (e + 97) << 8;
                        lgkm_wait<2>();
                        tie(wl[0]);
                        tie(wl[1]);
                        const v8i w_lo = __builtin_shufflevector(wl[0], wl[1], 0, 1, 2, 3, 4, 5, 6, 7);
                        acc[q][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w_lo, hi6, acc[q][0], BF6, BF6, 1, w_lo[6], 0, sb);
                        lgkm_wait<0>();
                        tie(wh[0]);
                        tie(wh[1]);
                        const v8i w_hi = __builtin_shufflevector(wh[0], wh[1], 0, 1, 2, 3, 4, 5, 6, 7);
                        acc[q][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w_hi, lo6, acc[q][0], BF6, BF6, 0, w_hi[6], 1, sb);
                    });
                    continue;
                }
                // two tile rows at a time: all 32 operand fragments of a macro-step would not fit next to the accumulators
                // (the weights are re-read from LDS for every part)
                constexpr int PH = 2;
                static_for<0, PT / PH>([&](auto hc) {
                    constexpr int p0 = decltype(hc)::value * PH;
                    half8 b_hi[4][PH], b_lo[4][PH];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        int g = 2 * j + hh;
                        g = g < grem ? g : grem;                 // groups past the segment: zero weights
#pragma unroll
                        for (int q = 0; q < PH; ++q) {
                            b_hi[j][q] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(xs + (pixo[p0 + q] + g * gstride)));   // read once
                            b_lo[j][q] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(xs + (pixo[p0 + q] + g * gstride + plane_bytes)));
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const half8 a_hi = *reinterpret_cast<const half8*>(wb + ((j * NT + nt) * 64 + lane) * 16);
#pragma unroll
                            for (int q = 0; q < PH; ++q)
                                acc[p0 + q][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi[j][q], acc[p0 + q][nt], 0, 0, 0);
                        }
                    }
                    v8i hi6[PH], lo6[PH];
                    int sb[PH];
#pragma unroll
                    for (int q = 0; q < PH; ++q) {
                        const half32 bh = cat32(b_hi[0][q], b_hi[1][q], b_hi[2][q], b_hi[3][q]);
                        const half32 bl = cat32(b_lo[0][q], b_lo[1][q], b_lo[2][q], b_lo[3][q]);
                        const int e = block_exp16(bh);
                        hi6[q] = bf6_of(bh, e + 109);
                        lo6[q] = bf6_of(bl, e + 97);
                        sb[q] = (e + 109) | (e + 97) << 8;
                    }
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const v8i w_hi = lds_read32(wb + WF16 + nt * 2048 + lane * 16);
                        const v8i w_lo = lds_read32(wb + WF16 + WF6 + nt * 2048 + lane * 16);
#pragma unroll
                        for (int q = 0; q < PH; ++q) {
                            acc[p0 + q][nt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w_lo, hi6[q], acc[p0 + q][nt], BF6, BF6, 1, w_lo[6], 0, sb[q]);
                            acc[p0 + q][nt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w_hi, lo6[q], acc[p0 + q][nt], BF6, BF6, 0, w_hi[6], 1, sb[q]);
                        }
                    }
                });
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if constexpr (!FLAT) continue;
        }
        // FLAT: two `if`s in a row, the second on a value the compiler cannot tell from the first.  As the two arms of ONE
        // branch the accumulators that enter the segment stay allocated next to the ones the direct loop works on (the
        // arm that does not run hands them on): 32 registers the 128 do not have.
        if constexpr (FLAT) {
            if (__builtin_amdgcn_readfirstlane(sg.direct)) continue;
        }
        // K is ONE stream of tap slots over the channel groups of the segment: slot q = (group q / tp, tap q % tp),
        // eight slots per weight stage, so a stage may finish one group and start the next (25 taps x 16 groups =
        // 50 full stages instead of 16 x 4 with 7 empty slots each).  Group g's halo image lives in LDS buffer
        // g & 1; the offset table carries the buffer with the tap.
        const int T = sg.kh * sg.kw;
        const int G = sg.nchunks;
        const int NS = sg.sc;
        const int plane_b = sg.np * 16;
        const int ppg = sg.np >> 6;

        for (int q = tid; q < NS * 8; q += THREADS) {
            const int g = q / sg.tp;
            const int t = q - g * sg.tp;
            // Padding slots (t >= T, or past the last group) have zero weights but their pixels still enter the lane's
            // block maximum, i.e. the scale of the REAL values of the block: they must read stable data.  They read tap
            // (0, 0) of the image of the group they pad -- resident for the whole stage -- never the other buffer, which
            // may be receiving the next group's image by DMA at that moment (run-to-run differences in the last bits).
            int off = ((g < G ? g : G - 1) & 1) * a.img_bytes;
            if (g < G && t < T) {
                const int dy = t / sg.kw;
                const int dx = t - dy * sg.kw;
                off += (dy * sg.iw + dx) * 16;
            }
            tap16[(q >> 3) * 8 + (q & 1) * 4 + ((q & 7) >> 1)] = off;             // [stage][half][k-step]
        }
        int pixb[PT];
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) pixb[pt] = ((PT * wave + pt) * sg.iw + r) * 16;

        const size_t plane_px = (size_t)sg.hs * sg.ws;
        // Every group's image has the same per-lane source offsets (only the group's base address differs): they are
        // worked out once per segment, so that inside the stage loop an image piece costs a select and one DMA
        // instruction.  -1: the pixel lies outside the image (or past the halo rows): it is fetched from the zero page.
        constexpr int MAXI = 4;                          // pieces per wave and image: 2 planes x <= 14 KiB over 8 waves
        static_assert(WAVES == 8, "MAXI");
        int img_src[MAXI];
#pragma unroll
        for (int i = 0; i < MAXI; ++i) {
            const int pc = WAVES * i + wave_u;
            const int pl = pc / ppg;
            const int p = (pc - pl * ppg) * 64 + lane;
            const int hy = p / sg.iw;
            const int hx = p - hy * sg.iw;
            const int yy = y0 - sg.pt + hy;
            const int xx = x0 - sg.pl + hx;
            const bool ok = pl < 2 && hy < sg.ih && yy >= 0 && yy < a.h && xx >= 0 && xx < a.w;
            img_src[i] = ok ? (int)(((size_t)pl * plane_px + (size_t)(yy >> sg.upy) * sg.ws + (xx >> sg.up)) * 16) : -1;
        }
        const size_t group_bytes = 2 * plane_px * 16;
        const char* const x_first = sg.x + ((size_t)n * sg.cg_total + sg.g_off) * group_bytes;   // uniform
        // piece i (compile-time) of the image of channel group `chunk` (uniform)
        auto img_piece = [&](int chunk, auto ic) {
            constexpr int i = decltype(ic)::value;
            if ((MPG_DIAG6 & 4) && chunk > 0) return;          // timing only: no image copies in the K loop
            if (i < sg.ni_img) {
                const int off = img_src[i];
                const char* src = (off >= 0 && chunk < sg.cg_seg) ? x_first + (size_t)chunk * group_bytes + off : a.zeros;
                dma16_stream(src, img_lds + (chunk & 1) * a.img_bytes + (WAVES * i + wave_u) * 1024);
            }
        };
        auto w_piece = [&](int stage, auto ic) {
            constexpr int i = decltype(ic)::value;
            const int sidx = stage < NS ? stage : NS - 1;
            if ((MPG_DIAG6 & 8) && stage >= D) return;         // timing only: no weight copies in the K loop
            dma16(sg.w + (size_t)sidx * WSTAGE + tid * 16 + i * (THREADS * 16),
                  w_lds + (stage % R) * WSTAGE + wave_u * 1024 + i * (THREADS * 16));
        };
        static_for<0, MAXI>([&](auto ic) { img_piece(0, ic); });
#pragma unroll
        for (int d = 0; d < D; ++d) static_for<0, NI>([&](auto ic) { w_piece(d, ic); });
        int g_next = 1;                                  // next group image to fetch

        // B fragments of a stage: lane (pixel r of tile row pt, half hh) holds, for k-step j, the 8 channels of slot
        // 2 j + hh: bh[pt][j] is both the fp16 B operand of k-step j and a quarter of the lane's bf6 block.
        half8 bh[PT][4];
        v4i o16n = {0, 0, 0, 0};
        const unsigned i_base = lds_off(img_lds);
        constexpr int AH = MPG_AH, G16 = 4 * NT;
        half8 aq[AH + 1];
        // MID: the reads of the first NPG fp16 groups of `stage` (tap offsets `o`), issued under the last correction step of
        // the stage before: no barrier stands between the two phases, the registers are free (the a_lo codes are made by
        // step NT - 1) and what they read landed in front of the barrier behind which they are issued
        constexpr int NAH = AH < G16 ? AH : G16;     // groups whose reads stand in front of the first group's MFMAs
        // (the 128-register kernel, which keeps the barrier at the stage boundary, would also spill 3 registers for it)
        constexpr int NPG = NT == 1 ? 0 : NAH;
        constexpr int NPRE = kx_cum(NPG, NT, PT);
        auto prefetch_head = [&](int stage, const v4i& o) {
            const unsigned ab = lds_off(w_lds + (stage % R) * WSTAGE) + (unsigned)lane * 16u;
            const int t[4] = {o.x, o.y, o.z, o.w};
            static_for<0, NPG>([&](auto gc) {
                constexpr int g = decltype(gc)::value, j = g / NT;
                if constexpr (g % NT == 0)
                    static_for<0, PT>([&](auto pc) {
                        constexpr int pt = decltype(pc)::value;
                        ds_read16<0>(bh[pt][j], i_base + (unsigned)(pixb[pt] + t[j]));
                    });
                ds_read16<g * 1024>(aq[g % (AH + 1)], ab);
            });
        };
#if MPG_STAMPS
        unsigned long long ts0 = 0, ts1 = 0, ts2 = 0, ts3 = 0, ts3_prev = 0;
        unsigned sum_head = 0, sum_f16 = 0, sum_f6 = 0, sum_bar = 0;
#endif

        // The stage loop.  MID (two to four cout tiles, segments with sg.pref: every image has two stages between its issue
        // and its first slot):
        // the ONE barrier of a stage stands between its fp16 groups and its correction steps,
        //     [first barrier] fp16(0) | corr(0) fp16(1) | corr(1) fp16(2) | ... | corr(NS-1) [drain]
        // so an interval between two barriers pairs the latency- and VALU-bound corrections of one wave of a SIMD with
        // the matrix-dense fp16 groups of its partner, and no operand wait stands directly behind a barrier but the
        // first correction step's, whose operands are in registers by then.  Barrier `|` of stage st:
        //   - every wave has left fp16(st) and corr(st-1): ring slot (st-1) % R and the image buffers that no slot of stage
        //     st or later reads are free.  The weight pieces of stage st + 2 are issued behind it, in corr(st), the image
        //     pieces (if a group is due) behind them in the first fp16 groups of stage st + 1: `vmcnt` issue order of an
        //     interval is [weights][image].
        //   - the wave's own wait in front of it covers what corr(st) and fp16(st+1) read: the weights of stage st + 1
        //     (issued in the interval before) and an image whose first slot lies in stage st + 1; an image first read
        //     later may stay in flight (run-time count), the next barrier's wait covers it with the weights behind it.
        // !MID (tp 8 / 12: an image is first read in the stage after its issue, so it would have to be issued while
        // corr(st-1) of a partner may still read the buffer it replaces): the barrier stands at the stage boundary.
        auto run_stages = [&](auto mc) {
        constexpr bool MID = decltype(mc)::value != 0;
        if constexpr (MID) {
            wait_dma_and_barrier<(D - 1) * NI>();     // image 0, stage 0 and the tap table
            ds_read16<0>(o16n, lds_off(tap16 + hh * 4));
            lgkm_wait<0>();
            tie(o16n);
            prefetch_head(0, o16n);
        }
        for (int st = 0; st < NS; ++st) {
            // !MID: stage st (and everything older, incl. the images issued before it) has landed; all waves are done
            // with stage st-1
            if constexpr (!MID) wait_dma_and_barrier<(D - 1) * NI>();
#if MPG_STAMPS
            if constexpr (!MID) {
                if (st > 0) {       // the barrier's lgkmcnt(0) completed every stamp of the previous stage
                    sum_head += (unsigned)(ts1 - ts0);
                    sum_f16 += (unsigned)(ts2 - ts1);
                    sum_f6 += (unsigned)(ts3 - ts2);
                    if (st > 1) sum_bar += (unsigned)(ts0 - ts3_prev);
                    ts3_prev = ts3;
                }
                MPG_STAMP(ts0);
            }
#endif
            // the tap table is constant over the segment: stage st + 1's entry is read at the head of stage st
            if constexpr (!MID) {
                if (st == 0) {
                    ds_read16<0>(o16n, lds_off(tap16 + hh * 4));
                    lgkm_wait<0>();
                }
            }
            tie(o16n);
            const v4i o16 = o16n;
            const int to16[4] = {o16.x, o16.y, o16.z, o16.w};
            {
                const int sn = st + 1 < NS ? st + 1 : st;
                ds_read16<0>(o16n, lds_off(tap16 + (sn * 2 + hh) * 4));
            }
            // image of group g_next goes into the buffer of group g_next - 2: free once no slot of this or a later
            // stage belongs to that group.  The LDS-DMA pieces of this stage are spread over its MFMA groups (one piece
            // at a time between the MFMAs) instead of being issued as a burst behind the barrier: a burst of WAVES x
            // (NI + image pieces) 1-KiB pieces queues up in the CU's address unit for ~1000-1500 cycles in which no
            // wave issues an MFMA (profiles/r02/kloop_analysis.md).  Order within the stage: the image pieces in the
            // first half of the groups, then the NI weight pieces of stage st + D, so `vmcnt((D-1) NI)` at the next
            // barrier still covers them.
            // MID: the fp16 groups of stage st run in the interval behind the barrier of stage st - 1, which is the one
            // that frees the buffer; the weight pieces go behind the correction MFMAs.
            const int st_free = MID ? st - 1 : st;
            const bool do_img = st_free >= 0 && g_next < G && st_free * 8 >= (g_next - 1) * sg.tp;
            const int img_chunk = g_next;
            // MID: the image stays in flight across this stage's barrier unless the next fp16 groups read it: its first
            // slot g_next * tp lies in stage st + 1 (sg.pref: never earlier)
            const int img_late = (MID && !(MPG_DIAG6 & 4) && do_img && (g_next * sg.tp) / 8 > st + 1) ? sg.ni_img : 0;
            if (do_img) ++g_next;
            const char* wb = w_lds + (st % R) * WSTAGE;
            const unsigned a_base = lds_off(wb) + (unsigned)lane * 16u;
            v8i hi6[PT], lo6[PT];
            int sb[PT], e16[PT];
            // fp16 group g = (k-step g / NT, cout tile g % NT): its reads are [the PT B fragments of the k-step when
            // g % NT == 0] + one A fragment, issued AH groups ahead of its MFMAs
            auto read_group = [&](auto gc) {
                constexpr int g = decltype(gc)::value, j = g / NT;
                if constexpr (g % NT == 0)
                    static_for<0, PT>([&](auto pc) {
                        constexpr int pt = decltype(pc)::value;
                        ds_read16<0>(bh[pt][j], i_base + (unsigned)(pixb[pt] + to16[j]));
                    });
                ds_read16<g * 1024>(aq[g % (AH + 1)], a_base);
            };
            auto make_hi6 = [&](auto pc) {
                constexpr int pt = decltype(pc)::value;
#if MPG_DIAG6 & 2
                const v4i q0 = __builtin_bit_cast(v4i, bh[pt][0]), q1 = __builtin_bit_cast(v4i, bh[pt][1]);
                hi6[pt] = __builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7);
                e16[pt] = 15;
                sb[pt] = 0x7f7f7f7f;
#else
                const half32 b32 = cat32(bh[pt][0], bh[pt][1], bh[pt][2], bh[pt][3]);
                e16[pt] = block_exp16(b32);
                hi6[pt] = bf6_of(b32, e16[pt] + 109);
                sb[pt] = (e16[pt] + 109) | (e16[pt] + 97) << 8;
#endif
            };
            constexpr int HALF = G16 / 2;
            constexpr int IPG = (MAXI + HALF - 1) / HALF;    // image pieces per group (first half of the groups)
            constexpr int WPG = (NI + HALF - 1) / HALF;      // weight pieces per group (second half)
            // bf6 weight planes of the correction steps: step k < NT reads w_lo6[k], step k >= NT w_hi6[k - NT]
            constexpr int KS6 = 2 * NT;                            // correction steps
            constexpr int WD = MPG_WD < KS6 - 1 ? MPG_WD : KS6 - 1;
            constexpr int WPC = (NI + NT - 1) / NT;          // MID: weight pieces per a_lo correction step
            v4i wq[WD + 1][2];
            auto read_w6 = [&](auto kc) {
                constexpr int k = decltype(kc)::value;
                constexpr int off = WF16 + (k < NT ? WF6 + k * 2048 : (k - NT) * 2048);
                ds_read16<off>(wq[k % (WD + 1)][0], a_base);
                ds_read16<off + 1024>(wq[k % (WD + 1)][1], a_base);
            };
            // ---- the fp16 product: G16 groups of PT MFMAs ----
            auto fp16_phase = [&]() {
                // the weight planes of correction step 0 are read in front of the last group: the correction phase starts on
                // operands that are there (MID: the first correction MFMA issues as soon as the barrier releases)
                constexpr bool W0_AHEAD = MPG_W0 != 0;
                static_for<(MID ? NPG : 0), NAH>([&](auto gc) { read_group(gc); });      // MID: the first NPG in prefetch_head
                static_for<0, G16>([&](auto gc) {
                    constexpr int g = decltype(gc)::value, j = g / NT, nt = g % NT;
                    // the LDS-DMA pieces of the group: a wave waits 60-185 cycles per piece for the CU's address unit.  Behind
                    // the group's MFMAs that wait runs under them; in front of the group (rounds 2-3) it delayed the group's
                    // own operand wait -- with one cout tile (three image pieces per group) the head of a stage was 830 cycles
                    auto pieces = [&]() {
                        if constexpr (g < HALF) {
                            if (do_img)
                                static_for<0, IPG>([&](auto kc) {
                                    constexpr int i = g * IPG + decltype(kc)::value;
                                    if constexpr (i < MAXI) img_piece(img_chunk, std::integral_constant<int, i>{});
                                });
                        } else if constexpr (!MID) {
                            static_for<0, WPG>([&](auto kc) {
                                constexpr int i = (g - HALF) * WPG + decltype(kc)::value;
                                if constexpr (i < NI) w_piece(st + D, std::integral_constant<int, i>{});
                            });
                        }
                    };
                    if constexpr (!MPG_PIECES_AFTER) pieces();
                    if constexpr (g + AH < G16) read_group(std::integral_constant<int, g + AH>{});
                    if constexpr (W0_AHEAD && g == G16 - 1) read_w6(std::integral_constant<int, 0>{});
                    // reads issued behind group g's own (MID: the tap-table read stands behind the NPG groups read ahead)
                    lgkm_wait<kx_allowed(g, NT, PT, AH) + (W0_AHEAD && g == G16 - 1 ? 2 : 0) + (MID && g < NPG ? 1 : 0)>();
                    if constexpr (g == 0 && !MID) { MPG_STAMP(ts1); }
                    tie(aq[g % (AH + 1)]);
                    if constexpr (nt == 0)
                        static_for<0, PT>([&](auto pc) { tie(bh[decltype(pc)::value][j]); });
                    static_for<0, PT>([&](auto pc) {
                        constexpr int pt = decltype(pc)::value;
                        acc[pt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq[g % (AH + 1)], bh[pt][j], acc[pt][nt], 0, 0, 0);
                    });
                    if constexpr (MPG_PIECES_AFTER) pieces();
                    // the a_hi block scales and codes (VALU work under the matrix pipe): tile row g - 3 NT behind each group
                    // of the last k-step, whatever is left behind the last group
                    if constexpr (g >= 3 * NT && g - 3 * NT < PT) make_hi6(std::integral_constant<int, g - 3 * NT>{});
                    if constexpr (g == G16 - 1 && NT < PT) static_for<NT, PT>([&](auto pc) { make_hi6(pc); });
                });
            };
            // ---- the two bf6 corrections: step k < NT is w_lo6[k] x a_hi6, step k >= NT is w_hi6[k - NT] x a_lo6 ----
            // LDS reads in order: W(0), the a_lo fragments (into the registers of the a_hi ones, which the conversions
            // above have consumed), W(1) .. W(WD), then W(k + WD) ahead of step k.
            auto bf6_phase = [&](auto w0c) {
            constexpr bool W0_DONE = decltype(w0c)::value != 0;    // W(0) was read in front of the last fp16 group
#if !(MPG_DIAG6 & 1)
            constexpr int PB = PT;                                 // all a_lo fragments at once: they land in the a_hi registers
            auto read_bl = [&](auto pc) {
                constexpr int pt = decltype(pc)::value;
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    ds_read16<0>(bh[pt][j], i_base + (unsigned)(plane_b + pixb[pt] + to16[j]));
                });
            };
            auto make_lo6 = [&](auto pc) {
                constexpr int pt = decltype(pc)::value;
                static_for<0, 4>([&](auto jc) { tie(bh[pt][decltype(jc)::value]); });
#if MPG_DIAG6 & 2
                const v4i q0 = __builtin_bit_cast(v4i, bh[pt][0]), q1 = __builtin_bit_cast(v4i, bh[pt][1]);
                lo6[pt] = __builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7);
#else
                lo6[pt] = bf6_of(cat32(bh[pt][0], bh[pt][1], bh[pt][2], bh[pt][3]), e16[pt] + 97);
#endif
            };
            if constexpr (!W0_DONE) read_w6(std::integral_constant<int, 0>{});
            static_for<0, PB>([&](auto pc) { read_bl(pc); });
            static_for<1, WD + 1>([&](auto kc) { read_w6(kc); });
            static_for<0, KS6>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                if constexpr (k >= 1 && k + WD < KS6) read_w6(std::integral_constant<int, k + WD>{});
                // reads issued behind W(k): at k = 0 the a_lo fragments and W(1 .. WD), later W(k + 1 .. k + WD)
                constexpr int ahead = (k + WD < KS6 ? k + WD : KS6 - 1) - k;
                // MID: behind the last W read, in front of the last step's wait, the head of the next stage's fp16 groups
                constexpr int pre = (MID && k == KS6 - 1) ? NPRE : 0;
                if constexpr (pre != 0) {
                    tie(o16n);
                    prefetch_head(st + 1, o16n);
                }
                lgkm_wait<(k == 0 ? 4 * PB : 0) + 2 * ahead + pre>();
                if constexpr (k == 0 && MID) { MPG_STAMP(ts1); }
                tie(wq[k % (WD + 1)][0]);
                tie(wq[k % (WD + 1)][1]);
                const v8i w6 = __builtin_shufflevector(wq[k % (WD + 1)][0], wq[k % (WD + 1)][1], 0, 1, 2, 3, 4, 5, 6, 7);
                static_for<0, PT>([&](auto pc) {
                    constexpr int pt = decltype(pc)::value;
                    if constexpr (k < NT)
                        acc[pt][k] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w6, hi6[pt], acc[pt][k], BF6, BF6, 1, w6[6], 0, sb[pt]);
                    else
                        acc[pt][k - NT] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w6, lo6[pt], acc[pt][k - NT], BF6, BF6, 0, w6[6], 1, sb[pt]);
                });
                // the a_lo codes of tile row pt (VALU: block maximum, scale, 32-value conversion) behind the MFMAs of the a_hi
                // step lo_step(pt), as late as still finishes in front of the first a_lo step NT: the conversions of the
                // rows run under the matrix work of different steps instead of in one piece in front of step 1
                if constexpr (k < NT) {
                    if constexpr (k == 0 && lo_step(0, NT, PT) == 0) lgkm_wait<2 * ahead>();     // the a_lo fragments are there
                    static_for<0, PT>([&](auto pc) {
                        if constexpr (lo_step(decltype(pc)::value, NT, PT) == k) make_lo6(pc);
                    });
                } else if constexpr (MID) {
                    // the weight pieces of stage st + D, one at a time behind the MFMAs of the a_lo steps, whose gaps carry
                    // no conversion work: the slot they overwrite was last read in corr(st - 1), which every wave left
                    // before this stage's barrier
                    static_for<0, WPC>([&](auto ic) {
                        constexpr int i = (k - NT) * WPC + decltype(ic)::value;
                        if constexpr (i < NI) w_piece(st + D, std::integral_constant<int, i>{});
                    });
                }
            });
#else
            if constexpr (MID) static_for<0, NI>([&](auto ic) { w_piece(st + D, ic); });
            // (named first: an asm operand alone does not capture a variable of the enclosing lambda)
            const v8i& h0 = hi6[0];
            const int &s0 = sb[0], &e0 = e16[0];
            asm volatile("" ::"v"(h0), "v"(s0), "v"(e0));
#endif
            };
            fp16_phase();
            MPG_STAMP(ts2);
            if constexpr (MID) {
                // the weights of stage st + 1 (the newest pieces but for an image issued in the groups above) have landed
                wait_dma_late_and_barrier(img_late);
#if MPG_STAMPS
                // (the barrier's lgkmcnt(0) completed every stamp in front of it) the interval behind the barrier of stage
                // st - 1: head ts0 .. ts1, correction steps .. ts3, fp16 groups .. ts2, wait for this barrier .. new ts0
                if (st > 0) {
                    sum_head += (unsigned)(ts1 - ts0);
                    sum_f6 += (unsigned)(ts3 - ts1);
                    sum_f16 += (unsigned)(ts2 - ts3);
                    if (st > 1) sum_bar += (unsigned)(ts0 - ts3_prev);
                    ts3_prev = ts2;
                }
                MPG_STAMP(ts0);
#endif
            }
            bf6_phase(std::integral_constant<int, MPG_W0>{});
            MPG_STAMP(ts3);
        }
        };
        // one loop per barrier position, chosen once per segment (a branch inside the stage body would merge the two
        // register allocations at every stage: 390 spilled registers when tried)
        // (two `if`s in a row, the second on a value the compiler cannot tell from the first, like the direct path above: as
        // the two arms of ONE branch the loops spill 130 to 830 registers)
        // The one-cout-tile kernel keeps the barrier at the stage boundary for every segment: with four waves per SIMD its
        // phases already run beside three other waves', and measured with the barrier in mid-stage b2.A took 217.9 us
        // against 213.9 and b2.B 92.5 against 89.6 (profiles/r14/bench_c2_per_layer.txt, kloop_stamps_barrier.txt).
        if constexpr (NT == 1) {
            run_stages(std::integral_constant<int, 0>{});
        } else {
            int mid = __builtin_amdgcn_readfirstlane(sg.pref);
            if (mid) run_stages(std::integral_constant<int, 1>{});
            asm volatile("" : "+s"(mid));
            if (!mid) run_stages(std::integral_constant<int, 0>{});
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
#if MPG_STAMPS
        if ((a.dbg & 8) && a.y != nullptr && s == 0 && lane == 0) {
            unsigned* o = reinterpret_cast<unsigned*>(a.y) + ((size_t)blockIdx.x * WAVES + wave) * 4;
            o[0] = sum_head; o[1] = sum_f16; o[2] = sum_f6; o[3] = sum_bar;
        }
#endif
    }
    conv_epilogue<NT, PT>(acc, ap, smem, n, y0, x0, wave, lane, pre);
}

}  // namespace

hipError_t mpg::conv::launch_conv_f6(int nt, dim3 grid, size_t lds, hipStream_t st, const ConvArgs& a) {
    switch (nt) {
        case 1: return mpg::launch_dyn_lds<conv_mfma_f6_kernel<1>>(grid, dim3(Pipe6<1>::WAVES * 64), lds, st, a);
        case 2: return mpg::launch_dyn_lds<conv_mfma_f6_kernel<2>>(grid, dim3(Pipe6<2>::WAVES * 64), lds, st, a);
        case 3: return mpg::launch_dyn_lds<conv_mfma_f6_kernel<3>>(grid, dim3(Pipe6<3>::WAVES * 64), lds, st, a);
        default: return mpg::launch_dyn_lds<conv_mfma_f6_kernel<4>>(grid, dim3(Pipe6<4>::WAVES * 64), lds, st, a);
    }
}
