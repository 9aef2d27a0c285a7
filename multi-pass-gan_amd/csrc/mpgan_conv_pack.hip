// Weight images of the fused convolution: HWIO fp32 -> what each kernel family's K loop reads (mpgan_conv.h).
#include "mpgan_conv.h"

using namespace mpg::conv;

namespace {

// e3m2 code (sign, 3 exponent bits, bias 3, 2 mantissa bits; no infinities) of x, round to nearest even, saturating at 28
__device__ __forceinline__ int e3m2_encode(float x) {
    const int s = (__builtin_bit_cast(unsigned, x) >> 31) << 5;
    const float ax = fabsf(x);
    if (!(ax < 28.f)) return s | 31;
    const int e = ax >= 0.25f ? ilogbf(ax) : -2;          // the binade whose step is used; subnormals share the step of [0.25, 0.5)
    const float step = ldexpf(1.f, e - 2);
    const float v = rintf(ax / step) * step;              // may reach the next binade
    if (v == 0.f) return s;
    const int e2 = ilogbf(v);
    if (e2 < -2) return s | (int)(v * 16.f);             // subnormal: M * 2^-4
    return s | (e2 + 3) << 2 | (int)((v * ldexpf(1.f, -e2) - 1.f) * 4.f);
}

// F16F6 weight image: per stage (8 consecutive tap slots of the segment's slot stream; fold: 8 channel groups):
//   [4 k-steps][NT][64 lanes][8 x fp16]  |  w_hi6: [NT][2 halves][64 lanes][16 B]  |  w_lo6: same
// Lane (row r of cout tile nt, half hh) holds the 32 values (k-step j, element e) -> slot 2 j + hh, channel e: the fp16 A
// fragments of the four k-steps AND, in that order, the K block of 32 of the bf6 instruction.  A bf6 plane keeps the
// lane's 32 six-bit codes (value i at bits 6 i .. 6 i + 5 of 24 bytes) in bytes 0-15 of half 0 and 0-7 of half 1; bytes
// 8-11 of half 1 are the scale word {E8M0 of the w_hi block, E8M0 of the w_lo block, 0, 0} (in both planes), 12-15 zero.
// Block scale: 2^(floor(log2 max|v|) - 3), i.e. the largest code magnitude lies in [8, 16).
__global__ void pack_weights_f6_kernel(const float* __restrict__ w, int kh, int kw, int cin_total, int c_off,
                                       int cin, int cout, float wscale, const float* __restrict__ cscale,
                                       int NT, int sc, int fold, int tp, char* __restrict__ out) {
    // fold (direct 1x1 segments): the "taps" of a macro-step are 8 consecutive channel groups
    const int T = kh * kw;
    const long total = (long)sc * NT * 64;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int lane = idx & 63;
    const int nt = (idx >> 6) % NT;
    const int st = (int)((idx >> 6) / NT);
    const int r = lane & 31, hh = lane >> 5;
    const int co = nt * 32 + r;
    char* base = out + (size_t)st * 8 * NT * 1024;
    auto weight = [&](int slot, int j) -> float {
        // slot within the stream: fold: channel group `slot`; else group slot / tp, tap slot % tp
        int tap, chn;
        if (fold) { tap = 0; chn = slot * 8 + j; }
        else { const int g = slot / tp; tap = slot - g * tp; chn = g * 8 + j; }
        if (tap >= T || chn >= cin || co >= cout) return 0.f;
        float v = w[((size_t)tap * cin_total + c_off + chn) * cout + co] * wscale;
        if (cscale != nullptr) v *= cscale[co];
        return v;
    };
    float v[32], lo[32];
    float mh = 0.f, ml = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        v[i] = weight(st * 8 + 2 * (i >> 3) + hh, i & 7);
        const _Float16 h = (_Float16)v[i];
        lo[i] = v[i] - (float)h;
        mh = fmaxf(mh, fabsf(v[i]));
        ml = fmaxf(ml, fabsf(lo[i]));
        reinterpret_cast<_Float16*>(base)[((size_t)((i >> 3) * NT + nt) * 64 + lane) * 8 + (i & 7)] = h;
    }
    int eh = mh > 0.f ? ilogbf(mh) - 3 : 0, el = ml > 0.f ? ilogbf(ml) - 3 : 0;
    eh = eh < -126 ? -126 : eh > 120 ? 120 : eh;
    el = el < -126 ? -126 : el > 120 ? 120 : el;
    const int scale_word = (eh + 127) | (el + 127) << 8;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        unsigned d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const float inv = ldexpf(1.f, -(pl ? el : eh));
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const unsigned long long c = (unsigned long long)e3m2_encode((pl ? lo[i] : v[i]) * inv) << ((6 * i) & 31);
            d[(6 * i) >> 5] |= (unsigned)c;
            if (((6 * i) >> 5) + 1 < 6) d[((6 * i) >> 5) + 1] |= (unsigned)(c >> 32);
        }
        d[6] = (unsigned)scale_word;
        char* p6 = base + 4 * NT * 1024 + (size_t)pl * NT * 2048 + (size_t)nt * 2048 + (size_t)lane * 16;
        *reinterpret_cast<uint4*>(p6) = make_uint4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<uint4*>(p6 + 1024) = make_uint4(d[4], d[5], d[6], d[7]);
    }
}

// weights HWIO fp32 -> per (chunk, stage) fragment-ordered fp16 hi [lo] planes
__global__ void pack_weights_kernel(const float* __restrict__ w, int kh, int kw, int cin_total, int c_off,
                                    int cin, int cout, float wscale, const float* __restrict__ cscale,
                                    int NT, int KS, int NPL, int cgc, int nchunks, int sc,
                                    _Float16* __restrict__ out) {
    const long total = (long)nchunks * sc * KS * NT * 512;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int j = idx & 7;
    const int lane = (idx >> 3) & 63;
    long rest = idx >> 9;
    const int nt = rest % NT; rest /= NT;
    const int ks = rest % KS; rest /= KS;
    const int st = rest % sc;
    const int c = rest / sc;
    const int r = lane & 31, hh = lane >> 5;
    const int q = 2 * (st * KS + ks) + hh;
    float v = 0.f;
    if (q < kh * kw * cgc) {
        const int tap = q / cgc;
        const int gg = q - tap * cgc;
        const int chn = (c * cgc + gg) * 8 + j;
        const int co = nt * 32 + r;
        if (chn < cin && co < cout) {
            v = w[((size_t)tap * cin_total + c_off + chn) * cout + co] * wscale;
            if (cscale != nullptr) v *= cscale[co];
        }
    }
    const long plane = (long)KS * NT * 512;
    const long stage = (long)c * sc + st;
    const long off = ((long)(ks * NT + nt) * 64 + lane) * 8 + j;
    const _Float16 hi = (_Float16)v;
    out[stage * plane * NPL + off] = hi;
    if (NPL == 2) out[stage * plane * NPL + plane + off] = (_Float16)(v - (float)hi);
}

// fp32 table [tap][ci 8][co 8] of a small layer (zero padded), scaled like the MFMA pack
__global__ void pack_small_kernel(const float* __restrict__ w, int taps, int cin_total, int c_off, int cin, int cout,
                                  float wscale, const float* __restrict__ cscale, float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= taps * 64) return;
    const int co = idx & 7, ci = (idx >> 3) & 7, tap = idx >> 6;
    float v = 0.f;
    if (ci < cin && co < cout) {
        v = w[((size_t)tap * cin_total + c_off + ci) * cout + co] * wscale;
        if (cscale != nullptr) v *= cscale[co];
    }
    out[idx] = v;
}

}  // namespace

extern "C" size_t mpg_conv_pack_size(int kh, int kw, int cin, int cout, int prec) {
    const size_t base = pack_base_bytes(kh, kw, cin, cout, prec);
    if (base == 0) return 0;
    return base + (small_layer(cin, cout) ? (size_t)kh * kw * 64 * sizeof(float) : 0);
}

extern "C" int mpg_conv_pack_weights(mpg_stream_t stream, const float* w_hwio, int kh, int kw, int w_cin_total,
                                     int w_c_off, int cin, int cout, float wscale, const float* cout_scale, int prec,
                                     void* out, size_t out_bytes) {
    MPG_REQUIRE(w_hwio && out, "mpg_conv_pack_weights: null pointer");
    MPG_REQUIRE(prec == MPG_PREC_F16X1 || prec == MPG_PREC_F16X3 || prec == MPG_PREC_F16F6,
                "mpg_conv_pack_weights: bad prec %d", prec);
    MPG_REQUIRE(kh >= 1 && kh <= 7 && kw >= 1 && kw <= 7, "mpg_conv_pack_weights: kernel %dx%d unsupported", kh, kw);
    MPG_REQUIRE(cin >= 1 && w_c_off >= 0 && w_c_off + cin <= w_cin_total, "mpg_conv_pack_weights: channel range");
    MPG_REQUIRE(cout >= 1 && cout <= 128, "mpg_conv_pack_weights: cout %d not in 1..128", cout);
    const size_t need = mpg_conv_pack_size(kh, kw, cin, cout, prec);
    MPG_REQUIRE(need > 0, "mpg_conv_pack_weights: %dx%d %d->%d not available at prec %d", kh, kw, cin, cout, prec);
    MPG_REQUIRE(out_bytes >= need, "mpg_conv_pack_weights: out buffer %zu < %zu", out_bytes, need);
    const int nt = (cout + 31) / 32;
    const SegShape ss = seg_shape(kh, kw, cin, nt, prec);
    if (prec == MPG_PREC_F16F6) {
        const long total = (long)ss.sc * nt * 64;
        hipLaunchKernelGGL(pack_weights_f6_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                           w_hwio, kh, kw, w_cin_total, w_c_off, cin, cout, wscale, cout_scale, nt, ss.sc, ss.direct, ss.tp,
                           (char*)out);
    } else {
        const int ks = pipe_shape(nt, prec).ks;
        const int npl = prec == MPG_PREC_F16X3 ? 2 : 1;
        const long total = (long)ss.stages * ks * nt * 512;
        hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           w_hwio, kh, kw, w_cin_total, w_c_off, cin, cout, wscale, cout_scale, nt, ks, npl, ss.cgc,
                           ss.nchunks, ss.sc, (_Float16*)out);
    }
    if (small_layer(cin, cout))
        hipLaunchKernelGGL(pack_small_kernel, dim3((kh * kw * 64 + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_hwio,
                           kh * kw, w_cin_total, w_c_off, cin, cout, wscale, cout_scale,
                           (float*)((char*)out + pack_base_bytes(kh, kw, cin, cout, prec)));
    MPG_LAUNCH_CHECK(prec == MPG_PREC_F16F6 ? "pack_weights_f6_kernel" : "pack_weights_kernel");
}
