// Host side of the fused convolution (mpgan_conv.h): how a launch is cut into segments, chunks and weight stages, its LDS
// plan, and the three entry points.  No kernels here: they live in mpgan_conv_f16.hip, mpgan_conv_f6.hip and
// mpgan_conv_small.hip, each behind its launch function.
#include "mpgan_conv.h"

using namespace mpg::conv;

namespace {

template <class P>
constexpr Shape shape_of() {
    return {P::TH, P::KS, P::WAVES, P::WSTAGE, P::R * P::WSTAGE, P::ROWF};
}
constexpr Shape SHAPES[3][4] = {   // [prec - 1][nt - 1]: the instantiations launch_conv_f16() / launch_conv_f6() pick from
    {shape_of<Pipe<1, 1>>(), shape_of<Pipe<2, 1>>(), shape_of<Pipe<3, 1>>(), shape_of<Pipe<4, 1>>()},
    {shape_of<Pipe6<1>>(), shape_of<Pipe6<2>>(), shape_of<Pipe6<3>>(), shape_of<Pipe6<4>>()},
    {shape_of<Pipe<1, 3>>(), shape_of<Pipe<2, 3>>(), shape_of<Pipe<3, 3>>(), shape_of<Pipe<4, 3>>()},
};
static_assert(MPG_PREC_F16X1 == 1 && MPG_PREC_F16F6 == 2 && MPG_PREC_F16X3 == 3, "SHAPES is indexed by prec - 1");

// LDS of a launch.  K loop: [tap-offset table][two halo images][weight ring]; conv_epilogue reuses it as
// [TAPOFF_BYTES][32 staging rows per wave].  A launch asks for the larger of the two.
constexpr size_t LDS_TWO_WG = 80 * 1024;   // what leaves room for a second workgroup on the CU
struct LdsPlan {
    size_t tap, loop, epi, total;
};
LdsPlan lds_plan(int tap_slots, int img_bytes, const Shape& ps) {
    LdsPlan l;
    // one int per tap slot in 1 KiB granules, at least the TAPOFF_BYTES the epilogue skips
    l.tap = ((size_t)tap_slots * 4 + 1023) / 1024 * 1024;
    if (l.tap < (size_t)TAPOFF_BYTES) l.tap = TAPOFF_BYTES;
    l.loop = l.tap + 2 * (size_t)img_bytes + ps.ring;
    l.epi = TAPOFF_BYTES + (size_t)ps.waves * 32 * ps.rowf * sizeof(float);
    l.total = l.loop > l.epi ? l.loop : l.epi;
    return l;
}

// the LDS halo image of a chunk of cgc channel groups: [group][plane][np pixels][16 B], copied in 1 KiB pieces, ni_img
// per wave
void set_image(SegShape& s, const Shape& ps, int kh, int kw, int cgc) {
    s.cgc = cgc;
    s.np = ((ps.th + kh - 1) * (TW + kw - 1) + 63) & ~63;
    s.ni_img = (cgc * 2 * (s.np / 64) + ps.waves - 1) / ps.waves;
    s.img_bytes = s.ni_img * ps.waves * 1024;
}

// MPG_PREC_F16F6 (conv_mfma_f6_kernel): nchunks = channel groups (one LDS halo image each), sc = weight stages of the
// whole segment
SegShape seg_shape_f6(int kh, int kw, int cin, int nt) {
    const Shape& ps = pipe_shape(nt, MPG_PREC_F16F6);
    const int stage_slots = 2 * ps.ks;
    SegShape s = {};
    if (kh == 1 && kw == 1 && cin > 8 && nt <= 2) {   // the kernel's direct path: K over channel groups, no image, no table
        s.direct = 1; s.cgc = 1;
        s.nchunks = 1;
        s.stages = s.sc = ((cin + 7) / 8 + stage_slots - 1) / stage_slots;
        return s;
    }
    set_image(s, ps, kh, kw, 1);
    s.nchunks = (cin + 7) / 8;
    // tap slots per group: the taps themselves when a group spans >= 2 stages; below that padded to 8, 12 or 16 so
    // that the image of group g+1 (issued once no stage touches group g-1) has >= 1 stage of flight before its
    // first slot: floor(tp (g+1) / 8) - ceil(tp g / 8) >= 1 for every g
    const int T = kh * kw;
    s.tp = T >= 16 ? T : T <= 8 ? 8 : T <= 12 ? 12 : 16;
    s.stages = s.sc = (s.nchunks * s.tp + stage_slots - 1) / stage_slots;
    s.slots = s.sc * stage_slots;
    // The image of group g is issued in stage ceil((g - 1) tp / 8) (the first stage that no longer touches group g - 2)
    // and its first slot lies in stage floor(g tp / 8).  The kernel may read stage st + 1's B fragments during stage st
    // only if every image is then already behind a barrier that followed its DMA wait: two stages between issue and
    // first use, for every group.
    s.pref = 1;
    for (int g = 1; g < s.nchunks; ++g)
        if ((g * s.tp) / stage_slots - ((g - 1) * s.tp + stage_slots - 1) / stage_slots < 2) s.pref = 0;
    return s;
}

// the depth-to-space output of mpg_conv2d_fused_d2s (block size 2)
struct D2SOut {
    int cs, coff;
};

// the channel window [co_off, co_off + cout) of c_total-channel outputs (mpg_conv2d_fused_window); mpg_conv2d_fused is
// the window {cout, 0}
struct WinOut {
    int c_total, co_off;
};

}  // namespace

const Shape& mpg::conv::pipe_shape(int nt, int prec) { return SHAPES[prec - 1][nt - 1]; }

// The K decomposition of one segment at `prec`.  MPG_PREC_F16X1 / F16X3 (conv_mfma_kernel): nchunks chunks of cgc
// channel groups, sc weight stages per chunk; two groups per chunk when that removes the half-empty k-step of an odd tap
// count and the double-buffered images still leave room for two workgroups per CU
SegShape mpg::conv::seg_shape(int kh, int kw, int cin, int nt, int prec) {
    if (prec == MPG_PREC_F16F6) return seg_shape_f6(kh, kw, cin, nt);
    const Shape& ps = pipe_shape(nt, prec);
    const int cg = (cin + 7) / 8;
    SegShape s = {};
    set_image(s, ps, kh, kw, 2);
    if (cg < 2 || !((kh * kw) & 1) || lds_plan(0, s.img_bytes, ps).loop > LDS_TWO_WG) set_image(s, ps, kh, kw, 1);
    s.nchunks = (cg + s.cgc - 1) / s.cgc;
    const int ksteps = (kh * kw * s.cgc + 1) / 2;
    s.sc = (ksteps + ps.ks - 1) / ps.ks;
    s.slots = s.sc * ps.ks * 2;
    s.stages = s.nchunks * s.sc;
    return s;
}

size_t mpg::conv::pack_base_bytes(int kh, int kw, int cin, int cout, int prec) {
    if (kh < 1 || kw < 1 || kh > 7 || kw > 7 || cin < 1 || cout < 1 || cout > 128) return 0;
    if (prec != MPG_PREC_F16X1 && prec != MPG_PREC_F16F6 && prec != MPG_PREC_F16X3) return 0;
    const int nt = (cout + 31) / 32;
    const SegShape ss = seg_shape(kh, kw, cin, nt, prec);
    // a segment whose tables + two images + ring cannot fit the LDS is "not available at this precision" (callers then
    // pack for MPG_PREC_F16X3), e.g. 7x7 with four cout tiles at MPG_PREC_F16F6
    if (lds_plan(ss.slots, ss.img_bytes, pipe_shape(nt, prec)).total > LDS_MAX) return 0;
    return (size_t)ss.stages * pipe_shape(nt, prec).wstage;
}

int mpg::conv::check_segment(const mpg_conv_desc* d, int s) {
    const mpg_conv_seg& g = d->seg[s];
    MPG_REQUIRE(g.x && g.wpack, "mpg_conv2d_fused: segment %d null pointer", s);
    MPG_REQUIRE(g.kh >= 1 && g.kh <= 7 && g.kw >= 1 && g.kw <= 7, "mpg_conv2d_fused: segment %d kernel %dx%d", s, g.kh, g.kw);
    MPG_REQUIRE(g.cin >= 1 && g.g_off >= 0 && g.g_off + (g.cin + 7) / 8 <= g.cgroups,
                "mpg_conv2d_fused: segment %d channel-group range", s);
    MPG_REQUIRE(g.up_log2 >= 0 && g.up_log2 <= 4, "mpg_conv2d_fused: segment %d up_log2 %d", s, g.up_log2);
    MPG_REQUIRE(g.up_x_only == 0 || g.up_x_only == 1, "mpg_conv2d_fused: segment %d up_x_only %d (0 or 1)", s, g.up_x_only);
    // a column-only upsample leaves the rows alone: only w has to divide
    MPG_REQUIRE((g.up_x_only || (d->h % (1 << g.up_log2)) == 0) && (d->w % (1 << g.up_log2)) == 0,
                "mpg_conv2d_fused: segment %d: %dx%d not divisible by upsample %d", s, d->h, d->w, 1 << g.up_log2);
    MPG_REQUIRE((((uintptr_t)g.x) & 15) == 0 && (((uintptr_t)g.wpack) & 15) == 0, "mpg_conv2d_fused: segment %d misaligned", s);
    return MPG_OK;
}

// conv_mfma_kernel / conv_mfma_f6_kernel; d2s: the depth-to-space store of mpg_conv2d_fused_d2s; win: where the outputs
// lie in their tensors
static int launch_mfma(hipStream_t stream, const mpg_conv_desc* d, const D2SOut* d2s, const WinOut& win) {
    const int nt = (d->cout + 31) / 32;
    const Shape& ps = pipe_shape(nt, d->prec);
    ConvArgs a;
    a.n = d->n; a.h = d->h; a.w = d->w; a.cout = d->cout; a.nseg = d->nseg;
    int max_img = 0, max_slots = 0;
    for (int s = 0; s < d->nseg; ++s) {
        if (const int rc = check_segment(d, s)) return rc;
        const mpg_conv_seg& g = d->seg[s];
        const SegShape ss = seg_shape(g.kh, g.kw, g.cin, nt, d->prec);
        // conv_mfma_kernel's table is the fixed TAPOFF_BYTES; conv_mfma_f6_kernel's grows with the launch (tap_bytes)
        MPG_REQUIRE(d->prec == MPG_PREC_F16F6 || ss.slots <= TAPOFF_BYTES / 4, "mpg_conv2d_fused: segment %d tap table too large", s);
        SegArgs& o = a.seg[s];
        o.x = (const char*)g.x; o.w = (const char*)g.wpack;
        o.cg_seg = (g.cin + 7) / 8; o.cg_total = g.cgroups; o.g_off = g.g_off;
        o.kh = g.kh; o.kw = g.kw; o.up = g.up_log2; o.upy = g.up_x_only ? 0 : g.up_log2;
        o.cgc = ss.cgc; o.nchunks = ss.nchunks; o.sc = ss.sc;
        o.ih = ps.th + g.kh - 1; o.iw = TW + g.kw - 1;
        o.pt = pad_before(g.kh, g.pad_hi); o.pl = pad_before(g.kw, g.pad_hi);
        o.hs = d->h >> o.upy; o.ws = d->w >> o.up;
        o.np = ss.np; o.ni_img = ss.ni_img;
        o.direct = ss.direct;
        o.tp = ss.tp;
        MPG_REQUIRE(!ss.direct || (size_t)o.hs * o.ws * 16 * 16 < ((size_t)1 << 31),
                    "mpg_conv2d_fused: segment %d: %dx%d too large for the 1x1 path (32-bit group offsets)", s, d->h, d->w);
        o.pref = ss.pref;
        max_img = ss.img_bytes > max_img ? ss.img_bytes : max_img;
        max_slots = ss.slots > max_slots ? ss.slots : max_slots;
    }
    for (int s = d->nseg; s < MPG_MAX_SEG; ++s) a.seg[s] = a.seg[0];
    a.bias = d->bias; a.in_amax = d->in_amax; a.act = d->act; a.leak = d->leak; a.pn = d->pixel_norm; a.pn_eps = d->pn_eps;
    a.post_add = d->post_add; a.pa_stride = d->post_add_stride; a.pa_coff = d->post_add_coff;
    MPG_REQUIRE(!d->post_add || d->post_add_coff + d->cout <= d->post_add_stride, "mpg_conv2d_fused: post_add channel range");
    // the window's first channel goes into the two pointers; the kernels keep the strides of the whole tensors
    a.y_stride = win.c_total;
    a.cg_img = (win.c_total + 7) / 8;
    a.y = d->y != nullptr ? d->y + win.co_off : nullptr;
    a.y_g8 = d->y_g8 != nullptr ? (char*)d->y_g8 + (size_t)(win.co_off / 8) * 2 * d->h * d->w * 16 : nullptr;
    MPG_REQUIRE((((uintptr_t)d->y) & 15) == 0 && (((uintptr_t)d->y_g8) & 15) == 0,
                "mpg_conv2d_fused: misaligned output");
    a.zeros = mpg::zero_page();
    MPG_REQUIRE(a.zeros != nullptr, "mpg_conv2d_fused: could not allocate the zero page");
    a.img_bytes = max_img;
    a.tiles_x = (d->w + TW - 1) / TW;
    a.tiles_y = (d->h + ps.th - 1) / ps.th;
    a.dbg = d->reserved;
    const long nblk = (long)d->n * a.tiles_x * a.tiles_y;
    MPG_REQUIRE(nblk < (1L << 31), "mpg_conv2d_fused: grid too large");
    const LdsPlan lds = lds_plan(max_slots, max_img, ps);
    a.tap_bytes = (int)lds.tap;
    MPG_REQUIRE(lds.total <= LDS_MAX, "mpg_conv2d_fused: LDS budget %zu exceeds 160 KiB", lds.total);
    const dim3 grid((unsigned)nblk);
    hipError_t le;
    if (d2s != nullptr) {
        ConvArgsD2S ad;
        ad.a = a;
        ad.cs = d2s->cs;
        ad.coff = d2s->coff;
        ad.cg = d2s->cs / 8;
        le = launch_conv_f16(d->prec, nt, grid, lds.total, stream, ad);
    } else if (d->prec == MPG_PREC_F16F6) {
        le = launch_conv_f6(nt, grid, lds.total, stream, a);
    } else {
        le = launch_conv_f16(d->prec, nt, grid, lds.total, stream, a);
    }
    if (le != hipSuccess) return mpg::hip_check(le, "mpg_conv2d_fused: hipFuncSetAttribute(dynamic LDS)");
    MPG_LAUNCH_CHECK("conv_mfma_kernel");
}

static int conv2d_fused(mpg_stream_t stream, const mpg_conv_desc* d, const D2SOut* d2s, const WinOut* window = nullptr) {
    MPG_REQUIRE(d != nullptr, "mpg_conv2d_fused: null desc");
    MPG_REQUIRE(d->n >= 1 && d->h >= 1 && d->w >= 1, "mpg_conv2d_fused: bad shape %d x %d x %d", d->n, d->h, d->w);
    MPG_REQUIRE(d->cout >= 1 && d->cout <= 128, "mpg_conv2d_fused: cout %d not in 1..128", d->cout);
    MPG_REQUIRE(d->nseg >= 1 && d->nseg <= MPG_MAX_SEG, "mpg_conv2d_fused: nseg %d", d->nseg);
    MPG_REQUIRE(d->y != nullptr || d->y_g8 != nullptr, "mpg_conv2d_fused: no output requested");
    MPG_REQUIRE(d->prec == MPG_PREC_F16X1 || d->prec == MPG_PREC_F16X3 || d->prec == MPG_PREC_F16F6,
                "mpg_conv2d_fused: bad prec %d", d->prec);
    MPG_REQUIRE(d->act >= MPG_ACT_NONE && d->act <= MPG_ACT_TANH, "mpg_conv2d_fused: bad act %d", d->act);
    // (the depth-to-space store is an epilogue of the MFMA kernels only: such a launch stays on them)
    // (a window store likewise: conv_small_kernel writes whole tensors, and callers cut wide layers so that no window is
    // that narrow, ops.wide_chunks)
    bool small = d->cout <= 8 && !d->pixel_norm && d->post_add == nullptr && d->reserved == 0 && d2s == nullptr && window == nullptr;
    for (int s = 0; s < d->nseg && small; ++s) small = d->seg[s].cin <= 8;
    const WinOut whole = {d->cout, 0};
    return small ? launch_small((hipStream_t)stream, d) : launch_mfma((hipStream_t)stream, d, d2s, window != nullptr ? *window : whole);
}

extern "C" int mpg_conv2d_fused(mpg_stream_t stream, const mpg_conv_desc* d) {
    return conv2d_fused(stream, d, nullptr);
}

extern "C" int mpg_conv2d_fused_d2s(mpg_stream_t stream, const mpg_conv_desc* d, int r, int c_total, int co_off) {
    MPG_REQUIRE(d != nullptr, "mpg_conv2d_fused_d2s: null desc");
    MPG_REQUIRE(r == 2, "mpg_conv2d_fused_d2s: block size %d (only 2)", r);
    MPG_REQUIRE(c_total >= 4 && c_total % 4 == 0, "mpg_conv2d_fused_d2s: %d channels are not a multiple of 4", c_total);
    MPG_REQUIRE(co_off >= 0 && d->cout >= 1 && co_off + d->cout <= c_total,
                "mpg_conv2d_fused_d2s: channels [%d, %d) outside 0..%d", co_off, co_off + d->cout, c_total);
    MPG_REQUIRE(!d->pixel_norm && d->post_add == nullptr, "mpg_conv2d_fused_d2s: no pixel norm or post-add");
    // the F16F6 kernel has no depth-to-space store (the shuffle's 1x1 contraction, K = C <= 256, runs as MPG_PREC_F16X3
    // under the planner's rule anyway)
    if (d->prec == MPG_PREC_F16F6) {
        mpg::set_error("mpg_conv2d_fused_d2s: MPG_PREC_F16F6 has no depth-to-space store (use MPG_PREC_F16X3 / F16X1)");
        return MPG_ERR_UNSUPPORTED;
    }
    const int cs = c_total / 4;
    // a G8 group of 8 channels must stay inside one parity of the shuffle
    MPG_REQUIRE(d->y_g8 == nullptr || (cs % 8 == 0 && co_off % 8 == 0 && d->cout % 8 == 0),
                "mpg_conv2d_fused_d2s: G8 output needs c_total/4 (%d), co_off (%d) and cout (%d) multiples of 8", cs, co_off,
                d->cout);
    MPG_REQUIRE((size_t)4 * d->h * d->w < ((size_t)1 << 31), "mpg_conv2d_fused_d2s: %dx%d too large", d->h, d->w);
    const D2SOut o = {cs, co_off};
    return conv2d_fused(stream, d, &o);
}

extern "C" int mpg_conv2d_fused_window(mpg_stream_t stream, const mpg_conv_desc* d, int c_total, int co_off) {
    MPG_REQUIRE(d != nullptr, "mpg_conv2d_fused_window: null desc");
    MPG_REQUIRE(c_total >= 1 && co_off >= 0 && d->cout >= 1 && co_off + d->cout <= c_total,
                "mpg_conv2d_fused_window: channels [%d, %d) outside 0..%d", co_off, co_off + d->cout, c_total);
    // the pixel norm of the whole tensor is mpg_pixel_norm_g8 behind the last window
    MPG_REQUIRE(!d->pixel_norm, "mpg_conv2d_fused_window: no pixel norm (a window does not hold the pixel's channels)");
    // a group of 8 channels belongs to one window; only the tensor's last group may be ragged (zero padded, like the
    // last group of a plain G8 output)
    MPG_REQUIRE(d->y_g8 == nullptr || (co_off % 8 == 0 && (d->cout % 8 == 0 || co_off + d->cout == c_total)),
                "mpg_conv2d_fused_window: G8 output needs co_off (%d) a multiple of 8, and cout (%d) too unless the window ends the tensor",
                co_off, d->cout);
    const WinOut o = {c_total, co_off};
    return conv2d_fused(stream, d, nullptr, &o);
}
