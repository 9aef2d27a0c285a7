/*
 * mpgan.h -- C ABI of the MI355X (gfx950) multi-pass GAN hot path.
 *
 * The reference (maxwerhahn/Multi-pass-GAN) is pure Python over TensorFlow 1.x
 * and has no FFI of its own; every entry point below
 * therefore names the TF / numpy / scipy call site it replaces.  Citations are
 * relative to the reference tree.
 *
 * Conventions
 *   - tensors are dense NHWC float32 in device memory (HBM) unless noted (the
 *     fused convolution reads its inputs in the G8 layout defined below);
 *     pointers are borrowed, the caller (PyTorch-ROCm or any HIP program) owns
 *     the memory;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work
 *     on it and is re-entrant per stream;
 *   - return value: MPG_OK or an MPG_ERR_* code; mpg_last_error() returns a
 *     thread-local message for the last failing call.
 */
#ifndef MPGAN_H
#define MPGAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mpg_stream_t;

enum { MPG_OK = 0, MPG_ERR_ARG = 1, MPG_ERR_HIP = 2, MPG_ERR_UNSUPPORTED = 3 };

/* activation ids: tf.nn.relu / lrelu (tools_wscale/GAN.py:733-737) / tf.nn.tanh */
enum { MPG_ACT_NONE = 0, MPG_ACT_RELU = 1, MPG_ACT_LRELU = 2, MPG_ACT_TANH = 3 };

/* arithmetic of the MFMA convolution: fp16 operands, fp32 accumulation.
 * F16X1: one fp16 term per operand (fast, ~3e-4 relative error per layer);
 * F16X3: hi/lo fp16 split of both operands, three MFMA products
 *        (a_hi*w_hi + a_lo*w_hi + a_hi*w_lo), fp32-equivalent (~1e-6). */
enum { MPG_PREC_F16X1 = 1, MPG_PREC_F16F6 = 2, MPG_PREC_F16X3 = 3 };
/* F16F6: the fp16 product a_hi*w_hi plus the two correction products a_lo*w_hi and a_hi*w_lo
 *        on the block-scaled bf6 (e3m2) MFMA path at four times the fp16 rate per K, with true MX
 *        block scales (per lane and 32 K values, formed in registers from the fp16 fragments):
 *        ~2^-14 per operand at any input range, half of the F16X3 matrix work. */

/* flavour of a G8 tensor's second plane: fp16 lo (every launch reads it since round 3; the
 * {8 x fp8 hi | 8 x fp8 lo} flavour of rounds 1-2 is gone) */
enum { MPG_G8_F16 = 0 };

const char* mpg_last_error(void);
/* library / device probe: returns MPG_OK when a gfx950 device is usable. */
int mpg_device_info(int* cu_count, char* arch_name, int arch_name_len);
const char* mpg_version(void);

/* ------------------------------------------------------------------------
 * "G8" activation tensors: what fused convolutions exchange.
 *     [N][CG = ceil(C/8)][2 planes: hi, lo][H][W][8 x fp16],   value = hi + lo
 * (two fp16 numbers per value; channels beyond C are +0 in both planes).
 * Channel-group-major, so a tile row of one group is a contiguous run of
 * 16-byte pixels that LDS-DMA can stream.
 *
 * The value contract.  Every producer in this library (mpg_f32_to_g8*, the G8 outputs of the convolutions,
 * mpg_pixel_norm_g8, mpg_bn_infer_act) stores the CANONICAL split of the fp32 value v it holds:
 *     hi = fp16(v)                  correctly rounded: IEEE round to nearest even with gradual underflow,
 *     lo = fp16(fp32(v) - fp32(hi)) of the hi that is stored (the fp32 difference is exact),
 * so a consumer that reads the hi plane alone (MPG_PREC_F16X1) reads the correctly rounded fp16 of v, and two
 * producers that hold the same v store the same bytes.  The contract covers finite v with |v| <= 65504 (for the
 * scaled conversion: |v * scale| <= 65504); beyond it hi is +-inf (the value hi + lo is then NaN: lo is the opposite infinity, NaN for an infinite v), and a NaN v
 * gives NaN in both planes.
 * Accuracy: |v - (hi + lo)| <= 2^-22 |v| for 2^-3 <= |v| <= 65504.  Below 2^-3 lo reaches the fp16 subnormal
 * range (spacing 2^-24) and the error is bounded absolutely instead: |v - (hi + lo)| <= 2^-25 (tests/test_g8_host.py holds both
 * bounds against a numpy restatement and shows values just below 2^-3 that miss the relative one).  Tensors of small
 * magnitude -- gradients -- therefore go through the scaled conversion (mpg_f32_to_g8_scaled).
 * ------------------------------------------------------------------------ */
size_t mpg_g8_bytes(int n, int h, int w, int c);
/* fp32 NHWC x[..., c_off : c_off+cin] -> G8 (flavour MPG_G8_*) with ceil(cin/8) groups */
int mpg_f32_to_g8(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int c_off, int cin,
                  int flavour, void* out);
/* G8 (flavour MPG_G8_F16, c channels) -> fp32 NHWC */
int mpg_g8_to_f32(mpg_stream_t stream, const void* g8, int n, int h, int w, int c, float* y);

/* ------------------------------------------------------------------------
 * Fused convolution  (replaces GAN.convolutional_layer = tf.nn.conv2d SAME +
 * bias + batch_norm(inference) + activation, tools_wscale/GAN.py:80-119,686-691;
 * the residual sum relu(convB(.) + conv1x1(.)) of resBlock,
 * GAN/multipassGAN-4x.py:517-523, GAN/multipassGAN-out.py:227-235;
 * GAN.pixel_norm, GAN.py:472-474; the nearest upsample in front of a block,
 * GAN.py:501-523,541; the channel concat of x_in_2, multipassGAN-out.py:357.)
 *
 *   y = post( act( sum_s conv_SAME(up_s(x_s)[groups g_off_s ..], W_s) + bias ) ) + post_add
 *
 * stride 1, SAME padding (pad_before = (k-1)/2, extra pad bottom/right).
 * Each segment s contributes one K-slice of the implicit GEMM: a residual
 * shortcut is a 1x1 segment, a channel concat is two segments with the same
 * kernel size, a fused nearest upsample is up_log2 > 0 (of both axes, or with
 * up_x_only of the columns alone; segments of one launch may differ in both).
 * The result is written as fp32 NHWC (y), as G8 (y_g8), or both.
 * ------------------------------------------------------------------------ */
#define MPG_MAX_SEG 4

typedef struct mpg_conv_seg {
    const void* x;       /* G8 [N][cgroups][2][H>>up_log2][W>>up_log2][8]; up_x_only: [N][cgroups][2][H][W>>up_log2][8] */
    const void* wpack;   /* from mpg_conv_pack_weights (same cout and prec as the launch) */
    int32_t cin;         /* channels consumed, starting at channel 8*g_off of x */
    int32_t cgroups;     /* channel groups of x */
    int32_t g_off;       /* first group consumed */
    int32_t kh, kw;      /* kernel size, 1..7 */
    int32_t up_log2;     /* fused nearest upsample: src = (y >> up_log2, x >> up_log2) */
    int32_t up_x_only;   /* 0: both axes as above (h and w multiples of 1 << up_log2); 1: columns only,
                          * src = (y, x >> up_log2), only w a multiple (max_depool(height_factor=1, width_factor=upRes),
                          * GAN/multipassGAN-4x.py:558: the 4x network that upsamples z itself); other values: MPG_ERR_ARG */
    int32_t pad_hi;           /* 0: TF SAME, pad_before = (k-1)/2; 1: pad_before = k/2 (the data gradient of an even filter) */
} mpg_conv_seg;

typedef struct mpg_conv_desc {
    int32_t n, h, w;          /* output batch / height / width */
    int32_t cout;             /* 1..128 */
    int32_t nseg;             /* 1..MPG_MAX_SEG */
    mpg_conv_seg seg[MPG_MAX_SEG];
    const float* bias;        /* [cout] effective bias (bias and folded batch norm) or NULL */
    int32_t act;              /* MPG_ACT_* */
    float   leak;             /* lrelu leak (0.2 in the reference) */
    int32_t pixel_norm;       /* 1: y *= rsqrt(mean_c(y^2) + pn_eps) after act */
    float   pn_eps;           /* 1e-8 */
    const float* post_add;    /* optional fp32 [N,H,W,post_add_stride], channels post_add_coff.. added last */
    int32_t post_add_stride;
    int32_t post_add_coff;
    float*  y;                /* fp32 NHWC [N,H,W,cout] or NULL */
    void*   y_g8;             /* G8 (MPG_G8_F16) with ceil(cout/8) groups or NULL; at least one of the two outputs */
    int32_t prec;             /* MPG_PREC_* */
    int32_t reserved;         /* must be 0 */
    const float* in_amax;     /* NULL, or device pointer to the absolute maximum the segment inputs were scaled by
                               * (mpg_f32_to_g8_scaled): the sum is divided by the same power of two before bias
                               * and activation.  Used for gradients, whose magnitude is below the fp16 normal range. */
} mpg_conv_desc;

/* bytes of the packed weight image of one segment; 0 when the shape is not available at `prec` (kernel larger
 * than 7x7, cout > 128, or -- MPG_PREC_F16F6 only -- LDS images that do not fit, e.g. 7x7 with cout > 96:
 * pack such a segment for MPG_PREC_F16X3 instead). */
size_t mpg_conv_pack_size(int kh, int kw, int cin, int cout, int prec);

/* Pack W[kh,kw,w_cin_total,cout] (HWIO fp32, device; GAN.py:93) channels
 * [w_c_off, w_c_off+cin) into the MFMA fragment order, multiplying by the
 * equalised-LR constant `wscale` (GAN.py:664-668) and an optional per-output
 * channel scale (folded batch norm gamma/sqrt(var+eps), GAN.py:110). */
int mpg_conv_pack_weights(mpg_stream_t stream, const float* w_hwio, int kh, int kw,
                          int w_cin_total, int w_c_off, int cin, int cout,
                          float wscale, const float* cout_scale,
                          int prec, void* out, size_t out_bytes);

int mpg_conv2d_fused(mpg_stream_t stream, const mpg_conv_desc* desc);

/* GAN.pixel_shuffle (GAN.py:554-560: a linear 1x1 convolution to 4C channels, then tf.depth_to_space(., 2)) with the
 * shuffle in the convolution's store: the launch mpg_conv2d_fused(desc) would run, with output channel co of the
 * (h, w) grid taken as channel co_off + co of a c_total-channel tensor and written to its depth-to-space position,
 *     y[n, 2h + i, 2w + j, c] = conv[n, h, w, (2i + j) * c_total/4 + c],
 * in desc->y (fp32 [N, 2H, 2W, c_total/4]) and / or desc->y_g8 (G8 with c_total/32 groups).  Outputs wider than
 * 128 channels are several launches with their co_off.  r must be 2; no pixel norm, no post-add; MPG_PREC_F16X3 or
 * MPG_PREC_F16X1 (MPG_PREC_F16F6: MPG_ERR_UNSUPPORTED, its kernel has no such store).  The G8 output
 * requires c_total/4, co_off and desc->cout to be multiples of 8 (an 8-channel group stays in one parity): otherwise
 * MPG_ERR_ARG, and the caller runs mpg_conv2d_fused and mpg_depth_to_space. */
int mpg_conv2d_fused_d2s(mpg_stream_t stream, const mpg_conv_desc* desc, int r, int c_total, int co_off);

/* Convolutions wider than 128 outputs (the first growing level of the 8x generators at the driver's own defaults,
 * startFms 512 / maxFms 256: RES(256,256), GAN/multipassGAN-8x.py; Session._match_fused, ops.conv2d_fused_wide):
 * the launch mpg_conv2d_fused(desc) would run, desc->cout in 1..128, with its outputs stored as channels
 * [co_off, co_off + cout) of tensors that have c_total channels: desc->y is fp32 [N,H,W,c_total], desc->y_g8 a G8
 * tensor of ceil(c_total/8) groups, both given by their base address.  Nothing outside the window is written, so the
 * windows of a wide layer are launches into the same tensors, in any order.  Every precision.  post_add is allowed
 * (post_add_coff addresses its window); pixel_norm is not (MPG_ERR_ARG): a window does not hold all channels of a
 * pixel, see mpg_pixel_norm_g8.  co_off + cout <= c_total.  A G8 output needs co_off % 8 == 0, and cout % 8 == 0
 * unless the window ends the tensor: the last group is then zero padded like that of a plain G8 output; a ragged
 * window anywhere else is MPG_ERR_ARG.  The launch stays on the matrix-core kernels whatever its width (the
 * small-channel kernel writes whole tensors only). */
int mpg_conv2d_fused_window(mpg_stream_t stream, const mpg_conv_desc* desc, int c_total, int co_off);

/* A whole residual block whose three convolutions have <= 8 channels on either side, as ONE launch:
 *     y = act_b( conv_b( act_a( conv_a(up(x)) + bias_a ) ) + conv_s(up(x)) + bias_b )
 * (resBlock 0 and 3 of gen_resnet, 1 -> 2 -> 8 and 8 -> 2 -> 1 channels: GAN/multipassGAN-4x.py:505-526,560,564).
 * The middle tensor stays in LDS (as two mpg_conv2d_fused launches it made a round trip through HBM).  fp32
 * arithmetic on the exact (hi16 + lo16) inputs whatever `prec` says; wpack_* come from mpg_conv_pack_weights
 * with that `prec` (the fp32 tables of small layers follow the matrix-core image).  Odd filters only, each of the
 * three at most 7x7 (what mpg_conv_pack_weights packs); the shortcut also no larger than kh_a + kh_b - 1 by
 * kw_a + kw_b - 1, the input tile of the two filters.  Anything else is MPG_ERR_ARG, and nothing is launched. */
typedef struct mpg_small_pair_desc {
    int32_t n, h, w;          /* output batch / height / width */
    const void* x;            /* G8 input [N][cgroups][2][H>>up_log2][W>>up_log2][8] ([H][W>>up_log2] with up_x_only); one
                               * channel group is read */
    int32_t cin, cgroups, g_off, up_log2;
    const void* wpack_a;      /* conv_a: kh_a x kw_a, cin -> cmid */
    int32_t kh_a, kw_a, cmid;
    const float* bias_a;      /* [cmid] or NULL */
    int32_t act_a;
    float   leak_a;
    const void* wpack_b;      /* conv_b: kh_b x kw_b, cmid -> cout */
    int32_t kh_b, kw_b;
    const void* wpack_s;      /* shortcut conv_s: kh_s x kw_s (odd, 1..7), cin -> cout, or NULL */
    int32_t kh_s, kw_s;
    const float* bias_b;      /* [cout] or NULL (bias of conv_b plus bias of conv_s) */
    int32_t act_b;
    float   leak_b;
    int32_t cout;
    float*  y;                /* fp32 NHWC [N,H,W,cout] or NULL */
    void*   y_g8;             /* G8 (one group) or NULL; at least one of the two */
    int32_t prec;             /* MPG_PREC_* the weights were packed for */
    int32_t up_x_only;        /* as mpg_conv_seg.up_x_only: 1 = the upsample repeats columns only; 0 or 1 */
} mpg_small_pair_desc;
int mpg_conv2d_small_pair(mpg_stream_t stream, const mpg_small_pair_desc* desc);

/* out[0] = max |x_i| over the elements that are not NaN (device float; whatever out held is overwritten): +0 for n = 0,
 * for a tensor of NaNs and for a tensor of zeros of either sign, +inf when an element is +-inf.  NaN elements are
 * skipped, never propagated: the scale of a tensor with a NaN in it is that of its other elements, and the NaN itself
 * arrives in the G8 tensor as NaN.  x needs no alignment (16-byte loads are used when it has it).
 * mpg_f32_to_g8_scaled converts x * 2^k (amax == NULL: k = 0, mpg_f32_to_g8).  With *amax = m 2^e, m in [0.5, 1):
 *     k = min(9 - e, 126)      for 0 < *amax < 3.0e38,
 *     k = 0                    for *amax <= 0, NaN, and *amax >= 3.0e38 (inf included).
 * 2^(9 - e) brings the maximum into [2^8, 2^9); the cap bites for *amax < 2^-118 (fp32 subnormals included), where the
 * scaled maximum is smaller than that but 2^k and its reciprocal stay normal fp32 numbers: a tensor of any magnitude
 * converts without inf or NaN, and x 2^k is exact.  A convolution over such an input takes the same pointer in
 * desc.in_amax and multiplies its sums by 2^-k; the weight gradient multiplies by 2^-(kx + kd) in two steps, so the
 * result is right wherever it is a normal fp32 number. */
int mpg_absmax(mpg_stream_t stream, const float* x, size_t n, float* out);
int mpg_f32_to_g8_scaled(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int c_off, int cin,
                         int flavour, const float* amax, void* out);

/* Plain fp32 direct convolution on the vector ALUs, any stride / kernel /
 * channel count (tf.nn.conv2d SAME, GAN.py:686-691; used for the strided
 * discriminator convs GAN/multipassGAN-4x.py:607-614 and as an independent
 * check of the MFMA kernel).  w is HWIO fp32, multiplied by wscale on the fly.
 * y = act(conv(x, w*wscale) * cout_scale + bias). */
int mpg_conv2d_direct(mpg_stream_t stream, const float* x, int n, int h, int w, int cin,
                      const float* w_hwio, int kh, int kw, int cout, int stride_h, int stride_w,
                      float wscale, const float* cout_scale, const float* bias,
                      int act, float leak, float* y);

/* ------------------------------------------------------------------------
 * Resampling (legacy TF1 coordinates: src = dst * in/out, no half-pixel centres).
 * src is the float32 product float32(dst) * (float32(in) / float32(out)), rounded to float32 before its floor and its
 * fraction are taken (never the fraction of the unrounded product), as the TF1 kernels do.
 * ------------------------------------------------------------------------ */
/* tf.image.resize_images(method=1) / kb.resize_images (GAN.py:517,541; multipassGAN-out.py:357) */
int mpg_resize_nearest(mpg_stream_t stream, const float* x, int n, int h, int w, int c,
                       float* y, int oh, int ow);
/* tf.image.resize_images(method=0) (GAN.py:541) */
int mpg_resize_bilinear(mpg_stream_t stream, const float* x, int n, int h, int w, int c,
                        float* y, int oh, int ow);
/* tf.image.resize_images(method=2): ResizeBicubic A=-0.75, 1/1024 weight table
 * (avg_depool(mode=2), multipassGAN-out.py:330) */
int mpg_resize_bicubic(mpg_stream_t stream, const float* x, int n, int h, int w, int c,
                       float* y, int oh, int ow);
/* The residual of the upsampling_mode 0 growing generator (multipassGAN-8x.py:720-721) in one pass:
 * out[n,h,wl*f,1] = dens[n,h,wl*f,1] + resize_images(src[n,h,wl,c][..., c_src], [h, wl*f], method=2).  The rows are kept, so
 * the row weights of mpg_resize_bicubic are exactly (0, 1, 0, 0) and four column taps remain per output pixel, with that
 * entry's coordinate, table offset and weights.  f: a power of two up to 64.  out is a buffer of its own.  16-byte accesses
 * to dens / out when wl * f is a multiple of 4 and both are 16-byte aligned, scalar ones otherwise; src needs no alignment. */
int mpg_bicubic_cols_add(mpg_stream_t stream, const float* src, int n, int h, int wl, int c, int c_src, int f,
                         const float* dens, float* out);
/* tf.nn.max_pool VALID, k x k window, stride s (GAN.max_pool, GAN.py:152-159).  arg (may be NULL; one byte per output)
 * receives the window position dy * k + dx of the first maximum in scan order; mpg_max_pool_bwd sends dy there
 * (dx [n,h,w,c] is overwritten). */
int mpg_max_pool(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int k, int s, float* y,
                 unsigned char* arg);
int mpg_max_pool_bwd(mpg_stream_t stream, const float* dy, const unsigned char* arg, int n, int h, int w, int c,
                     int k, int s, float* dx);
/* tf.nn.avg_pool 2x2 VALID (GAN.py:162-169) */
int mpg_avg_pool2(mpg_stream_t stream, const float* x, int n, int h, int w, int c, float* y);
/* GAN.pixel_norm standalone (GAN.py:472-474) */
int mpg_pixel_norm(mpg_stream_t stream, const float* x, size_t npix, int c, float eps, float* y);
/* GAN.pixel_norm of a G8 tensor (MPG_G8_F16, c <= 512 channels) in place, behind the window launches of a wide layer
 * (ops.conv2d_fused_wide): x = hi + lo, y = x * rsqrt(mean_c(x^2) + eps) accumulated in fp32, written back as hi / lo
 * planes and, when y is not NULL, as fp32 NHWC [n,h,w,c] too.  The planes are the canonical split of exactly the fp32
 * values y receives, with or without y.  The padding channels of the last group are not read into the mean (the
 * divisor is c; whatever they held) and are written as zero.  n <= 65535; g8 and y 16-byte aligned. */
int mpg_pixel_norm_g8(mpg_stream_t stream, void* g8, int n, int h, int w, int c, float eps, float* y);
/* GAN.minibatch_stddev_layer (GAN.py:476-488): y[n,h,w,c+1] = concat(x, s[n % M]) with s[m] the mean over
 * (h,w,c) of the standard deviation over the G = min(group_size, n) members {g*M + m} of group m, M = n / G.
 * stat: M floats of scratch. */
int mpg_minibatch_stddev(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int group_size,
                         float* stat, float* y);
/* its gradient: dx[n,h,w,c] from dy[n,h,w,c+1] (the pass-through channels plus the statistic's dependence on
 * every member of the group); dstat: M floats of scratch. */
int mpg_minibatch_stddev_bwd(mpg_stream_t stream, const float* x, const float* dy, int n, int h, int w, int c,
                             int group_size, float* dstat, float* dx);
/* second derivative of GAN.minibatch_stddev_layer (GAN.py:476-488) for the WGAN-GP penalty (multipassGAN-8x.py:1123-1140
 * with use_mb_stddev, :847-848 and :907-908): given the upstream gradient ggx [n,h,w,c] of mpg_minibatch_stddev_bwd's dx,
 * g_x [n,h,w,c] and g_dy [n,h,w,c+1].  Per-group sums in a fixed order; partials: >= 514 * M floats (M = n / G). */
int mpg_minibatch_stddev_bwd2(mpg_stream_t stream, const float* x, const float* dy, const float* ggx, int n, int h, int w,
                              int c, int group_size, float* g_x, float* g_dy, float* partials, size_t partials_floats);
/* y = act(a + b) elementwise (tf.nn.relu(tf.add(..)), multipassGAN-4x.py:523); b may be NULL */
int mpg_add_act(mpg_stream_t stream, const float* a, const float* b, size_t n, int act, float leak, float* y);

/* ------------------------------------------------------------------------
 * Volume marshalling (generate3DUniForNewNetwork)
 * ------------------------------------------------------------------------ */
/* scipy.ndimage.zoom(v, factor on ONE axis, order=1, mode='constant')
 * (multipassGAN-out.py:401-421,465-485,527-547; multipassGAN-4x.py:1095-1103):
 * v viewed as [outer, n, inner] -> [outer, big, inner], src = o*(n-1)/(big-1). */
int mpg_axis_zoom_linear(mpg_stream_t stream, const float* v, size_t outer, int n, size_t inner,
                         float* out, int big);

/* numpy transpose of a [d0,d1,d2,c] array to axes order perm (a permutation of
 * 0,1,2; channels stay last), fused with the per-pass velocity channel
 * permutation chan_map (out[..., k] = in[..., chan_map[k]], NULL = identity;
 * multipassGAN-out.py:402-419,472-475) and the storage cutoff
 * (x < cutoff -> 0, multipassGAN-out.py:614-615; cutoff <= 0 disables). */
int mpg_volume_transpose(mpg_stream_t stream, const float* v, int d0, int d1, int d2, int c,
                         const int* perm, const int* chan_map, float cutoff, float* out);

/* add_adj_idcs channels (multipassGAN-out.py:423-436): out[i] = concat(in[i],
 * in[i-1][...,0], in[i+1][...,0]) with zeros at the ends.  in: [s, hw, c] -> out: [s, hw, c+2].
 * s_off/s_total let a rank build only its slice range of a sharded pass. */
int mpg_add_adjacent(mpg_stream_t stream, const float* in, int s_total, size_t hw, int c,
                     int s_off, int s_cnt, float* out);

/* Channel marshalling between the passes (multipassGAN-4x.py:278-283, 1095-1119: the velocity channels are cut out of the
 * low-res array, scaled by the upres factor and the velocity scale, and concatenated behind the density slices of the
 * previous pass): out[p][j] = (s[p][map[j]] * scale[j]) * scale2[j], where s is the channel-wise concatenation of
 * a [npix, ca] and b [npix, cb] (b may be NULL with cb = 0); map, scale and scale2 are HOST arrays of
 * cout <= MPG_GATHER_MAX_C entries (a NULL scale = all ones; two factors because the reference multiplies twice). */
#define MPG_GATHER_MAX_C 8
int mpg_channel_gather(mpg_stream_t stream, const float* a, int ca, const float* b, int cb, size_t npix,
                       const int* map, const float* scale, const float* scale2, int cout, float* out);

/* out[i] = v[i] < cutoff ? 0 : v[i]   (multipassGAN-4x.py:1156-1157) */
int mpg_cutoff(mpg_stream_t stream, const float* v, size_t n, float cutoff, float* out);

/* tf.nn.conv2d_transpose(x, W, output_shape = [n, h*stride_h, w*stride_w, cout], strides, "SAME") + bias + activation:
 * GAN.deconv2d / GAN.deconvolutional_layer (GAN.py:566-619, 703-708).  w_hwoi[kh,kw,cout,cin] is TensorFlow's
 * transposed-convolution filter layout (output channels before input channels).  y[n, h*stride_h, w*stride_w, cout].
 * fp32 vector-ALU gather, any stride / filter; the matrix-core route for stride 1 and 2 is composed above the ABI from
 * mpg_conv2d_fused (flipped / sub-pixel filters) and mpg_depth_to_space (ops.conv2d_transpose). */
int mpg_conv2d_transpose(mpg_stream_t stream, const float* x, int n, int h, int w, int cin, const float* w_hwoi,
                         int kh, int kw, int cout, int stride_h, int stride_w, float wscale, const float* bias,
                         int act, float leak, float* y);
/* tf.depth_to_space(x, r) (GAN.pixel_shuffle, GAN.py:554-560): x[n,h,w,c] -> y[n, h*r, w*r, c / r^2] */
int mpg_depth_to_space(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int r, float* y);
/* its adjoint, the gradient of GAN.pixel_shuffle's shuffle (GAN.py:554-560): x[n,h,w,c] -> y[n, h/r, w/r, c * r^2],
 * y[n, q, p, (i*r + j)*c + k] = x[n, r*q + i, r*p + j, k]; h and w multiples of r */
int mpg_space_to_depth(mpg_stream_t stream, const float* x, int n, int h, int w, int c, int r, float* y);

/* ------------------------------------------------------------------------
 * Device-side DEFLATE of a .uni payload: replaces the gzip.open(...).write(content.tobytes()) of the reference writer
 * (tools_wscale/uniio.py:91-123), whose zlib pass over the whole volume is the longest step of a 4x frame.
 * The payload is cut into units of MPG_DEFLATE_UNIT bytes.  Every unit becomes a byte-aligned, NON-final raw DEFLATE
 * stream (RFC 1951): one fixed-Huffman block of word-granular tokens (a word equal to its predecessor extends a run,
 * runs become matches of distance 4 and length 4 * min(r, 64), every other word is four literals) closed by an empty
 * stored block, or, where that would be longer, one stored block.  Unit streams concatenate into one deflate body;
 * the caller ends a body with an empty final block (bytes 03 00).
 * ------------------------------------------------------------------------ */
#define MPG_DEFLATE_UNIT 32768                       /* payload bytes per unit */
#define MPG_DEFLATE_SLOT (MPG_DEFLATE_UNIT + 16)     /* workspace bytes per unit: the stored form (5 + unit), 16-byte slots */
#define MPG_DEFLATE_SLAB (64 << 20)                  /* most payload bytes per encode call */
/* bytes of slot workspace for n_bytes of payload (uniio.py:91-123) */
size_t mpg_deflate_ws_bytes(size_t n_bytes);
/* encode n_bytes (a positive multiple of 4, at most MPG_DEFLATE_SLAB; src 16-byte aligned) of payload (uniio.py:91-123):
 * unit u's stream goes to slots + u * MPG_DEFLATE_SLOT (slots: mpg_deflate_ws_bytes(n_bytes), 16-byte aligned),
 * its length to sizes[u], and the CRC-32 (zlib.crc32) of its input bytes to crcs[u]; ceil(n_bytes / unit) units. */
int mpg_deflate_encode(mpg_stream_t stream, const void* src, size_t n_bytes, void* slots, uint32_t* sizes,
                       uint32_t* crcs);
/* mpg_deflate_encode with a Huffman code per unit (uniio.py:91-123): same arguments, units, tokens, slots and CRCs; the
 * literal/length symbols of a unit are coded with canonical codes of at most 15 bits built from the unit's own counts
 * (ties by symbol index, so a unit always gives the same bytes) in one dynamic block (BTYPE 10) closed by the empty
 * stored block.  A unit is written in whichever of the dynamic, fixed and stored forms is shortest, so sizes[u] is
 * never above what mpg_deflate_encode reports. */
int mpg_deflate_encode_dynamic(mpg_stream_t stream, const void* src, size_t n_bytes, void* slots, uint32_t* sizes,
                               uint32_t* crcs);
/* compaction (uniio.py:91-123): out[sum(sizes[0..u)) ...] = the sizes[u] bytes of slot u, for u < n_units; nothing is
 * written at or beyond out + out_bytes. */
int mpg_deflate_compact(mpg_stream_t stream, const void* slots, const uint32_t* sizes, size_t n_units, void* out,
                        size_t out_bytes);
/* The way back: replaces the gzip.open(...).read() of the reference reader (tools_wscale/uniio.py:81-88) for files whose
 * members record their unit sizes (uniio.unit_index).  Decodes n_units = ceil(n_bytes / MPG_DEFLATE_UNIT) unit streams in
 * parallel.  offsets and sizes are HOST arrays: unit u's stream is the sizes[u] bytes at packed + offsets[u] (any
 * alignment).  packed (device, 16-byte aligned, packed_bytes a multiple of 16) is read only in the 16-byte lines a stream
 * touches.  The call fails with MPG_ERR_ARG before anything is launched if a stream leaves packed_bytes; it uploads the two
 * arrays in stream order and returns once they are on the device (the kernel may still be running).
 * Unit u's bytes go to out + u * MPG_DEFLATE_UNIT (device, 16-byte aligned; the last unit takes the rest of n_bytes, a
 * positive multiple of 4), their CRC-32 to crcs[u], and to status[u] 0 = decoded, 1 = valid DEFLATE outside the token
 * language of mpg_deflate_encode (another distance, a final block, output that is not word-granular), 2 = corrupt
 * (bad code, LEN / NLEN, input or output that ends early or late).  With a non-zero status the unit's output and CRC are
 * unspecified, but nothing outside the unit's output range is written, whatever the bytes say. */
int mpg_inflate_units(mpg_stream_t stream, const void* packed, size_t packed_bytes, const uint64_t* offsets,
                      const uint32_t* sizes, size_t n_units, void* out, size_t n_bytes, uint32_t* crcs, uint32_t* status);

/* ------------------------------------------------------------------------
 * Training step: what tf.gradients produces for
 * the layers of GAN.py, and the optimiser update.  fp32 NHWC device tensors;
 * geometry is tf.nn.conv2d SAME of an [n,h,w,cin] input (GAN.py:686-691).
 * ------------------------------------------------------------------------ */
/* d loss / d W for W stored unscaled (GAN.py:664-668): dw[kh,kw,cin,cout] =
 * wscale * sum_p x[p + tap] * dy[p].  dy is [n, ceil(h/sh), ceil(w/sw), cout]; dw is overwritten. */
int mpg_conv2d_wgrad(mpg_stream_t stream, const float* x, int n, int h, int w, int cin, const float* dy,
                     int cout, int kh, int kw, int stride_h, int stride_w, float wscale, float* dw);
/* The same weight gradient on the matrix cores for stride-1 filters (kh <= 7, kw in 1,3,4,5):
 * x and dy are converted to G8 (fp16 hi + lo planes, power-of-two scaled; mpg_f32_to_g8_scaled) inside
 * `workspace` (>= mpg_conv2d_wgrad_mfma_ws_bytes, 256-byte aligned), then contracted over pixels
 * with v_mfma_f32_32x32x16_f16, the pixel-major fragments read out of the channel-grouped G8 rows with the
 * transposing LDS read (ds_read_b64_tr_b16).  prec MPG_PREC_F16X3 (three products, fp32-grade) or MPG_PREC_F16X1.
 * dy_amax / x_amax (device scalars, may be NULL): max |dy| / max |x| when the caller already has them (the kernel that
 * produced dy returns it; a forward activation needs no scaling: pass a scalar holding 256.0f = scale 1) -- without
 * them each costs a reduction pass over its tensor. */
size_t mpg_conv2d_wgrad_mfma_ws_bytes(int n, int h, int w, int cin, int cout);
int mpg_conv2d_wgrad_mfma(mpg_stream_t stream, const float* x, int n, int h, int w, int cin,
                          const float* dy, int cout, int kh, int kw, float wscale, int prec,
                          void* workspace, size_t workspace_bytes, const float* dy_amax, const float* x_amax,
                          float* dw);
/* ... with both operands already in G8 (MPG_G8_F16, 16-byte aligned): the layer's forward input as mpg_conv2d_fused
 * read it, and the scaled dy the data-gradient convolution reads -- no conversion pass and no workspace.
 * x_amax / dy_amax: the device scalars the tensors were scaled with by mpg_f32_to_g8_scaled, NULL for an unscaled one.
 * This is what tf.gradients' Conv2DBackpropFilter does for the layers of GAN.py:686-691 under multipassGAN-4x.py:880-902. */
int mpg_conv2d_wgrad_g8(mpg_stream_t stream, const void* x_g8, int n, int h, int w, int cin, const void* dy_g8, int cout,
                        int kh, int kw, float wscale, int prec, const float* x_amax, const float* dy_amax, float* dw);
/* The launches the two entries above make for a shape, in launch order: a query like mpg_conv_pack_size, host arithmetic
 * only (no device is touched).  Returns the number of launches, 0 for a shape or filter the entries refuse, and fills
 * records[i * MPG_WGRAD_PLAN_INTS + field] for the first max_records of them (records may be NULL to count only).
 * Fields of a record (a field of the other form is 0):
 *    0 form            MPG_WGRAD_FORM_ROW: one filter row per block; MPG_WGRAD_FORM_RING: all rows of a square 3x3 / 4x4 / 5x5
 *                      filter per block, x rows in an LDS ring
 *    1 k               kernel instantiation: filter width (row form), filter size (ring form)
 *    2 cotw            ... cout tiles of 32 per wave (row form) / per window (ring form)
 *    3 prec            ... products: 3 (MPG_PREC_F16X3) or 1 (MPG_PREC_F16X1)
 *    4 blocks          grid size, padding blocks included
 *    5 lds_bytes       dynamic LDS of a block
 *   row form: a launch covers input channels [ci0, ci0 + cin) and `windows` windows of `cout` output channels from co0
 *    6 ci0   7 co0   8 cin   9 cout
 *   10 cit             ci tiles of 32, one per wave
 *   11 cog             groups of cotw cout tiles, one per wave
 *   12 ks              waves that share the 16-pixel k-steps of a chunk (cit * cog * ks <= 8 waves)
 *   13 chunk           pixels of a row staged at a time
 *   14 windows         equal cout windows merged into this launch (>= 1)
 *   15 nsplit          blocks per filter row and window: ranges of the n * h image rows
 *   16 rows_per_split  image rows of a range
 *   ring form: one launch covers all channels
 *   17 chunks          column chunks of 64 pixels per row
 *   18 n_ci            ci tiles of 32
 *   19 n_cow           cout windows of 32 * cotw
 *   20 ranges          row ranges per image
 *   21 rows_per_range  output rows of a range
 *   22 n_outer         n * ranges * chunks; each runs n_ci * n_cow blocks
 *   23 reserved        0 */
#define MPG_WGRAD_PLAN_INTS 24
#define MPG_WGRAD_FORM_ROW 0
#define MPG_WGRAD_FORM_RING 1
int mpg_conv2d_wgrad_plan(int n, int h, int w, int cin, int cout, int kh, int kw, int prec, int32_t* records, int max_records);
/* dy_amax: NULL, or a device float holding max |dy| already computed with mpg_absmax */
/* d loss / d x of the same convolution, any stride / filter size (the strided 4x4 discriminator
 * convs, multipassGAN-4x.py:607-614).  The filter is passed with its channel axes swapped,
 * w_hwoi[kh,kw,cout,cin].  Stride-1 filters can instead run mpg_conv2d_fused on dy with the
 * flipped w_hwoi and pad_hi = 1. */
int mpg_conv2d_dgrad(mpg_stream_t stream, const float* dy, int n, int h, int w, int cin,
                     const float* w_hwoi, int cout, int kh, int kw, int stride_h, int stride_w,
                     float wscale, float* dx);
/* GAN.fully_connected_layer (GAN.py:438-456): y[rows,cout] = act(x[rows,k] @ (w[k,cout] * wscale) + bias).
 * Its gradients are mpg_conv2d_wgrad / mpg_conv2d_dgrad with h = w = 1. */
int mpg_fc_forward(mpg_stream_t stream, const float* x, int rows, int k, const float* w, int cout,
                   float wscale, const float* bias, int act, float leak, float* y);
/* out[c] = sum over pixels of x[p, c]  (bias gradient, GAN.py:683), the blocks' sums added in a fixed order:
 * partials holds >= mpg_bn_partials_floats(c) + c floats */
int mpg_channel_sum_ordered(mpg_stream_t stream, const float* x, size_t npix, int c, float* out, float* partials,
                            size_t partials_floats);
/* tf.contrib.layers.batch_norm(is_training=True) (GAN.py:110): batch mean / biased variance over
 * all pixels, y = act((x - mean) * rsqrt(var + eps) * gamma + beta); the moments are returned, and
 * the moving averages (the UPDATE_OPS, multipassGAN-4x.py:773-776) are advanced in place when
 * moving_mean / moving_var are given: moving = decay * moving + (1 - decay) * batch.
 * The blocks' partial sums are kept in `partials` (>= mpg_bn_partials_floats(c) floats of device memory) and
 * added in block order, not by atomics: the batch statistics -- and with them every ReLU mask of the step -- are
 * then the same bits on every run (a pre-activation within 1e-6 of zero otherwise changes side now and then, and one
 * flipped mask element moves the gradients upstream of it by 1 / sqrt(elements): DESIGN section 10).
 * The moments come from one pass over x around a per-channel shift (the mean of 64 pixels spread through the batch) that
 * is kept in batch_mean while x is read: batch_mean and batch_var must not overlap x or each other. */
size_t mpg_bn_partials_floats(int c);
int mpg_bn_train_fwd_ordered(mpg_stream_t stream, const float* x, size_t npix, int c, const float* gamma,
                             const float* beta, float eps, int act, float leak, float* y, float* batch_mean,
                             float* batch_var, float* moving_mean, float* moving_var, float decay, float* partials,
                             size_t partials_floats);
/* gradient of the normalisation above (dy is taken before the activation).  amax (may be NULL) receives max |dx|:
 * the data- and weight-gradient convolutions that consume dx scale it by a power of two before the fp16 split
 * (mpg_absmax would re-read the tensor for it).  The blocks' partial sums of dbeta / dgamma are kept in `partials`
 * (mpg_bn_partials_floats(c) floats) and added in a fixed order, as mpg_bn_train_fwd_ordered does for the statistics */
int mpg_bn_train_bwd_ordered(mpg_stream_t stream, const float* dy, const float* x, size_t npix, int c,
                             const float* batch_mean, const float* batch_var, const float* gamma, float eps,
                             float* dx, float* dgamma, float* dbeta, float* amax, float* partials, size_t partials_floats);
/* second derivative of the normalisation above, for the WGAN-GP penalty through a batch-normalised critic
 * (tf.gradients at y_gp, multipassGAN-8x.py:1123-1140, differentiating batch_norm(is_training=True) of GAN.py:108-110 twice).
 * The first backward maps (dz, x, gamma) -> (dx, dgamma, dbeta); given the upstream gradients gdx [npix,c], gdgamma [c],
 * gdbeta [c] (each may be NULL = zero) it returns g_dz [npix,c], g_x [npix,c] and g_gamma [c].  The per-channel sums are
 * block sums in `partials` (mpg_bn_partials_floats(c) floats) added in a fixed order: the same bits on every run. */
int mpg_bn_train_bwd2_ordered(mpg_stream_t stream, const float* dz, const float* x, size_t npix, int c,
                              const float* batch_mean, const float* batch_var, const float* gamma, float eps,
                              const float* gdx, const float* gdgamma, const float* gdbeta, float* g_dz, float* g_x,
                              float* g_gamma, float* partials, size_t partials_floats);
/* dx = dy * act'(.) written through the activation OUTPUT y (relu, lrelu GAN.py:733-737, tanh); amax as above */
int mpg_act_bwd(mpg_stream_t stream, const float* dy, const float* y, size_t n, int act, float leak, float* dx,
                float* amax);
/* gradient of GAN.pixel_norm (GAN.py:472-474) */
int mpg_pixel_norm_bwd(mpg_stream_t stream, const float* dy, const float* x, size_t npix, int c, float eps,
                       float* dx);
/* Second-order companions of mpg_act_bwd, mpg_pixel_norm_bwd and mpg_max_pool_bwd: what a gradient penalty (a gradient
 * of a gradient) through tanh, GAN.pixel_norm and GAN.max_pool needs.  Each takes a cotangent g of the first backward's
 * output.  The derivative with respect to the first backward's dy is that backward itself applied to g (all three are
 * linear in dy) and has no entry of its own; these are the remaining terms.  64-bit offsets, no atomics, every element of
 * the output is written, the same input gives the same bits.  Null pointers and bad shapes are refused (MPG_ERR_ARG)
 * before anything is launched.
 *
 * mpg_act_bwd2: mpg_act_bwd's dx = dy * (1 - y^2) (MPG_ACT_TANH) differentiated in y, n elements:
 *     d_y = ((-2 * y) * dy) * g          two rounded float32 products (-2 * y is exact), in that order.
 *   16-byte accesses when dy, y, g and d_y are all 16-byte aligned, scalar ones otherwise; n == 0 launches nothing.  Every
 *   other act is MPG_ERR_ARG: relu and lrelu are piecewise linear, their derivative in y is zero and the caller passes
 *   nothing on; `leak` is ignored.
 *
 * mpg_pixel_norm_bwd2: mpg_pixel_norm_bwd's dx = r dy - r^3 s x differentiated in x ([npix, c] each, npix, c >= 1):
 *     r = rsqrt(mean_c(x^2) + eps), s = mean_c(x dy), t = mean_c(x g), u = mean_c(dy g)
 *     d_x = -r^3 (u x + s g + t dy) + 3 r^5 s t x
 *   in float32 in this order: lanes = the largest power of two <= min(c, 64) lanes share a pixel; each of the four sums is
 *   an fmaf chain from 0 over the lane's channels l, l + lanes, ..., folded by a xor tree from lanes / 2 down to 1 and
 *   divided by (float)c; m = Sxx / c + eps, r = rsqrtf(m), r2 = r r, r3 = r2 r, k = (((3 r3) r2) s) t,
 *   p_i = fmaf(t, dy_i, fmaf(s, g_i, u x_i)), d_x_i = fmaf(k, x_i, -(r3 p_i)).  A pixel of zeros gives zeros.  No alignment
 *   is asked of any pointer.  More than (2^31 - 1) * 256 / lanes pixels are refused.
 *
 * mpg_max_pool_gather: the adjoint of mpg_max_pool_bwd, with its geometry (g [n,h,w,c]; arg and out [n,oh,ow,c],
 *   oh = (h - k) / s + 1, ow = (w - k) / s + 1; n, c >= 1, 1 <= k <= 15, s >= 1, h, w >= k, else MPG_ERR_ARG):
 *     out[b,oy,ox,ch] = g[b, s oy + a / k, s ox + a % k, ch],  a = arg[b,oy,ox,ch]
 *   a copy, bit for bit.  arg is the plane mpg_max_pool writes (a < k k); a byte outside the window reads nothing and
 *   gives 0. */
int mpg_act_bwd2(mpg_stream_t stream, const float* dy, const float* y, const float* g, size_t n, int act, float leak,
                 float* d_y);
int mpg_pixel_norm_bwd2(mpg_stream_t stream, const float* dy, const float* x, const float* g, size_t npix, int c, float eps,
                        float* d_x);
int mpg_max_pool_gather(mpg_stream_t stream, const float* g, const unsigned char* arg, int n, int h, int w, int c, int k,
                        int s, float* out);
/* gradient of the nearest upsample by integer factors (GAN.py:517; dy is [n,oh,ow,c]) */
int mpg_resize_nearest_bwd(mpg_stream_t stream, const float* dy, int n, int oh, int ow, int c, float* dx,
                           int h, int w);
/* gradients of mpg_resize_bilinear / mpg_resize_bicubic (tf.image.resize_images method 0 / 2, GAN.py:541; the upsampling
 * inside the first 8x generator with upsampleMode 0 / 2, multipassGAN-8x.py:629).  dy is [n,oh,ow,c]; dx [n,h,w,c] is
 * overwritten, every element, those that no output reads with 0.  Any h, w, oh, ow >= 1, as in the forward.  The resize is
 * Y = R_h X R_w^T, the gradient R_h^T dY R_w in two gather passes (along H into tmp, n*h*ow*c floats provided by the caller,
 * then along W) with the forward's coordinates, indices and clamping; the bicubic weights carry the bits of the TF1
 * coefficient table.  The order of every sum is fixed: the same dy gives the same bits. */
int mpg_resize_bilinear_bwd(mpg_stream_t stream, const float* dy, int n, int oh, int ow, int c, float* dx,
                            int h, int w, float* tmp);
int mpg_resize_bicubic_bwd(mpg_stream_t stream, const float* dy, int n, int oh, int ow, int c, float* dx,
                           int h, int w, float* tmp);
/* gradient of mpg_avg_pool2 (dx is [n,h,w,c], dy [n,h/2,w/2,c]) */
int mpg_avg_pool2_bwd(mpg_stream_t stream, const float* dy, int n, int h, int w, int c, float* dx);
/* lerp(x, y, t) = x + (y - x) * t with t already clipped to [0,1] (multipassGAN-8x.py:598-599); x NULL = zeros */
int mpg_lerp(mpg_stream_t stream, const float* x, const float* y, size_t n, float t, float* out);
/* tensorResample (multipassGAN-4x.py:398-441; 8x.py:547-595), 2D: out[b,i,j,:] = bilinear look-up of
 * value[b] at pos[b,i,j] = (y, x) in cell-centred coordinates, indices clamped to the grid when `clamp`
 * (script default); the advection step of the temporal discriminator inputs.  _bwd: gradient with
 * respect to value (dvalue is overwritten). */
int mpg_tensor_resample(mpg_stream_t stream, const float* value, const float* pos, int n, int h, int w, int c,
                        int clamp, float* out);
int mpg_tensor_resample_bwd(mpg_stream_t stream, const float* dy, const float* pos, int n, int h, int w, int c,
                            int clamp, float* dvalue);
/* The temporal critic's input with useVelInTDisc (multipassGAN-8x.py:1204-1208, read as [-1,th,th,12] at :878): frames
 * [3B,th,th,1] (advected, at tile size th) and x_t [3B,tl,tl,4] (velocity in channels 1..3) -> out [B, 12 th th], the
 * reference's reshape [-1,3,P] / transpose (0,2,1) of concat(frames, scale * legacy-bilinear resize of the velocity to
 * [th,th]) in one pass; the velocity values have the bits of scale * mpg_resize_bilinear.  th % tl == 0. */
int mpg_tempo_vel_pack(mpg_stream_t stream, const float* frames, const float* x_t, int B, int tl, int th, float scale,
                       float* out);
/* gradient of mpg_tempo_vel_pack with respect to the frames (multipassGAN-8x.py:1204-1208 read backwards): dframes
 * [3B,th,th,1] gathers its element of dout [B, 12 th th]; the velocity slots of dout reach nothing. */
int mpg_tempo_vel_pack_bwd(mpg_stream_t stream, const float* dout, int B, int th, float* dframes);
/* One optimiser call of the 8x training loop (multipassGAN-8x.py:1305-1362 with the dynamic loss scaling of :490-541):
 * Adam on the elements of the flat buffer whose `mask` entry is non-zero (the variables of the current growing
 * stage; NULL = all), on the gradient times coef = exp(-ls_var ln 2) / total_grads (use_loss_scaling; the gradient
 * buffer holds d(loss * 2^ls_var)), applied only if every such product is finite -- otherwise nothing moves and
 * ls_var -= ls_dec; after an applied update ls_var += ls_inc and the optimiser's own step count t advances, from which
 * lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) is formed (lr: one float in DEVICE memory).  ema_shadow (or NULL):
 * MovingAverageOptimizer shadow of p, pulled towards the new values with (1 - ema_decay) on applied updates.
 * state: 8 floats of device memory owned by the optimiser, [0] = ls_var, [3] = t (initialise to 64 / 0).
 * Everything is decided on the device: a captured hipGraph of the iteration replays correctly. */
int mpg_adam_step_staged(mpg_stream_t stream, float* p, const float* grad, float* m, float* v, const float* mask,
                         size_t n, float* state, const float* lr, int total_grads, int use_loss_scaling,
                         float beta1, float beta2, float eps, float ls_inc, float ls_dec, float* ema_shadow,
                         float ema_decay);
/* GAN.advect (GAN.py:347-418): semi-Lagrangian / MacCormack advection of [n,h,w,c] fields (2D, h == w) for the
 * temporal-coherence branch with adv_mode 1 / 2 (multipassGAN-8x.py:1199,1225).
 *   mpg_advect_velocity: vel[n,hv,wv,cv] with channels (x, y, ..) -> out[n,h,w,2] = the (y, x) displacement the look-up
 *     uses: legacy-bilinear resize to [h,w], times max(h/hv, w/wv), averaged with its successor along its own axis
 *     (MAC -> cell centre, zero past the end), times dt * (+1, 0, -1)[b % 3] (:376-396); n is a multiple of 3.
 *   mpg_semi_lagrange: out[b,i,j,:] = sum over the 2x2 cells around q = (i + 0.5, j + 0.5) - sign * vel[b,i,j] of
 *     source * prod(1 - |q - index|), indices clamped to the grid, weights from the clamped indices (:175-204).
 *     _bwd: gradient with respect to source (dsource is overwritten).
 *   mpg_maccormack (one channel): the MacCormack correction forward + strength/2 (source - backward) where
 *     flags < 0.2, clamped back to `forward` where it leaves the [min, max] of the fluid cells around the truncated
 *     look-up position (:206-343, index clipping as written there: for three of the four corners the batch index is
 *     clipped to w-1 too -- and so is the row index, which for h < w would leave the batch entry: h != w is
 *     MPG_ERR_ARG, decided on the host before anything is launched).  keep (may be NULL) receives 1 where the
 *     correction term survived: the only place where d out / d source differs from the semi-Lagrangian one
 *     (TensorFlow differentiates tf.where by its branches). */
int mpg_advect_velocity(mpg_stream_t stream, const float* vel, int n, int hv, int wv, int cv, int h, int w, float dt,
                        float* out);
int mpg_semi_lagrange(mpg_stream_t stream, const float* source, const float* vel, int n, int h, int w, int c,
                      float vel_sign, float* out);
int mpg_semi_lagrange_bwd(mpg_stream_t stream, const float* dy, const float* vel, int n, int h, int w, int c,
                          float vel_sign, float* dsource);
int mpg_maccormack(mpg_stream_t stream, const float* source, const float* forward, const float* backward,
                   const float* flags, const float* vel, int n, int h, int w, float strength, float* out, float* keep);
/* ------------------------------------------------------------------------
 * Training-tile supply on device-resident frames (tools_wscale/tilecreator_t.py).  The random
 * decisions stay on the host (multi-pass-gan_amd/tiles_device.py); these are the array operations.
 *   mpg_tile_gather: out[b] = frames[f][z0:z0+tz, y0:y0+ty, x0:x0+tx, c0:c0+c] with (f, c0, z0, y0, x0) = table[5 b ..]
 *     (cutTile / getDatum, :403-450,562-574); frames [n_frames, z, y, x, cf], table in device memory.
 *   mpg_resample_affine: scipy.ndimage.affine_transform / zoom with order 1, mode 'constant', cval 0 of a [zs,ys,xs,c]
 *     array (:808-879): source coordinate = matrix9 * (z,y,x)_dst + offset3 in float64; channel_mix (c x c, or NULL)
 *     is applied to the interpolated channels (vector components rotate / scale with the grid, :700-760,846-856).
 *   mpg_tile_orient: crop [off, off + size) of src, axes permuted / reversed (the composed np.rot90 / np.flip of
 *     :762-806), channels permuted / negated (chan_map, chan_sign: the vector components follow the turn).
 *   Both take 1 <= c <= MPG_TILE_MAX_CHANNELS packed channels (more: MPG_ERR_ARG, nothing launched).  The widest tile
 *     the drivers cut is 'd,vx,vy,vz,d,d' x 3 coherent frames = 18 (the first 8x network with useVelocities and
 *     add_adj_idcs); 24 leaves room for a seventh and eighth channel per frame, and the c x c mix, passed by value,
 *     keeps resample_kernel's arguments at 2.4 KiB of the 4 KiB a kernel may take.
 *   mpg_semilagr_positions: getSemiLagrPosBatch (:1345-1378), 2D: vel [n_batch,h,w,3] (MAC, x,y,z), dt [n_batch] ->
 *     pos [n_batch, n_out, n_out, 2] = (y, x) - v dt. */
#define MPG_TILE_MAX_CHANNELS 24
int mpg_tile_gather(mpg_stream_t stream, const float* frames, int n_frames, int z, int y, int x, int cf,
                    const int* table, int n_tiles, int tz, int ty, int tx, int c, float* out);
int mpg_resample_affine(mpg_stream_t stream, const float* src, int zs, int ys, int xs, int c, float* dst, int zd, int yd,
                        int xd, const double* matrix9, const double* offset3, const float* channel_mix);
int mpg_tile_orient(mpg_stream_t stream, const float* src, int zs, int ys, int xs, int c, const int* crop_off3,
                    const int* crop_size3, const int* perm3, const int* flip3, const int* chan_map,
                    const float* chan_sign, float* dst);
int mpg_semilagr_positions(mpg_stream_t stream, const float* vel, const float* dt, int n_batch, int h, int w, int n_out,
                           float* pos);
/* The vorticity input channels of useVorticities (addVorticity, GAN/multipassGAN-8x.py:1440-1446, 2D branch as written;
 * called per batch and per temporal batch at -8x.py:1482-1490,1508-1511 and -4x.py:491-499,1026-1029).
 * x [n,h,w,c] fp32 -> y [n,h,w,c+3] fp32, not overlapping:  y[..., :c] = x;  y[..., c] = y[..., c+1] = 0;
 *   y[i,j,c+2] = 0.5f * ((x[i+1,j,2] - x[i-1,j,2]) - (x[i,j+1,1] - x[i,j-1,1]))  for 1 <= i <= h-2, 1 <= j <= w-2
 * (i the row, j the column), 0 elsewhere -- all of it when h < 3 or w < 3.  Not the textbook curl; bit-defined (no
 * contraction possible).  One read of x, one write of y, 64-bit offsets.  MPG_ERR_ARG: c < 4, h or w < 1, n < 0, null
 * pointers, more than 2^32 - 1 pixels; n == 0 (with a valid h, w, c) succeeds, launches nothing and does not look at the
 * pointers. */
int mpg_vorticity_append(mpg_stream_t stream, const float* x, int n, int h, int w, int c, float* y);
/* ------------------------------------------------------------------------
 * Slice mode of the training-set loader on a device-resident source (tools_wscale/fluiddataloader.py:387-544; SURVEY 8f
 * rank 2).  File handling and every random draw stay on the host (multi-pass-gan_amd/fluiddataloader_device.py).
 * Both entries work on the virtual array V = scipy.ndimage.zoom(transpose(src, perm3 + (3,)), order=1), which is never
 * stored: src [dims3[0], dims3[1], dims3[2], c] fp32, perm3 the axis order of the slice view (:416-431; NULL = identity),
 * out3 V's spatial size (int(round(n * factor)) per axis, from the caller).  Along an axis of n source and o output
 * points index i reads the coordinate i * ((n - 1) / (o - 1)), in float64 (i * 1.0 where o == 1), and is 0 where that
 * exceeds n - 1, as scipy's; fp32 linear weights, axis by axis; an axis whose weight is 0 takes no blend, so factor 1
 * returns the source's bits.
 *   mpg_slice_zoom_means: means[s] = mean over (i, j) of V[s, i, j, chan], s in [0, out3[0]) -- the quantity
 *     removeSlices compares with density_threshold (:295-313).  Block sums added in a fixed order: the same bits on every
 *     run.  workspace: at least 64 * out3[0] floats of device memory.
 *   mpg_slice_zoom_gather: out[r, i, j, c_off + q] = V[slices[r], i, j, chan_map[q]], q in [0, n_chan); slices (device
 *     memory) holds n_slices indices along V's axis 0; a row of out has out_c channels, so several sources fill their
 *     channel windows of one array.  chan_map (host memory, NULL = identity, n_chan <= 16) carries the exchange of
 *     velocity components of the slice view.  adj != 0 is addAdjSlices (:315-336): n_chan is three packed frames, each
 *     followed by channel 0 of that frame in V[slices[r] - 1] and in V[slices[r] + 1] (0 beyond the ends), n_chan + 6
 *     channels written. */
int mpg_slice_zoom_means(mpg_stream_t stream, const float* src, const int* dims3, int c, const int* perm3,
                         const int* out3, int chan, float* means, float* workspace, size_t workspace_floats);
int mpg_slice_zoom_gather(mpg_stream_t stream, const float* src, const int* dims3, int c, const int* perm3,
                          const int* out3, const int* slices, int n_slices, const int* chan_map, int n_chan, int adj,
                          float* out, int out_c, int c_off);

/* the reductions of the generator losses (multipassGAN-4x.py:754,764-765): out[0] = sum |a - b| (mode 0,
 * tf.reduce_mean(tf.abs(..)) after division by n) or sum (a - b)^2 (mode 1, 2 * tf.nn.l2_loss); b NULL = 0 */
int mpg_pair_reduce(mpg_stream_t stream, const float* a, const float* b, size_t n, int mode, float* out);
/* tf.train.AdamOptimizer update on a flat parameter buffer (multipassGAN-4x.py:880-902):
 * m += (g-m)(1-b1); v += (g*g-v)(1-b2); p -= lr_t * m / (sqrt(v) + eps), with
 * lr_t = lr * sqrt(1-b2^t)/(1-b1^t) computed by the caller and read from DEVICE memory (one float),
 * so that a captured hipGraph of the iteration can be replayed with a new step size. */
int mpg_adam_step(mpg_stream_t stream, float* p, const float* grad, float* m, float* v, size_t n,
                  const float* lr_t, float beta1, float beta2, float eps);

/* Held-out evaluation: the "test model" section of the training loops (multipassGAN-4x.py:1410-1500,
 * multipassGAN-8x.py:2094-2196), which runs the networks with train: False and fetches means of the critic outputs.
 *   mpg_logit_stats: out6 = means over the n logits of { l, sigmoid(l), sigmoid cross entropy against label 1, against
 *     label 0 (tf.nn.sigmoid_cross_entropy_with_logits: max(l,0) - l z + log1p(exp(-|l|))), (l - 1)^2, l^2 }.  One block,
 *     sums folded in a fixed order, no atomics, nothing cleared: the same input gives the same bits, and the call is safe
 *     inside a captured hipGraph.  A critic output has one logit per tile; n is not limited.
 *   mpg_bn_infer_act: tf.contrib.layers.batch_norm(is_training=False) + activation (GAN.py:108-119) on [n,h,w,c] with the
 *     moving averages given: y = act((x - mean) * rsqrt(var + eps) * gamma + beta); nothing is updated.  y (fp32 NHWC)
 *     and / or y_g8 (G8, MPG_G8_F16, mpg_g8_bytes(n,h,w,c), 16-byte aligned; equal to mpg_f32_to_g8 of y bit for bit).
 *     Without y_g8 this launches the apply kernels of mpg_bn_train_fwd_ordered.
 *   mpg_tiles_to_gray8: tiles [n_tiles,th,tw,c] -> n_tiles / (rows*cols) mosaics [rows*th, cols*tw] of channel `channel`
 *     as 8-bit grey, uint8(clip(v,0,1) * 255) truncated (tilecreator_t.savePngsGrayscale, :1125-1157): one byte per
 *     pixel leaves the device. */
int mpg_logit_stats(mpg_stream_t stream, const float* logits, size_t n, float* out6);
int mpg_bn_infer_act(mpg_stream_t stream, const float* x, int n, int h, int w, int c, const float* mean,
                     const float* var, const float* gamma, const float* beta, float eps, int act, float leak,
                     float* y, void* y_g8);
int mpg_tiles_to_gray8(mpg_stream_t stream, const float* tiles, int n_tiles, int th, int tw, int c, int channel,
                       int rows, int cols, unsigned char* out);

/* Preview images of the inference drivers, taken from a pass volume vol [a,b,c] fp32 where it lies in device memory.
 *   mpg_volume_projections: the three axis sums of save_img_3d (multipassGAN-out.py:208-210, called with dim_output / 80
 *     at :461,523,585; multipassGAN-4x.py:1134,1146; multipassGAN-8x.py:1718):
 *       p0[j,k] = sum_i fl(vol[i,j,k] / divisor), p1[i,k] = sum_j ..., p2[i,j] = sum_k ...
 *     The division is per element and correctly rounded, before the sums, as the reference orders it.  One read of the
 *     volume: tiles write partial sums into ws (mpg_volume_projections_ws_bytes(a,b,c) bytes of device memory, 16-byte
 *     aligned), a second kernel adds them in a fixed order.  No atomics: the same volume gives the same bits on every run.
 *     16-byte loads where c % 4 == 0 and vol is 16-byte aligned, scalar loads otherwise.  Any a, b, c >= 1.
 *   mpg_volume_planes_gray8: the planes of the slice loop (multipassGAN-out.py:592-604).  For t in [0, n_idx) the plane of
 *     vol at index idx[t] (HOST memory) of `axis` (0..2), its two remaining axes in array order, or swapped when
 *     `transposed`, as 8-bit grey into gray[t] (device memory).  mean (device memory, n_idx floats, may be NULL): the fp32
 *     mean of the unquantised plane, from a sum in a fixed order (the quantity :595,601 compare with 0.0001).
 *   mpg_gray8: save_img's quantisation (multipassGAN-out.py:204-206) of n floats: uint8(clip(v * 255, 0, 255)), a float32
 *     product, truncated.  mpg_volume_planes_gray8 applies the same. */
size_t mpg_volume_projections_ws_bytes(int a, int b, int c);
int mpg_volume_projections(mpg_stream_t stream, const float* vol, int a, int b, int c, float divisor, float* p0,
                           float* p1, float* p2, void* ws);
int mpg_volume_planes_gray8(mpg_stream_t stream, const float* vol, int a, int b, int c, int axis, const int* idx,
                            int n_idx, int transposed, unsigned char* gray, float* mean);
int mpg_gray8(mpg_stream_t stream, const float* img, size_t n, unsigned char* out);

#ifdef __cplusplus
}
#endif
#endif /* MPGAN_H */
