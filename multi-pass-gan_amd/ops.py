"""Operator layer: thin, checked wrappers of the C ABI on PyTorch-ROCm tensors.

PyTorch is used for device memory and streams only; every function here
enqueues hand-written HIP kernels from libmpgan_hip.so on torch's current
stream.  Tensors are NHWC float32 on the GPU.
"""
import ctypes

import torch

from . import _lib
from ._lib import G8_F16, PREC_F16F6, PREC_F16X1, PREC_F16X3  # noqa: F401  (re-exported)

DEFAULT_PREC = PREC_F16X3     # kernel-level default (weight packing, generic sessions, training)
# what the inference drivers and multipass.Generator run unless told otherwise (`prec` parameter): held to
# 5e-4 relative L2 of the oracle at the full C2 / C4 sizes by tests/test_fullsize_gpu.py (north_star: 1e-3)
INFERENCE_PREC = PREC_F16F6
# contractions up to this length run as MPG_PREC_F16X3 inside an F16F6 session (session._match_fused)
F16F6_MIN_K = 256


def parse_prec(v):
    """`prec` parameter of the GAN/ drivers: 2 / "f16f6" (default), 3 / "f16x3" (fp32-grade), 1 / "f16x1" """
    names = {"f16f6": PREC_F16F6, "f16x3": PREC_F16X3, "f16x1": PREC_F16X1, "fp32": PREC_F16X3}
    s = str(v).strip().lower()
    if s in names:
        return names[s]
    try:
        p = int(s)
    except ValueError:
        p = -1
    if p not in (PREC_F16X1, PREC_F16F6, PREC_F16X3):
        raise _lib.MpgError("prec %r: expected 1 (f16x1), 2 (f16f6) or 3 (f16x3)" % (v,))
    return p


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name="tensor", dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MpgError("%s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != dtype:
        raise _lib.MpgError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.MpgError("%s must be contiguous" % name)
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class G8(object):
    """A "G8" activation tensor (include/mpgan.h): [N][ceil(C/8)][2 planes hi, lo][H][W][8 x fp16]."""

    __slots__ = ("buf", "n", "h", "w", "c", "flavour")

    def __init__(self, buf, n, h, w, c, flavour=G8_F16):
        self.buf, self.n, self.h, self.w, self.c, self.flavour = buf, n, h, w, c, flavour

    @property
    def groups(self):
        return (self.c + 7) // 8

    def data_ptr(self):
        return self.buf.data_ptr()

    @staticmethod
    def empty(n, h, w, c, device, flavour=G8_F16):
        buf = torch.empty((n, (c + 7) // 8, 2, h, w, 8), dtype=torch.float16, device=device)
        return G8(buf, n, h, w, c, flavour)


def f6_available(cout, segments=()):
    """MPG_PREC_F16F6 is built for every output width of the fused convolution (1..128); a segment (kh, kw, cin)
    whose LDS images do not fit at that width (7x7 with four cout tiles) answers 0 to the pack-size query"""
    if not 1 <= cout <= 128:
        return False
    lib = _lib.load()
    return all(lib.mpg_conv_pack_size(kh, kw, cin, cout, PREC_F16F6) > 0 for (kh, kw, cin) in segments)


def absmax(x):
    """device scalar max |x| (mpg_absmax)"""
    lib = _lib.load()
    x = _dev(x.contiguous(), "x")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _lib.check(lib.mpg_absmax(_stream(), _ptr(x), x.numel(), _ptr(out)), "mpg_absmax")
    return out


def to_g8(x, c_off=0, cin=None, flavour=G8_F16, amax=None):
    """fp32 NHWC x[..., c_off:c_off+cin] -> G8 (mpg_f32_to_g8)"""
    lib = _lib.load()
    x = _dev(x, "x")
    if x.dim() != 4:
        raise _lib.MpgError("to_g8: expected NHWC, got %s" % (tuple(x.shape),))
    n, h, w, c = x.shape
    cin = c - c_off if cin is None else cin
    g = G8.empty(n, h, w, cin, x.device, flavour)
    if x.numel():
        _lib.check(lib.mpg_f32_to_g8_scaled(_stream(), _ptr(x), n, h, w, c, c_off, cin, flavour, _ptr(amax), _ptr(g.buf)),
                   "mpg_f32_to_g8")
    return g


def from_g8(g):
    """G8 -> fp32 NHWC (mpg_g8_to_f32)"""
    lib = _lib.load()
    if g.flavour != G8_F16:
        raise _lib.MpgError("from_g8: only the fp16 hi/lo flavour converts back to fp32")
    y = torch.empty((g.n, g.h, g.w, g.c), dtype=torch.float32, device=g.buf.device)
    _lib.check(lib.mpg_g8_to_f32(_stream(), _ptr(g.buf), g.n, g.h, g.w, g.c, _ptr(y)), "mpg_g8_to_f32")
    return y


class PackedWeights(object):
    """Weights of one conv segment in MFMA fragment order (mpg_conv_pack_weights)."""

    __slots__ = ("buf", "kh", "kw", "cin", "cout", "prec")

    def __init__(self, buf, kh, kw, cin, cout, prec):
        self.buf, self.kh, self.kw, self.cin, self.cout, self.prec = buf, kh, kw, cin, cout, prec


def pack_conv_weights(w_hwio, wscale=1.0, cout_scale=None, c_off=0, cin=None, prec=DEFAULT_PREC):
    """Pack W[kh,kw,cin_total,cout] channels [c_off, c_off+cin) times wscale
    (GAN.weight_variable, GAN.py:664-668) times an optional per-channel scale
    (folded batch norm, GAN.py:110)."""
    lib = _lib.load()
    w = _dev(w_hwio, "w_hwio")
    kh, kw, cin_total, cout = w.shape
    cin = cin_total - c_off if cin is None else cin
    nbytes = lib.mpg_conv_pack_size(kh, kw, cin, cout, prec)
    if nbytes == 0:
        raise _lib.MpgError("mpg_conv_pack_size: unsupported conv %dx%d %d->%d" % (kh, kw, cin, cout))
    buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    cs = _dev(cout_scale, "cout_scale") if cout_scale is not None else None
    rc = lib.mpg_conv_pack_weights(_stream(), _ptr(w), kh, kw, cin_total, c_off, cin, cout, float(wscale), _ptr(cs),
                                   prec, _ptr(buf), nbytes)
    _lib.check(rc, "mpg_conv_pack_weights")
    return PackedWeights(buf, kh, kw, cin, cout, prec)


class Segment(object):
    """One K-slice of a fused convolution: G8 source (an fp32 NHWC tensor is converted on the
    fly), first channel group consumed, packed weights, fused nearest upsample (up_x_only=1: of the columns alone,
    the source is [N, H, W >> up_log2])."""

    __slots__ = ("x", "packed", "g_off", "up_log2", "up_x_only", "pad_hi")

    def __init__(self, x, packed, c_off=0, up_log2=0, pad_hi=0, up_x_only=0):
        self.pad_hi = int(pad_hi)
        self.up_x_only = int(up_x_only)
        if isinstance(x, torch.Tensor):
            x = to_g8(x, c_off, packed.cin)
            c_off = 0
        if c_off % 8:
            raise _lib.MpgError("Segment: channel offset %d of a G8 source is not a multiple of 8" % c_off)
        self.x, self.packed, self.g_off, self.up_log2 = x, packed, c_off // 8, up_log2


def _conv_desc(segments, out_hw, bias, act, leak):
    """the ConvDesc of a fused-convolution launch without its outputs: the checked segments, bias (a contiguous fp32
    GPU tensor of cout entries), activation and precision"""
    if not 1 <= len(segments) <= _lib.MAX_SEG:
        raise _lib.MpgError("conv2d_fused: %d segments (1..%d supported)" % (len(segments), _lib.MAX_SEG))
    p0 = segments[0].packed
    h, w = out_hw
    n = segments[0].x.n
    d = _lib.ConvDesc()
    d.n, d.h, d.w, d.cout, d.nseg = n, h, w, p0.cout, len(segments)
    for i, s in enumerate(segments):
        g8, pk = s.x, s.packed
        if (pk.cout, pk.prec) != (p0.cout, p0.prec):
            raise _lib.MpgError("conv2d_fused: segments packed with different cout/prec")
        if g8.flavour != G8_F16:
            raise _lib.MpgError("conv2d_fused: segment %d input has G8 flavour %d, every precision reads flavour %d"
                                % (i, g8.flavour, G8_F16))
        if g8.n != n or g8.h << (0 if s.up_x_only else s.up_log2) != h or g8.w << s.up_log2 != w:
            raise _lib.MpgError("conv2d_fused: segment %d input %dx%dx%d does not match output %dx%dx%d (up 2^%d%s)"
                                % (i, g8.n, g8.h, g8.w, n, h, w, s.up_log2, " of the columns" if s.up_x_only else ""))
        if s.g_off * 8 + pk.cin > g8.c:
            raise _lib.MpgError("conv2d_fused: segment %d channel window [%d,%d) exceeds %d"
                                % (i, s.g_off * 8, s.g_off * 8 + pk.cin, g8.c))
        g = d.seg[i]
        g.x, g.wpack = g8.buf.data_ptr(), pk.buf.data_ptr()
        g.cin, g.cgroups, g.g_off = pk.cin, g8.groups, s.g_off
        g.kh, g.kw, g.up_log2, g.up_x_only = pk.kh, pk.kw, s.up_log2, s.up_x_only
        g.pad_hi = s.pad_hi
    if bias is not None:
        if bias.numel() != p0.cout:
            raise _lib.MpgError("conv2d_fused: bias has %d entries, cout is %d" % (bias.numel(), p0.cout))
        d.bias = bias.data_ptr()
    d.act, d.leak = _lib.act_id(act), leak
    d.prec = p0.prec
    return d


def _alloc_outputs(shape, dev, want_f32, want_g8, out, what):
    """the outputs of a launch of NHWC `shape`: (fp32 tensor or None, G8 or None, [those requested, in that order]).
    `out`, a contiguous fp32 GPU tensor of exactly that shape, receives the fp32 result (and asks for it)."""
    y = y8 = None
    if out is not None:
        y = _dev(out, "out")
        if tuple(y.shape) != tuple(shape):
            raise _lib.MpgError("%s: out has shape %s" % (what, tuple(y.shape)))
    elif want_f32:
        y = torch.empty(shape, dtype=torch.float32, device=dev)
    if want_g8:
        y8 = G8.empty(*shape, dev, G8_F16)
    outs = [o for o in (y, y8) if o is not None]
    if not outs:
        raise _lib.MpgError("%s: no output requested" % what)
    return y, y8, outs


def _checked_post_add(post_add, coff, shape, what):
    """post_add as the epilogue reads it: a contiguous fp32 NHWC GPU tensor over the pixels of the output `shape` that
    holds channels [coff, coff + shape[3])"""
    pa = _dev(post_add, "post_add")
    if pa.dim() != 4 or tuple(pa.shape[:3]) != tuple(shape[:3]) or coff + shape[3] > pa.shape[3]:
        raise _lib.MpgError("%s: post_add %s does not match output" % (what, tuple(pa.shape)))
    return pa


def conv2d_fused(segments, out_hw, bias=None, act=None, leak=0.2, pixel_norm=False, pn_eps=1e-8,
                 post_add=None, post_add_coff=0, out=None, want_f32=True, want_g8=False, reserved=0,
                 in_amax=None):
    """y = post(act(sum_s conv_SAME(up_s(x_s), W_s) + bias)) [+ post_add]; see include/mpgan.h.
    Returns the requested outputs in the order (fp32 NHWC, G8): a single object when one is requested,
    else a tuple."""
    lib = _lib.load()
    d = _conv_desc(segments, out_hw, _dev(bias, "bias") if bias is not None else None, act, leak)
    shape = (d.n, d.h, d.w, d.cout)
    d.pixel_norm, d.pn_eps = int(bool(pixel_norm)), pn_eps
    if post_add is not None:
        pa = _checked_post_add(post_add, post_add_coff, shape, "conv2d_fused")
        d.post_add, d.post_add_stride, d.post_add_coff = pa.data_ptr(), pa.shape[3], post_add_coff
    y, y8, outs = _alloc_outputs(shape, segments[0].x.buf.device, want_f32, want_g8, out, "conv2d_fused")
    d.y, d.y_g8 = _ptr(y), _ptr(y8)
    d.reserved = reserved
    if in_amax is not None:     # the inputs were converted with to_g8(..., amax=in_amax): undo the power-of-two scale
        d.in_amax = _dev(in_amax, "in_amax").data_ptr()
    _lib.check(lib.mpg_conv2d_fused(_stream(), ctypes.byref(d)), "mpg_conv2d_fused")
    return outs[0] if len(outs) == 1 else tuple(outs)


def _launch_windows(what, entry, lead_args, chunks, out_hw, c_total, out_c, bias, act, leak, want_f32, want_g8, out,
                    post_add=None, post_add_coff=0, g8_only=False):
    """What conv2d_fused_wide and conv2d_fused_d2s share: the output windows `chunks` = [(segments, co_off), ...] of one
    c_total-channel convolution (each window's weights packed for its own output channels) as one launch each of the
    library's `entry`(stream, desc, *lead_args, c_total, co_off) into the same tensors of out_c = (rows and columns per
    input pixel, channels).  Checked once: the windows cover channels 0..c_total, the bias has c_total entries, the
    outputs; per window the bias is sliced and post_add read at the window's channels.  g8_only: the windows write the
    G8 tensor alone, which exists then whether it was asked for or not.  Returns (fp32 or None, G8 or None, [those
    requested]) like _alloc_outputs."""
    lib = _lib.load()
    if not chunks:
        raise _lib.MpgError("%s: no chunks" % what)
    co = 0
    for segments, co_off in sorted(chunks, key=lambda ch: ch[1]):
        if co_off != co:
            break
        co += segments[0].packed.cout
    if co != c_total:
        raise _lib.MpgError("%s: the chunks do not cover channels 0..%d once" % (what, c_total))
    if bias is not None:
        bias = _dev(bias, "bias")
        if bias.numel() != c_total:
            raise _lib.MpgError("%s: bias has %d entries, expected %d" % (what, bias.numel(), c_total))
    x0 = chunks[0][0][0].x
    shape = (x0.n, out_c[0] * out_hw[0], out_c[0] * out_hw[1], out_c[1])
    y, y8, outs = _alloc_outputs(shape, x0.buf.device, want_f32, want_g8, out, what)
    pa = _checked_post_add(post_add, post_add_coff, shape, what) if post_add is not None else None
    if g8_only and y8 is None:
        y8 = G8.empty(*shape, x0.buf.device, G8_F16)
    for segments, co_off in chunks:
        cw = segments[0].packed.cout
        d = _conv_desc(segments, out_hw, bias[co_off:co_off + cw].contiguous() if bias is not None else None, act, leak)
        if pa is not None:
            d.post_add, d.post_add_stride, d.post_add_coff = pa.data_ptr(), pa.shape[3], post_add_coff + co_off
        d.y, d.y_g8 = _ptr(None if g8_only else y), _ptr(y8)
        _lib.check(getattr(lib, entry)(_stream(), ctypes.byref(d), *lead_args, c_total, co_off), entry)
    return y, y8, outs


def conv2d_fused_d2s(chunks, out_hw, c_total, bias=None, act=None, leak=0.2, out=None, want_f32=True, want_g8=False):
    """GAN.pixel_shuffle (GAN.py:554-560) with the shuffle in the store: depth_to_space(conv(...) + bias, 2) of a
    c_total-channel convolution given as 128-wide output chunks [(segments, co_off), ...] (each chunk's weights packed
    for its own output channels), one mpg_conv2d_fused_d2s launch per chunk into the same tensors.  Returns fp32
    [N, 2H, 2W, c_total/4] and / or G8, like conv2d_fused.  Raises MpgError where the launch refuses (G8 output with
    c_total/4 not a multiple of 8): the caller then runs conv2d_fused and depth_to_space."""
    if c_total % 4 or not chunks:
        raise _lib.MpgError("conv2d_fused_d2s: %d channels are not a multiple of 4" % c_total)
    if want_g8 and (c_total // 4) % 8:
        raise _lib.MpgError("conv2d_fused_d2s: G8 output of %d channels (not a multiple of 8)" % (c_total // 4))
    outs = _launch_windows("conv2d_fused_d2s", "mpg_conv2d_fused_d2s", (2,), chunks, out_hw, c_total, (2, c_total // 4), bias,
                           act, leak, want_f32, want_g8, out)[2]
    return outs[0] if len(outs) == 1 else tuple(outs)


WIDE_MAX_COUT = 512


def wide_chunks(c_total):
    """the output windows [(co_off, width), ...] a convolution of c_total > 128 outputs runs as: as few launches as 128
    outputs each allow, of equal width rounded up to a G8 group.  No window is narrower than 57 channels (136 outputs run
    as 72 + 64, not 128 + 8), so none falls to the small-channel kernel, which has no window store."""
    k = -(-c_total // 128)
    width = -(-c_total // (8 * k)) * 8
    return [(co, min(width, c_total - co)) for co in range(0, c_total, width)]


def pixel_norm_g8(g, eps=1e-8, want_f32=False, out=None):
    """GAN.pixel_norm of the G8 tensor `g` in place (mpg_pixel_norm_g8); with want_f32 / out the fp32 NHWC result too,
    which is returned (else g)"""
    lib = _lib.load()
    if g.flavour != G8_F16:
        raise _lib.MpgError("pixel_norm_g8: only the fp16 hi/lo flavour")
    y = None
    if want_f32 or out is not None:
        y, _, _ = _alloc_outputs((g.n, g.h, g.w, g.c), g.buf.device, True, False, out, "pixel_norm_g8")
    _lib.check(lib.mpg_pixel_norm_g8(_stream(), _ptr(g.buf), g.n, g.h, g.w, g.c, eps, _ptr(y)), "mpg_pixel_norm_g8")
    return y if y is not None else g


def conv2d_fused_wide(chunks, out_hw, c_total, bias=None, act=None, leak=0.2, pixel_norm=False, pn_eps=1e-8,
                      post_add=None, post_add_coff=0, want_f32=True, want_g8=False, out=None):
    """conv2d_fused for c_total > 128 output channels, given as output windows [(segments, co_off), ...] (each window's
    weights packed for its own <= 128 output channels, see wide_chunks): one mpg_conv2d_fused_window launch per window
    into the same tensors, with the bias sliced per window and post_add read at the window's channels.  The reference
    applies the activation, then the pixel norm (GAN.py:472-474 behind the layer), which needs every channel of a pixel:
    the windows then write G8 only (the working form, also when only fp32 is wanted) and mpg_pixel_norm_g8 runs last,
    rewriting that tensor in place and writing the fp32 result.  Returns like conv2d_fused."""
    if post_add is not None and pixel_norm:
        raise _lib.MpgError("conv2d_fused_wide: post_add follows the pixel norm, which runs behind the window launches")
    y, y8, outs = _launch_windows("conv2d_fused_wide", "mpg_conv2d_fused_window", (), chunks, out_hw, c_total, (1, c_total),
                                  bias, act, leak, want_f32, want_g8, out, post_add, post_add_coff, g8_only=bool(pixel_norm))
    if pixel_norm:
        _lib.check(_lib.load().mpg_pixel_norm_g8(_stream(), _ptr(y8.buf), y8.n, y8.h, y8.w, c_total, pn_eps, _ptr(y)),
                   "mpg_pixel_norm_g8")
    return outs[0] if len(outs) == 1 else tuple(outs)


def space_to_depth(x, r):
    """the adjoint of depth_to_space (mpg_space_to_depth): [N,H,W,C] -> [N,H/r,W/r,C*r^2]"""
    lib = _lib.load()
    x = _dev(x, "x")
    n, h, w, c = x.shape
    if h % r or w % r:
        raise _lib.MpgError("space_to_depth: %dx%d is not a multiple of %d" % (h, w, r))
    y = torch.empty((n, h // r, w // r, c * r * r), dtype=torch.float32, device=x.device)
    _lib.check(lib.mpg_space_to_depth(_stream(), _ptr(x), n, h, w, c, r, _ptr(y)), "mpg_space_to_depth")
    return y


PAIR_MAX_CIN = 4


def small_pair_ok(cin, cmid, cout, ka, kb, ks=None, planner=False):
    """shapes mpg_conv2d_small_pair takes: <= 8 channels everywhere, odd filters up to 7x7, shortcut inside the input tile.
    planner=True: the shapes the launch planner fuses -- only inputs of <= 4 channels: the first convolution is recomputed
    on the halo of the second (x1.33 at 5x5 on 64x16 tiles), which one launch less pays for at 1 -> 2 -> 8 (26.8 against
    37.6 us per 8 slices of 256^2) and not at 8 -> 2 -> 1 (50.0 against 37.1 us; tools/probe_small.py)"""
    if not (1 <= cin <= 8 and 1 <= cmid <= 8 and 1 <= cout <= 8):
        return False
    if planner and cin > PAIR_MAX_CIN:
        return False
    for k in (ka, kb) + ((ks,) if ks is not None else ()):
        if k[0] % 2 == 0 or k[1] % 2 == 0 or max(k) > 7:
            return False
    return ks is None or (ks[0] <= ka[0] + kb[0] - 1 and ks[1] <= ka[1] + kb[1] - 1)


def conv2d_small_pair(x, c_off, up_log2, pk_a, pk_b, pk_s, out_hw, bias_a=None, act_a=None, leak_a=0.2, bias_b=None,
                      act_b=None, leak_b=0.2, want_f32=True, want_g8=False, out=None, up_x_only=0):
    """y = act_b(conv_b(act_a(conv_a(up(x)) + bias_a)) + conv_s(up(x)) + bias_b): a residual block of <= 8-channel
    convolutions as one launch (mpg_conv2d_small_pair); x: G8 (or fp32 NHWC, converted), pk_*: PackedWeights;
    up_x_only=1: the upsample repeats columns only (x is [N, H, W >> up_log2])."""
    lib = _lib.load()
    if isinstance(x, torch.Tensor):
        x = to_g8(x, c_off, pk_a.cin)
        c_off = 0
    if c_off % 8:
        raise _lib.MpgError("conv2d_small_pair: channel offset %d of a G8 source is not a multiple of 8" % c_off)
    h, w = out_hw
    if x.h << (0 if up_x_only else up_log2) != h or x.w << up_log2 != w:
        raise _lib.MpgError("conv2d_small_pair: input %dx%d does not match output %dx%d (up 2^%d%s)"
                            % (x.h, x.w, h, w, up_log2, " of the columns" if up_x_only else ""))
    if pk_b.cin != pk_a.cout or (pk_s is not None and (pk_s.cin != pk_a.cin or pk_s.cout != pk_b.cout)):
        raise _lib.MpgError("conv2d_small_pair: channel counts of the three convolutions do not chain")
    if len(set(p.prec for p in (pk_a, pk_b) + ((pk_s,) if pk_s is not None else ()))) != 1:
        raise _lib.MpgError("conv2d_small_pair: weights packed for different precisions")
    if c_off + pk_a.cin > x.c:
        raise _lib.MpgError("conv2d_small_pair: channel window exceeds the input")
    dev = x.buf.device
    d = _lib.SmallPairDesc()
    d.n, d.h, d.w = x.n, h, w
    d.x, d.cin, d.cgroups, d.g_off, d.up_log2 = x.buf.data_ptr(), pk_a.cin, x.groups, c_off // 8, up_log2
    d.up_x_only = int(up_x_only)          # the library refuses anything but 0 and 1
    d.wpack_a, d.kh_a, d.kw_a, d.cmid = pk_a.buf.data_ptr(), pk_a.kh, pk_a.kw, pk_a.cout
    d.wpack_b, d.kh_b, d.kw_b, d.cout = pk_b.buf.data_ptr(), pk_b.kh, pk_b.kw, pk_b.cout
    if pk_s is not None:
        d.wpack_s, d.kh_s, d.kw_s = pk_s.buf.data_ptr(), pk_s.kh, pk_s.kw
    if bias_a is not None:
        d.bias_a = _dev(bias_a, "bias_a").data_ptr()
    if bias_b is not None:
        d.bias_b = _dev(bias_b, "bias_b").data_ptr()
    d.act_a, d.leak_a, d.act_b, d.leak_b = _lib.act_id(act_a), leak_a, _lib.act_id(act_b), leak_b
    d.prec = pk_a.prec
    shape = (x.n, h, w, pk_b.cout)
    if not want_f32:
        out = None
    elif out is not None:       # any contiguous fp32 tensor of that many elements (the planner's destination buffers)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != x.n * h * w * pk_b.cout or out.device != dev:
            raise _lib.MpgError("conv2d_small_pair: `out` does not hold a contiguous fp32 [%d,%d,%d,%d]" % shape)
        out = out.view(shape)
    y, y8, outs = _alloc_outputs(shape, dev, want_f32, want_g8, out, "conv2d_small_pair")
    d.y, d.y_g8 = _ptr(y), _ptr(y8)
    _lib.check(lib.mpg_conv2d_small_pair(_stream(), ctypes.byref(d)), "mpg_conv2d_small_pair")
    return outs[0] if len(outs) == 1 else tuple(outs)


def conv2d_direct(x, w_hwio, stride=(1, 1), wscale=1.0, cout_scale=None, bias=None, act=None, leak=0.2):
    """fp32 vector-ALU convolution, any stride (tf.nn.conv2d SAME, GAN.py:686-691)."""
    lib = _lib.load()
    x = _dev(x, "x")
    w = _dev(w_hwio, "w_hwio")
    n, h, wd, cin = x.shape
    kh, kw, cin2, cout = w.shape
    if cin != cin2:
        raise _lib.MpgError("conv2d_direct: input has %d channels, weights expect %d" % (cin, cin2))
    sh, sw = stride
    oh, ow = -(-h // sh), -(-wd // sw)
    y = torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)
    cs = _dev(cout_scale, "cout_scale") if cout_scale is not None else None
    b = _dev(bias, "bias") if bias is not None else None
    rc = lib.mpg_conv2d_direct(_stream(), _ptr(x), n, h, wd, cin, _ptr(w), kh, kw, cout, sh, sw, float(wscale),
                               _ptr(cs), _ptr(b), _lib.act_id(act), leak, _ptr(y))
    _lib.check(rc, "mpg_conv2d_direct")
    return y


def depth_to_space(x, r):
    """tf.depth_to_space (GAN.pixel_shuffle, GAN.py:554-560): [N,H,W,C] -> [N,H*r,W*r,C/r^2]"""
    lib = _lib.load()
    x = _dev(x, "x")
    n, h, w, c = x.shape
    if c % (r * r):
        raise _lib.MpgError("depth_to_space: %d channels are not a multiple of %d^2" % (c, r))
    y = torch.empty((n, h * r, w * r, c // (r * r)), dtype=torch.float32, device=x.device)
    _lib.check(lib.mpg_depth_to_space(_stream(), _ptr(x), n, h, w, c, r, _ptr(y)), "mpg_depth_to_space")
    return y


def subpixel_filter(w_hwoi, stride):
    """The stride-s transposed convolution as ONE stride-1 SAME convolution with s*s*cout outputs followed by
    depth_to_space: output row s*q + p gathers x[q + e] * W[ky] for the taps ky with (p + pad - ky) = s*e, so each
    output phase p is a stride-1 correlation over the offsets e.  Returns V[K',K',cin,s*s*cout] (K' odd) in HWIO."""
    kh, kw, cout, cin = w_hwoi.shape
    s = int(stride)
    pad = [max(k - s, 0) // 2 for k in (kh, kw)]

    def taps(k, p0):
        out = []            # (phase, tap, offset e)
        for ph in range(s):
            for t in range(k):
                if (ph + p0 - t) % s == 0:
                    out.append((ph, t, (ph + p0 - t) // s))
        return out

    ty, tx = taps(kh, pad[0]), taps(kw, pad[1])
    ey = max([abs(e) for _, _, e in ty] + [0])
    ex = max([abs(e) for _, _, e in tx] + [0])
    v = torch.zeros((2 * ey + 1, 2 * ex + 1, cin, s * s * cout), dtype=w_hwoi.dtype, device=w_hwoi.device)
    for py, ky, dy in ty:
        for px, kx, dx in tx:
            c0 = (py * s + px) * cout
            v[ey + dy, ex + dx, :, c0:c0 + cout] = w_hwoi[ky, kx].t()
    return v


def conv2d_transpose(x, w_hwoi, stride=(1, 1), wscale=1.0, bias=None, act=None, leak=0.2, prec=None):
    """tf.nn.conv2d_transpose(x, W[kh,kw,cout,cin], [N, H*sh, W*sw, cout], strides, "SAME") + bias + act
    (GAN.deconvolutional_layer, GAN.py:566-619,703-708).  prec None: the fp32 vector-ALU kernel (any stride / filter).
    prec 1/2/3: the matrix cores -- stride 1 as the fused convolution with the mirrored filter, stride 2 as a fused
    convolution with the sub-pixel filter + depth_to_space; shapes that route cannot take fall back to the fp32 kernel."""
    lib = _lib.load()
    x = _dev(x, "x")
    w = _dev(w_hwoi, "w_hwoi")
    n, h, wd, cin = x.shape
    kh, kw, cout, cin2 = w.shape
    if cin != cin2:
        raise _lib.MpgError("conv2d_transpose: input has %d channels, filter expects %d" % (cin, cin2))
    sh, sw = stride
    b = _dev(bias, "bias") if bias is not None else None
    if prec is not None and sh == sw and sh in (1, 2):
        if sh == 1 and kh <= 7 and kw <= 7 and cout <= 128:
            v = w.flip(0, 1).permute(0, 1, 3, 2).contiguous()
            p = prec if f6_available(cout, [(kh, kw, cin)]) or prec != PREC_F16F6 else PREC_F16X3
            seg = Segment(x, pack_conv_weights(v, wscale=wscale, prec=p), pad_hi=1)
            return conv2d_fused([seg], (h, wd), bias=b, act=act, leak=leak)
        if sh == 2 and 4 * cout <= 128:
            v = subpixel_filter(w, 2)
            if v.shape[0] <= 7 and v.shape[1] <= 7:
                p = prec if f6_available(4 * cout, [(v.shape[0], v.shape[1], cin)]) or prec != PREC_F16F6 else PREC_F16X3
                seg = Segment(x, pack_conv_weights(v, wscale=wscale, prec=p))
                z = conv2d_fused([seg], (h, wd), bias=b.repeat(4) if b is not None else None, act=act, leak=leak)
                return depth_to_space(z, 2)
    y = torch.empty((n, h * sh, wd * sw, cout), dtype=torch.float32, device=x.device)
    rc = lib.mpg_conv2d_transpose(_stream(), _ptr(x), n, h, wd, cin, _ptr(w), kh, kw, cout, sh, sw, float(wscale), _ptr(b),
                                  _lib.act_id(act), leak, _ptr(y))
    _lib.check(rc, "mpg_conv2d_transpose")
    return y


def _resize(fn_name, x, oh, ow):
    lib = _lib.load()
    x = _dev(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    _lib.check(getattr(lib, fn_name)(_stream(), _ptr(x), n, h, w, c, _ptr(y), oh, ow), fn_name)
    return y


def resize_nearest(x, oh, ow):
    return _resize("mpg_resize_nearest", x, oh, ow)


def resize_bilinear(x, oh, ow):
    return _resize("mpg_resize_bilinear", x, oh, ow)


def resize_bicubic(x, oh, ow):
    return _resize("mpg_resize_bicubic", x, oh, ow)


def resize_images(x, oh, ow, method):
    """tf.image.resize_images method ids (GAN.py:541): 0 bilinear, 1 nearest, 2 bicubic."""
    if method == 0:
        return resize_bilinear(x, oh, ow)
    if method == 1:
        return resize_nearest(x, oh, ow)
    if method == 2:
        return resize_bicubic(x, oh, ow)
    raise _lib.MpgError("resize method %r not supported" % (method,))


def bicubic_cols_add_ok(src_shape, c_src, f):
    """does mpg_bicubic_cols_add take channel c_src of a [n, h, wl, c] tensor at column factor f?  (the planner asks before
    it emits the kernel; what it refuses runs as slice, resize_bicubic and add)"""
    return (len(src_shape) == 4 and 0 <= c_src < src_shape[3] and 1 <= f <= 64 and f & (f - 1) == 0
            and src_shape[2] * f < 2 ** 31)


def bicubic_cols_add(src, c_src, f, dens, out=None):
    """dens [n,h,wl*f,1] + the bicubic resize of src[n,h,wl,c][..., c_src] along the columns by f (mpg_bicubic_cols_add: the
    residual of the upsampling_mode 0 growing generator, multipassGAN-8x.py:720-721).  out: where the result goes (fp32,
    contiguous, as many elements as dens, not dens itself), else a new tensor."""
    lib = _lib.load()
    src, dens = _dev(src, "src"), _dev(dens, "dens")
    if src.dim() != 4:
        raise _lib.MpgError("bicubic_cols_add: expected NHWC src, got %s" % (tuple(src.shape),))
    n, h, wl, c = src.shape
    if dens.numel() != n * h * wl * f:
        raise _lib.MpgError("bicubic_cols_add: dens %s is not [%d,%d,%d,1]" % (tuple(dens.shape), n, h, wl * f))
    if out is None:
        out = torch.empty((n, h, wl * f, 1), dtype=torch.float32, device=src.device)
    elif _dev(out, "out").numel() != dens.numel():
        raise _lib.MpgError("bicubic_cols_add: out %s does not match dens %s" % (tuple(out.shape), tuple(dens.shape)))
    _lib.check(lib.mpg_bicubic_cols_add(_stream(), _ptr(src), n, h, wl, c, int(c_src), int(f), _ptr(dens), _ptr(out)),
               "mpg_bicubic_cols_add")
    return out.view(n, h, wl * f, 1)


def max_pool(x, k=2, s=2, want_arg=False):
    """tf.nn.max_pool(x, k, s, VALID) (GAN.py:152-159); with want_arg also the uint8 window positions of the maxima"""
    lib = _lib.load()
    x = _dev(x, "x")
    n, h, w, c = x.shape
    if h < k or w < k:
        raise _lib.MpgError("max_pool: window %d does not fit %dx%d" % (k, h, w))
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    arg = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=x.device) if want_arg else None
    _lib.check(lib.mpg_max_pool(_stream(), _ptr(x), n, h, w, c, k, s, _ptr(y), _ptr(arg) if want_arg else None), "mpg_max_pool")
    return (y, arg) if want_arg else y


def avg_pool2(x):
    lib = _lib.load()
    x = _dev(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    _lib.check(lib.mpg_avg_pool2(_stream(), _ptr(x), n, h, w, c, _ptr(y)), "mpg_avg_pool2")
    return y


def pixel_norm(x, eps=1e-8):
    lib = _lib.load()
    x = _dev(x, "x")
    c = x.shape[-1]
    y = torch.empty_like(x)
    _lib.check(lib.mpg_pixel_norm(_stream(), _ptr(x), x.numel() // c, c, eps, _ptr(y)), "mpg_pixel_norm")
    return y


def minibatch_stddev(x, group_size=4):
    """GAN.minibatch_stddev_layer (GAN.py:476-488): [N,H,W,C] -> [N,H,W,C+1]"""
    lib = _lib.load()
    x = _dev(x, "x")
    n, h, w, c = x.shape
    g = min(group_size, n)
    stat = torch.empty((n // g,), dtype=torch.float32, device=x.device)
    y = torch.empty((n, h, w, c + 1), dtype=torch.float32, device=x.device)
    _lib.check(lib.mpg_minibatch_stddev(_stream(), _ptr(x), n, h, w, c, group_size, _ptr(stat), _ptr(y)), "mpg_minibatch_stddev")
    return y


def add_act(a, b=None, act=None, leak=0.2):
    lib = _lib.load()
    a = _dev(a, "a")
    if b is not None:
        b = _dev(b, "b")
        if b.shape != a.shape:
            raise _lib.MpgError("add_act: shapes differ %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    y = torch.empty_like(a)
    _lib.check(lib.mpg_add_act(_stream(), _ptr(a), _ptr(b), a.numel(), _lib.act_id(act), leak, _ptr(y)), "mpg_add_act")
    return y


def axis_zoom_linear(v, axis, factor):
    """scipy.ndimage.zoom(v, factor on `axis`, order=1) (multipassGAN-out.py:421)."""
    lib = _lib.load()
    v = _dev(v, "v")
    n = v.shape[axis]
    big = int(round(n * factor))
    outer = 1
    for d in v.shape[:axis]:
        outer *= d
    inner = 1
    for d in v.shape[axis + 1:]:
        inner *= d
    shape = list(v.shape)
    shape[axis] = big
    out = torch.empty(shape, dtype=torch.float32, device=v.device)
    if v.numel() == 0:
        return out
    _lib.check(lib.mpg_axis_zoom_linear(_stream(), _ptr(v), outer, n, inner, _ptr(out), big), "mpg_axis_zoom_linear")
    return out


def volume_transpose(v, perm, chan_map=None, cutoff=0.0):
    """numpy.transpose of [d0,d1,d2(,c)] by `perm` (3 axes) with optional channel
    permutation and cutoff (multipassGAN-out.py:459,472-475,614)."""
    lib = _lib.load()
    v = _dev(v, "v")
    if v.dim() == 3:
        d0, d1, d2 = v.shape
        c = 1
        squeeze = True
    elif v.dim() == 4:
        d0, d1, d2, c = v.shape
        squeeze = False
    else:
        raise _lib.MpgError("volume_transpose: expected a 3D or 4D tensor, got %s" % (tuple(v.shape),))
    perm = [int(p) for p in perm]
    if sorted(perm) != [0, 1, 2]:
        raise _lib.MpgError("volume_transpose: perm %r is not a permutation of (0,1,2)" % (perm,))
    dims = (d0, d1, d2)
    oshape = [dims[perm[0]], dims[perm[1]], dims[perm[2]]] + ([] if squeeze else [c])
    out = torch.empty(oshape, dtype=torch.float32, device=v.device)
    if v.numel() == 0:
        return out
    p_arr = (ctypes.c_int * 3)(*perm)
    cm = None
    if chan_map is not None:
        if len(chan_map) != c:
            raise _lib.MpgError("volume_transpose: chan_map has %d entries for %d channels" % (len(chan_map), c))
        cm = (ctypes.c_int * c)(*[int(k) for k in chan_map])
    rc = lib.mpg_volume_transpose(_stream(), _ptr(v), d0, d1, d2, c, p_arr, cm, float(cutoff), _ptr(out))
    _lib.check(rc, "mpg_volume_transpose")
    return out


def add_adjacent(x, s_off=0, s_cnt=None):
    """add_adj_idcs channels for slices [s_off, s_off+s_cnt) of x [S,H,W,C] (multipassGAN-out.py:423-436)."""
    lib = _lib.load()
    x = _dev(x, "x")
    s, h, w, c = x.shape
    s_cnt = s - s_off if s_cnt is None else s_cnt
    out = torch.empty((s_cnt, h, w, c + 2), dtype=torch.float32, device=x.device)
    _lib.check(lib.mpg_add_adjacent(_stream(), _ptr(x), s, h * w, c, s_off, s_cnt, _ptr(out)), "mpg_add_adjacent")
    return out


def channel_gather(a, b, cmap, scales=None, scales2=None):
    """out[..., j] = (cat(a, b)[..., cmap[j]] * scales[j]) * scales2[j] in one pass (mpg_channel_gather): the slice / scale /
    concat steps of the velocity channels between the passes (multipassGAN-4x.py:278-283, 1113-1119)"""
    lib = _lib.load()
    a = _dev(a.contiguous(), "a")
    ca, cb = a.shape[-1], 0
    if b is not None:
        b = _dev(b.contiguous(), "b")
        cb = b.shape[-1]
        if tuple(b.shape[:-1]) != tuple(a.shape[:-1]):
            raise _lib.MpgError("channel_gather: %s and %s differ outside the channel axis" % (tuple(a.shape), tuple(b.shape)))
    n = len(cmap)
    npix = a.numel() // ca
    out = torch.empty(tuple(a.shape[:-1]) + (n,), dtype=torch.float32, device=a.device)
    m = (ctypes.c_int * n)(*[int(c) for c in cmap])
    sc = (ctypes.c_float * n)(*[float(x) for x in (scales if scales is not None else [1.0] * n)])
    sc2 = (ctypes.c_float * n)(*[float(x) for x in (scales2 if scales2 is not None else [1.0] * n)])
    _lib.check(lib.mpg_channel_gather(_stream(), _ptr(a), ca, _ptr(b), cb, npix, m, sc, sc2, n, _ptr(out)), "mpg_channel_gather")
    return out


def vorticity_append(x):
    """[..., h, w, C] -> [..., h, w, C + 3]: the input next to the three vorticity channels of useVorticities
    (mpg_vorticity_append: addVorticity of multipassGAN-8x.py:1440-1446, 2D branch as written).  Any leading dimensions,
    e.g. [B, 1, h, w, C]; every [h, w] slice is a stencil of its own."""
    lib = _lib.load()
    x = _dev(x, "x")
    if x.dim() < 3:
        raise _lib.MpgError("vorticity_append: x %s has no [h, w, C] at its end" % (tuple(x.shape),))
    h, w, c = (int(d) for d in x.shape[-3:])
    n = x.numel() // max(h * w * c, 1)
    out = torch.empty(tuple(x.shape[:-1]) + (c + 3,), dtype=torch.float32, device=x.device)
    _lib.check(lib.mpg_vorticity_append(_stream(), _ptr(x), n, h, w, c, _ptr(out)), "mpg_vorticity_append")
    return out


def cutoff(v, thr=0.0005, out=None):
    """v[v < thr] = 0 (multipassGAN-4x.py:1156-1157)."""
    lib = _lib.load()
    v = _dev(v, "v")
    out = torch.empty_like(v) if out is None else out
    _lib.check(lib.mpg_cutoff(_stream(), _ptr(v), v.numel(), thr, _ptr(out)), "mpg_cutoff")
    return out


# ---------------------------------------------------------------- device codec of the .uni writer (tools_wscale/uniio.py:91-123)
DEFLATE_UNIT, DEFLATE_SLOT, DEFLATE_SLAB = _lib.DEFLATE_UNIT, _lib.DEFLATE_SLOT, _lib.DEFLATE_SLAB


def deflate_ws_bytes(n_bytes):
    """bytes of slot workspace that deflate_encode needs for n_bytes of payload"""
    return int(_lib.load().mpg_deflate_ws_bytes(int(n_bytes)))


def deflate_encode(src, slots=None, sizes=None, crcs=None, dynamic=False):
    """Deflate the bytes of `src` (contiguous float32 GPU tensor, at most DEFLATE_SLAB bytes, 16-byte aligned) in units
    of DEFLATE_UNIT bytes -> (slots uint8 [units * DEFLATE_SLOT], sizes int32 [units], crcs int32 [units]): unit u's
    raw DEFLATE stream is slots[u * DEFLATE_SLOT:][:sizes[u]], crcs[u] (read as uint32) the CRC-32 of its input.
    dynamic: a Huffman code per unit (mpg_deflate_encode_dynamic) instead of the fixed one; same workspace."""
    lib = _lib.load()
    src = _dev(src, "src")
    n_bytes = src.numel() * 4
    units = (n_bytes + DEFLATE_UNIT - 1) // DEFLATE_UNIT
    if slots is None:
        slots = torch.empty(units * DEFLATE_SLOT, dtype=torch.uint8, device=src.device)
    if sizes is None:
        sizes = torch.empty(units, dtype=torch.int32, device=src.device)
    if crcs is None:
        crcs = torch.empty(units, dtype=torch.int32, device=src.device)
    _dev(slots, "slots", torch.uint8), _dev(sizes, "sizes", torch.int32), _dev(crcs, "crcs", torch.int32)
    if slots.numel() < units * DEFLATE_SLOT or sizes.numel() < units or crcs.numel() < units:
        raise _lib.MpgError("deflate_encode: workspace too small for %d units" % units)
    name = "mpg_deflate_encode_dynamic" if dynamic else "mpg_deflate_encode"
    _lib.check(getattr(lib, name)(_stream(), _ptr(src), n_bytes, _ptr(slots), _ptr(sizes), _ptr(crcs)), name)
    return slots, sizes, crcs


def deflate_compact(slots, sizes, units, out=None):
    """the unit streams of deflate_encode, back to back: out[sum(sizes[:u]):][:sizes[u]] = slot u"""
    lib = _lib.load()
    _dev(slots, "slots", torch.uint8), _dev(sizes, "sizes", torch.int32)
    units = int(units)
    if slots.numel() < units * DEFLATE_SLOT or sizes.numel() < units:
        raise _lib.MpgError("deflate_compact: %d units exceed the workspace" % units)
    if out is None:
        out = torch.empty(units * DEFLATE_SLOT, dtype=torch.uint8, device=slots.device)
    _dev(out, "out", torch.uint8)
    _lib.check(lib.mpg_deflate_compact(_stream(), _ptr(slots), _ptr(sizes), units, _ptr(out), out.numel()), "mpg_deflate_compact")
    return out


def inflate_units(packed, offsets, sizes, n_bytes, out=None):
    """Decode the unit streams of the device .uni codecs on the GPU (tools_wscale/uniio.py:81-88 reads with gzip): unit u
    is the sizes[u] bytes at packed[offsets[u]:] (packed: uint8 GPU tensor; offsets, sizes: host sequences, one entry per
    DEFLATE_UNIT of the n_bytes of output) -> (out uint8 [n_bytes], crcs int32 [units], status int32 [units]): crcs[u]
    (read as uint32) is the CRC-32 of unit u's bytes, status[u] 0 = decoded, 1 = outside the writer's token language,
    2 = corrupt.  Streams that leave `packed` are refused before anything is launched."""
    import numpy as np
    lib = _lib.load()
    packed = _dev(packed, "packed", torch.uint8)
    n_bytes = int(n_bytes)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32).reshape(-1)
    units = (n_bytes + DEFLATE_UNIT - 1) // DEFLATE_UNIT
    if len(offsets) != units or len(sizes) != units:
        raise _lib.MpgError("inflate_units: %d offsets and %d sizes for %d units" % (len(offsets), len(sizes), units))
    packed_bytes = packed.numel()
    if units and int((offsets + sizes).max()) > packed_bytes:
        raise _lib.MpgError("inflate_units: a stream leaves the %d packed bytes" % packed_bytes)
    if packed_bytes % 16 or packed.data_ptr() % 16:                # the kernel reads whole 16-byte lines
        padded = torch.zeros((packed_bytes + 15) // 16 * 16, dtype=torch.uint8, device=packed.device)
        padded[:packed_bytes].copy_(packed)
        packed = padded
    if out is None:
        out = torch.empty(n_bytes, dtype=torch.uint8, device=packed.device)
    _dev(out, "out", torch.uint8)
    if out.numel() != n_bytes:
        raise _lib.MpgError("inflate_units: out holds %d bytes, not %d" % (out.numel(), n_bytes))
    crcs = torch.empty(units, dtype=torch.int32, device=packed.device)
    status = torch.empty(units, dtype=torch.int32, device=packed.device)
    _lib.check(lib.mpg_inflate_units(_stream(), _ptr(packed), packed.numel(), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                     sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), units, _ptr(out), n_bytes, _ptr(crcs),
                                     _ptr(status)), "mpg_inflate_units")
    return out, crcs, status


# ---------------------------------------------------------------- preview images of the inference drivers
def _volume3(vol, what):
    vol = _dev(vol, "vol")
    if vol.dim() != 3 or vol.numel() == 0:
        raise _lib.MpgError("%s: expected a non-empty [a, b, c] volume, got %s" % (what, tuple(vol.shape)))
    return vol, [int(d) for d in vol.shape]


def volume_projections(vol, divisor=80.0):
    """(sum over axis 0 [b,c], over axis 1 [a,c], over axis 2 [a,b]) of vol / divisor, from one read of the volume:
    np.sum(img, axis=0..2) of save_img_3d (multipassGAN-out.py:208-210)."""
    lib = _lib.load()
    vol, (a, b, c) = _volume3(vol, "volume_projections")
    p0 = torch.empty((b, c), dtype=torch.float32, device=vol.device)
    p1 = torch.empty((a, c), dtype=torch.float32, device=vol.device)
    p2 = torch.empty((a, b), dtype=torch.float32, device=vol.device)
    ws = torch.empty(int(lib.mpg_volume_projections_ws_bytes(a, b, c)), dtype=torch.uint8, device=vol.device)
    _lib.check(lib.mpg_volume_projections(_stream(), _ptr(vol), a, b, c, float(divisor), _ptr(p0), _ptr(p1), _ptr(p2), _ptr(ws)),
               "mpg_volume_projections")
    return p0, p1, p2


def volume_planes_gray8(vol, axis, idx, transposed=False):
    """the planes of vol [a,b,c] at the indices idx of `axis` as 8-bit grey [len(idx), rows, cols] (the two remaining axes
    in array order, swapped when transposed) and their float32 means [len(idx)] (multipassGAN-out.py:592-604)."""
    lib = _lib.load()
    vol, dims = _volume3(vol, "volume_planes_gray8")
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise _lib.MpgError("volume_planes_gray8: axis %r (0..2)" % (axis,))
    idx = [int(i) for i in idx]
    rest = [d for k, d in enumerate(dims) if k != axis]
    if transposed:
        rest.reverse()
    gray = torch.empty([len(idx)] + rest, dtype=torch.uint8, device=vol.device)
    mean = torch.empty(len(idx), dtype=torch.float32, device=vol.device)
    if not idx:
        return gray, mean
    arr = (ctypes.c_int * len(idx))(*idx)
    _lib.check(lib.mpg_volume_planes_gray8(_stream(), _ptr(vol), dims[0], dims[1], dims[2], axis, arr, len(idx),
                                           1 if transposed else 0, _ptr(gray), _ptr(mean)), "mpg_volume_planes_gray8")
    return gray, mean


def gray8(img):
    """uint8(clip(img * 255, 0, 255)) of a float32 image (save_img, multipassGAN-out.py:204-206)."""
    lib = _lib.load()
    img = _dev(img, "img")
    out = torch.empty(img.shape, dtype=torch.uint8, device=img.device)
    _lib.check(lib.mpg_gray8(_stream(), _ptr(img), img.numel(), _ptr(out)), "mpg_gray8")
    return out
