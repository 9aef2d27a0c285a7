"""Convolutions wider than 128 outputs on the MI355X: the channel-window store of the fused convolution
(mpg_conv2d_fused_window), the pixel norm of a G8 tensor (mpg_pixel_norm_g8), ops.conv2d_fused_wide on top of both, and the
default-width 8x generators (startFms 512, maxFms 256) against the oracle.

Shapes: N = 2, 40 x 40 pixels (ragged against the 16 x 32 and 8 x 32 tiles in both directions, several blocks), cin 16,
in some cases a second 1x1 segment of 8 channels."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import conv_exact_ref as CE
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, H, W, CIN, CIN2 = 2, 40, 40, 16, 8
MPG_ERR_ARG = 1


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


class Layer(object):
    """one wide layer: inputs, weights of every segment for all c_total outputs, bias, post-add tensor"""

    def __init__(self, c_total, k, two_segments, exact, ops):
        rng = np.random.default_rng(zlib.crc32(("%d %d %d %d" % (c_total, k, two_segments, exact)).encode()))
        shapes = [(k, CIN)] + ([(1, CIN2)] if two_segments else [])
        kk = sum(kf * kf * ci for kf, ci in shapes)
        make = (lambda s: CE.lo_exact(rng, s, 13 if kk <= 2046 else 12)[0]) if exact else (lambda s: rng.standard_normal(s).astype(np.float32))
        self.c_total = c_total
        self.x = [ops.to_g8(_t(make((N, H, W, ci)))) for _, ci in shapes]
        self.w = [_t(make((kf, kf, ci, c_total))) for kf, ci in shapes]
        self.bias = _t(rng.standard_normal(c_total))
        self.post = _t(rng.standard_normal((N, H, W, c_total + 5)))      # the post-add window starts at channel 3 of it

    def segments(self, ops, co, cw, prec):
        return [ops.Segment(x, ops.pack_conv_weights(w[..., co:co + cw].contiguous(), prec=prec)) for x, w in zip(self.x, self.w)]


def _equal(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.numel())


# ---- a. a window holds what the launch of its channels alone computes, bit for bit ------------------------------------
@pytest.mark.parametrize("prec", [1, 2, 3])
@pytest.mark.parametrize("c_total", [136, 192, 256, 264, 320])
def test_window_equals_launch(gpu_ops, c_total, prec):
    ops = gpu_ops
    chunks = ops.wide_chunks(c_total)
    # 3x3 and 5x5, one and two segments, lo-plane-exact and dense normal data; bias + lrelu + post-add in every launch
    for k, two, exact in ((3, True, True), (5, False, True), (3, False, False), (5, True, False)):
        L = Layer(c_total, k, two, exact, ops)
        launches = [(L.segments(ops, co, cw, prec), co) for co, cw in chunks]
        kw = dict(act="lrelu", leak=0.2, post_add=L.post)
        y, g = ops.conv2d_fused_wide(launches, (H, W), c_total, bias=L.bias, post_add_coff=3, want_f32=True, want_g8=True, **kw)
        g_only = ops.conv2d_fused_wide(launches, (H, W), c_total, bias=L.bias, post_add_coff=3, want_f32=False, want_g8=True, **kw)
        # without post-add a G8-only launch takes the register-store path of the epilogue
        r_only = ops.conv2d_fused_wide(launches, (H, W), c_total, bias=L.bias, act="lrelu", want_f32=False, want_g8=True)
        assert (g.c, g.groups, g_only.groups) == (c_total, (c_total + 7) // 8, (c_total + 7) // 8)
        y8, y8_only, r8_only = ops.from_g8(g), ops.from_g8(g_only), ops.from_g8(r_only)
        for (co, cw), (segs, _) in zip(chunks, launches):
            what = "c_total %d prec %d %dx%d window [%d, %d)" % (c_total, prec, k, k, co, co + cw)
            py, pg = ops.conv2d_fused(segs, (H, W), bias=L.bias[co:co + cw].contiguous(), post_add_coff=3 + co, want_f32=True,
                                      want_g8=True, **kw)
            _equal(y[..., co:co + cw], py, what + " fp32")
            _equal(y8[..., co:co + cw], ops.from_g8(pg), what + " G8")
            _equal(y8_only[..., co:co + cw], ops.from_g8(pg), what + " G8 alone")
            pr = ops.conv2d_fused(segs, (H, W), bias=L.bias[co:co + cw].contiguous(), act="lrelu", want_f32=False, want_g8=True)
            _equal(r8_only[..., co:co + cw], ops.from_g8(pr), what + " G8 alone, no post-add")


def test_wide_argument_checks(gpu_ops):
    ops = gpu_ops
    from mpgan_amd import _lib
    L = Layer(192, 3, False, False, ops)
    a, b = L.segments(ops, 0, 96, 3), L.segments(ops, 96, 96, 3)
    for bad in ([(a, 0)], [(a, 0), (b, 104)], [(a, 0), (a, 0), (b, 96)], [(b, 96)]):
        with pytest.raises(_lib.MpgError):
            ops.conv2d_fused_wide(bad, (H, W), 192)
    with pytest.raises(_lib.MpgError):
        ops.conv2d_fused_wide([(a, 0), (b, 96)], (H, W), 192, bias=L.bias[:96].contiguous())
    with pytest.raises(_lib.MpgError):       # the post-add would have to follow the pixel norm
        ops.conv2d_fused_wide([(a, 0), (b, 96)], (H, W), 192, pixel_norm=True, post_add=L.post)
    with pytest.raises(_lib.MpgError):
        ops.pack_conv_weights(L.w[0], prec=3)                 # one launch's weight image stays at 128 outputs


# ---- b. nothing outside the window is written ---------------------------------------------------------------------------
def _desc(ops, L, co, cw, prec, y, y8):
    segs = L.segments(ops, co, cw, prec)
    d = ops._conv_desc(segs, (H, W), L.bias[co:co + cw].contiguous(), "lrelu", 0.2)
    d.y, d.y_g8 = ops._ptr(y), ops._ptr(y8)
    return d, segs


@pytest.mark.parametrize("prec", [1, 2, 3])
@pytest.mark.parametrize("outputs", ["both", "g8", "f32"])
def test_window_writes_only_its_channels(gpu_ops, prec, outputs):
    ops = gpu_ops
    from mpgan_amd import _lib
    lib = _lib.load()
    c_total, co, cw = 320, 128, 64
    L = Layer(c_total, 3, True, False, ops)
    y = torch.full((N, H, W, c_total * 4), 0xA5, dtype=torch.uint8, device=DEV).view(torch.float32) if outputs != "g8" else None
    g = ops.G8.empty(N, H, W, c_total, DEV) if outputs != "f32" else None
    if g is not None:
        g.buf.view(torch.uint8).fill_(0x5A)
    d, segs = _desc(ops, L, co, cw, prec, y, g)
    _lib.check(lib.mpg_conv2d_fused_window(ops._stream(), ctypes.byref(d), c_total, co), "mpg_conv2d_fused_window")
    py, pg = ops.conv2d_fused(segs, (H, W), bias=L.bias[co:co + cw].contiguous(), act="lrelu", want_f32=True, want_g8=True)
    torch.cuda.synchronize()
    if y is not None:
        raw = y.view(torch.uint8).reshape(N, H, W, c_total, 4)
        assert bool((raw[..., :co, :] == 0xA5).all()) and bool((raw[..., co + cw:, :] == 0xA5).all())
        _equal(y[..., co:co + cw], py, "fp32 window")
    if g is not None:
        raw = g.buf.view(torch.uint8)               # [N][40 groups][2][H][W][16 bytes]
        assert bool((raw[:, :co // 8] == 0x5A).all()) and bool((raw[:, (co + cw) // 8:] == 0x5A).all())
        assert torch.equal(g.buf[:, co // 8:(co + cw) // 8], pg.buf)


# ---- c. the ragged last group -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 2, 3])
def test_ragged_last_group_is_zero_padded(gpu_ops, prec):
    ops = gpu_ops
    from mpgan_amd import _lib
    lib = _lib.load()
    c_total = 130
    L = Layer(c_total, 3, False, False, ops)
    chunks = ops.wide_chunks(c_total)
    launches = [(L.segments(ops, co, cw, prec), co) for co, cw in chunks]
    for both in (True, False):
        res = ops.conv2d_fused_wide(launches, (H, W), c_total, bias=L.bias, act="lrelu", want_f32=both, want_g8=True)
        g = res[1] if both else res
        assert g.groups == 17
        assert bool((g.buf[:, 16, :, :, :, 2:] == 0).all()), "padding channels of the last group"
        assert bool((g.buf[:, 16, 0, :, :, :2] != 0).all())
        if both:
            _equal(ops.from_g8(g), torch.as_tensor(CE.g8_roundtrip(res[0].cpu().numpy()), device=DEV), "G8 against fp32")
        # the last window again into a tensor that starts out as a byte pattern: the zeros found are zeros written
        co, cw = chunks[-1]
        g2 = ops.G8.empty(N, H, W, c_total, DEV)
        g2.buf.view(torch.uint8).fill_(0x3C)
        y2 = torch.zeros((N, H, W, c_total), dtype=torch.float32, device=DEV) if both else None
        d, _ = _desc(ops, L, co, cw, prec, y2, g2)
        _lib.check(lib.mpg_conv2d_fused_window(ops._stream(), ctypes.byref(d), c_total, co), "mpg_conv2d_fused_window")
        assert torch.equal(g2.buf[:, co // 8:], g.buf[:, co // 8:])
        assert bool((g2.buf.view(torch.uint8)[:, :co // 8] == 0x3C).all())


# ---- d. what the window launch refuses ----------------------------------------------------------------------------------
def test_window_launch_refuses(gpu_ops):
    ops = gpu_ops
    from mpgan_amd import _lib
    lib = _lib.load()
    c_total = 320
    L = Layer(c_total, 3, False, False, ops)
    y = torch.zeros((N, H, W, c_total), dtype=torch.float32, device=DEV)
    g = ops.G8.empty(N, H, W, c_total, DEV)
    g.buf.zero_()

    def rc(co, cw, y_=y, g_=g, pn=0, total=c_total):
        d, _ = _desc(ops, L, max(0, min(co, c_total - cw)), cw, 3, y_, g_)
        d.pixel_norm = pn
        return lib.mpg_conv2d_fused_window(ops._stream(), ctypes.byref(d), total, co)

    assert rc(128, 64) == 0
    assert rc(2, 64, g_=None) == 0                   # fp32 alone may start anywhere (rows off the 16-byte grid)
    _equal(y[..., 2:66], ops.conv2d_fused(L.segments(ops, 2, 64, 3), (H, W), bias=L.bias[2:66].contiguous(), act="lrelu"), "window at 2")
    assert rc(4, 64) == MPG_ERR_ARG                  # a G8 group belongs to one window
    assert rc(132, 64, y_=None) == MPG_ERR_ARG
    assert rc(288, 64) == MPG_ERR_ARG                # past c_total
    assert rc(0, 64, total=32) == MPG_ERR_ARG
    assert rc(-8, 64) == MPG_ERR_ARG
    assert rc(128, 64, pn=1) == MPG_ERR_ARG          # the pixel norm needs every channel of the pixel
    assert rc(128, 60) == MPG_ERR_ARG                # ragged inner window
    assert rc(128, 60, g_=None) == 0                 # ... which fp32 alone allows
    assert rc(264, 50, total=314) == 0               # ragged last window (314 channels: the same 40 groups)
    assert b"mpg_conv2d_fused_window" in lib.mpg_last_error()
    torch.cuda.synchronize()


# ---- e. pixel norm of a G8 tensor ---------------------------------------------------------------------------------------
# Bound of the issue: the G8 input is exact to 2^-22 and the kernel adds a few fp32 roundings (sum, divide, rsqrt,
# multiply) and the 2^-22 of the output split: max |diff| <= 2^-20 max |y| per tensor.
PN_BOUND = 2.0 ** -20


@pytest.mark.parametrize("c", [72, 128, 130, 256])
def test_pixel_norm_g8(gpu_ops, c):
    """against float64 oracle.ops.pixel_norm of the values the G8 tensor holds; for c <= 128 also against the pixel norm
    of the fused epilogue.  Each figure is printed before it is asserted.  Measured on an MI355X (max |diff| / max |y|,
    bound 9.5e-7): c = 72 / 128 / 130 / 256: fp32 1.05e-7 / 1.13e-7 / 1.20e-7 / 1.21e-7, G8 1.46e-7 / 1.24e-7 / 1.34e-7 /
    1.39e-7; against the fused epilogue 1.6e-7 (c = 72), 2.2e-7 (c = 128)."""
    ops = gpu_ops
    from oracle import ops as O
    rng = np.random.default_rng(c)
    x = (rng.standard_normal((N, H, W, c)) * np.exp(rng.standard_normal((N, H, W, 1)))).astype(np.float32)
    g = ops.to_g8(_t(x))
    held = ops.from_g8(g).cpu().numpy().astype(np.float64)
    want = held / np.sqrt(np.mean(held * held, axis=3, keepdims=True) + 1e-8)
    assert np.array_equal(O.pixel_norm(held.astype(np.float32)), want.astype(np.float32))     # that is the oracle's formula
    g2 = ops.to_g8(_t(x))
    y = ops.pixel_norm_g8(g, 1e-8, want_f32=True)
    assert ops.pixel_norm_g8(g2, 1e-8) is g2
    assert torch.equal(g.buf, g2.buf)
    got32, got8 = y.cpu().numpy().astype(np.float64), ops.from_g8(g).cpu().numpy().astype(np.float64)
    e32, e8 = np.abs(got32 - want).max() / np.abs(want).max(), np.abs(got8 - want).max() / np.abs(want).max()
    print("pixel_norm_g8 c %d: max |diff| / max |y| fp32 %.3e, G8 %.3e (bound %.3e)" % (c, e32, e8, PN_BOUND))
    assert e32 <= PN_BOUND and e8 <= PN_BOUND
    if c % 8:
        assert bool((g.buf[:, -1, :, :, :, c % 8:] == 0).all()), "padding channels after the in-place pass"
    if c <= 128:
        # the same values through the fused epilogue: a 1x1 convolution with the identity matrix
        eye = ops.pack_conv_weights(torch.eye(c, device=DEV).reshape(1, 1, c, c).contiguous(), prec=3)
        f = ops.conv2d_fused([ops.Segment(ops.to_g8(_t(x)), eye)], (H, W), pixel_norm=True, pn_eps=1e-8).cpu().numpy().astype(np.float64)
        ef = np.abs(got32 - f).max() / np.abs(f).max()
        print("pixel_norm_g8 c %d: against the fused epilogue %.3e" % (c, ef))
        assert ef <= PN_BOUND


def test_wide_pixel_norm_outputs(gpu_ops):
    """conv2d_fused_wide with pixel norm: fp32 alone, G8 alone and both hold the same values; the norm follows the activation"""
    ops = gpu_ops
    c_total = 136
    L = Layer(c_total, 3, True, False, ops)
    launches = [(L.segments(ops, co, cw, 3), co) for co, cw in ops.wide_chunks(c_total)]
    kw = dict(bias=L.bias, act="lrelu", pixel_norm=True, pn_eps=1e-8)
    y, g = ops.conv2d_fused_wide(launches, (H, W), c_total, want_f32=True, want_g8=True, **kw)
    y_only = ops.conv2d_fused_wide(launches, (H, W), c_total, want_f32=True, want_g8=False, **kw)
    out = torch.empty_like(y)
    assert ops.conv2d_fused_wide(launches, (H, W), c_total, want_f32=False, want_g8=False, out=out, **kw) is out
    g_only = ops.conv2d_fused_wide(launches, (H, W), c_total, want_f32=False, want_g8=True, **kw)
    _equal(y_only, y, "fp32 alone")
    _equal(out, y, "fp32 into out")
    assert torch.equal(g_only.buf, g.buf)
    lin = ops.conv2d_fused_wide(launches, (H, W), c_total, bias=L.bias, act="lrelu").cpu().numpy().astype(np.float64)
    want = lin / np.sqrt(np.mean(lin * lin, axis=3, keepdims=True) + 1e-8)
    # the windows hand their values over as G8 (2^-22) in front of the norm
    err = np.abs(y.cpu().numpy() - want).max() / np.abs(want).max()
    print("conv2d_fused_wide pixel norm: max |diff| / max |y| %.3e" % err)
    assert err <= 2 * PN_BOUND


# ---- f. / g. the default-width generators ------------------------------------------------------------------------------
DEFAULTS = dict(filter_size=3, start_fms=512, max_fms=256, use_res_net=True, first_nn_arch=False)
NETS = {"first": dict(first_gen=True, add_adj=True, **DEFAULTS), "later": dict(first_gen=False, **DEFAULTS)}
TOL = {3: 1e-4, 2: 5e-4}
LOW, UP, NCH = 8, 8, 4


@pytest.fixture(scope="module")
def oracle_nets():
    """inputs, parameters and the oracle's output of both configurations, computed once"""
    from oracle import nets as ON
    from oracle import torch_ref
    res = {}
    for name, cfg in NETS.items():
        rng = np.random.default_rng(3)
        ps = ON.ParamSource(seed=11)
        with torch_ref.fast_convs():
            if cfg["first_gen"]:
                x, yp = rng.standard_normal((2, LOW, LOW, NCH + 2)).astype(np.float32), None
                ref = ON.growing_gen(ps, x, UP, True, 3, 512, 256, False, True)[..., 0]
            else:
                x = rng.standard_normal((2, LOW, LOW, NCH)).astype(np.float32)
                yp = rng.random((2, LOW * UP, LOW * UP, 1)).astype(np.float32)
                ref = ON.growing_gen(ps, ON.gen2_input(yp, x, LOW * UP), UP, False, 3, 512, 256, False, True)[..., 0]
        assert np.isfinite(ref).all() and np.linalg.norm(ref) > 1.0 and ref.std() > 1e-2, "degenerate oracle output"
        res[name] = (x, yp, ps, ref)
    return res


@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("name", ["first", "later"])
def test_default_width_generator(mpg, oracle_nets, name, prec):
    from mpgan_amd import multipass as MP
    x, yp, ps, ref = oracle_nets[name]
    gen = MP.Generator("growing_gen", dict(tile_low=LOW, up_res=UP, channels=NCH, **NETS[name]), params=ps.params, prec=prec)
    assert sorted(gen.graph.variables) == sorted(ps.params)
    wide = [e for e in gen.sess.plan_summary(gen.sampler) if e.get("launches")]
    assert [(e["kind"], e["cout"], e["launches"]) for e in wide] == [("conv2d_fused", 256, 2)] * 2
    y = gen(_t(x), _t(yp[..., 0]) if yp is not None else None).cpu().numpy()
    err = rel_l2(y, ref)
    print("default-width %s generator prec %d: rel L2 %.3e (bound %.1e)" % (name, prec, err, TOL[prec]))
    assert err < TOL[prec], err


def test_default_width_pass_lanes(mpg):
    """the slice batches of a pass on two HIP streams give the plain loop's bits with the wide layers (window launches
    and the G8 pixel norm of one lane next to the matrix-core kernels of the other)"""
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    keep = MP.PASS_LANES[0]
    try:
        low = _t(synthetic_volume(LOW, NCH, 2))
        g1 = MP.Generator("growing_gen", dict(tile_low=LOW, up_res=UP, channels=NCH, **NETS["first"]), None, 2, seed=40)
        g2 = MP.Generator("growing_gen", dict(tile_low=LOW, up_res=UP, channels=NCH, **NETS["later"]), None, 2, seed=41)
        res = {}
        for lanes in (1, 2):
            MP.set_pass_lanes(lanes)
            v1 = MP.single_pass_8x(g1, low, None, UP, batch=8)
            v2 = MP.single_pass_8x(g2, low, v1, UP, batch=8)
            torch.cuda.synchronize()
            res[lanes] = (v1.cpu().numpy(), v2.cpu().numpy())
        assert np.isfinite(res[1][1]).all() and np.abs(res[1][0]).max() > 0 and np.abs(res[1][1]).max() > 0
        assert np.array_equal(res[2][0], res[1][0]) and np.array_equal(res[2][1], res[1][1])
    finally:
        MP.set_pass_lanes(keep)
