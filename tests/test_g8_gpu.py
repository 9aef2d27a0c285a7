"""The G8 tensor functions against an independent numpy model (g8_ref.py), byte for byte.

Every fused convolution, the weight gradient and mpg_bn_infer_act exchange activations as G8 tensors, and the exact suites
of those kernels feed their inputs through ops.to_g8 and read their results through ops.from_g8: a fault shared by the two
conversions, a mis-rounded hi plane with a compensating lo, or a scale that overflows passes all of them.  Here

1. mpg_f32_to_g8 / mpg_f32_to_g8_scaled store exactly g8_ref.pack(): both kernels, every predicate of the dispatch,
   every data class (ties, fp16 subnormals, flushed lo, -0, the ends of the range), unscaled and under every amax of the
   scale-law table, written into a device float directly;
2. mpg_g8_to_f32 returns exactly g8_ref.unpack() of planes that are no split of anything;
3. mpg_absmax returns the reference's bits: scalar and 16-byte paths, tails, the grid cap, NaN, inf, -0;
4. mpg_pixel_norm_g8 stores the canonical split of the fp32 values it returns, for both instantiations, ragged pixel
   blocks and c < 32, and stays within PN_BOUND of the float64 pixel norm;
5. every other G8 store site (the staged and the register path of csrc/mpgan_conv.h, depth-to-space, window, small_store
   and the pair kernel) stores the canonical split of the launch's own fp32 output on general data;
6. the scale law holds at its consumers where the uncapped law gave NaN (activations of 2^-122) and 0 (the weight gradient
   of x 2^-55 and dy 2^-60).

Outputs lie inside larger buffers filled with a sentinel: the guard words on both sides must be untouched, and inside the
tensor every byte must equal the model, zero padding included.  All assertions are on bits; the one tolerance is the
PN_BOUND of test_wide_conv_gpu.py.  test_g8_host.py proves on the CPU what the model and the case tables claim.
"""
import ctypes

import numpy as np
import pytest
import torch

import g8_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
GUARD = 64                       # sentinel words on both sides of an output
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
MPG_ERR_ARG = 1
PN_BOUND = 2.0 ** -20            # of test_wide_conv_gpu.py


@pytest.fixture(scope="module")
def lib(gpu_ops):
    from mpgan_amd import _lib
    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _ok(rc, lib, what):
    assert rc == 0, "%s: %d %s" % (what, rc, lib.mpg_last_error().decode())


class Guarded(object):
    """`words` elements of 2 or 4 bytes between two guards of sentinel words, all on the device; .ptr is the first element
    (16-byte aligned, `misalign` bytes further on request)"""

    def __init__(self, words, size, misalign=0, init=None):
        self.words, self.size, self.off = words, size, GUARD + misalign // size
        dt, self.np_dt, self.sent = (torch.int16, np.uint16, SENT16) if size == 2 else (torch.int32, np.uint32, SENT32)
        sent = int(np.array([self.sent], self.np_dt).view(np.int16 if size == 2 else np.int32)[0])
        self.buf = torch.full((GUARD + words + GUARD + 16,), sent, dtype=dt, device=DEV)
        assert self.buf.data_ptr() % 16 == 0 and (GUARD * size) % 16 == 0
        if init is not None:
            src = np.ascontiguousarray(init).reshape(-1).view(np.int16 if size == 2 else np.int32)
            assert src.size == words
            self.buf[self.off:self.off + words].copy_(torch.from_numpy(src.copy()))
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.off * size)

    def read(self, what):
        """the tensor's words (flat, unsigned) after checking the guards"""
        got = self.buf.cpu().numpy().view(self.np_dt)
        assert (got[:self.off] == self.sent).all(), what + ": written in front of the tensor"
        assert (got[self.off + self.words:] == self.sent).all(), what + ": written behind the tensor"
        return got[self.off:self.off + self.words]


def _upload(x, misalign=0):
    """x (float32 numpy) on the device at `misalign` bytes off a 16-byte boundary: (keep-alive tensor, pointer)"""
    flat = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    buf = torch.empty(flat.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0 and misalign % 4 == 0
    view = buf[misalign // 4:misalign // 4 + flat.size]
    view.copy_(torch.from_numpy(flat))
    return buf, ctypes.c_void_p(buf.data_ptr() + misalign)       # (an empty view has no address of its own)


def _g8_report(got, want, shape, what):
    """'' when the uint16 images are equal, else where they differ: how many words, the first (n, group, plane, y, x, lane)"""
    got, want = np.asarray(got).reshape(shape), np.asarray(want).reshape(shape)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return ""
    i = tuple(int(v) for v in bad[0])
    planes = sorted({int(b[2]) for b in bad})
    grps = sorted({int(b[1]) for b in bad})
    return ("%s: %d of %d words differ; first at (n, group, plane, y, x, lane) = %s: got 0x%04x (%r), expected 0x%04x (%r); planes hit %s, "
            "groups hit %s" % (what, len(bad), got.size, i, int(got[i]), float(got[i].view(np.float16)), int(want[i]),
                               float(want[i].view(np.float16)), planes, grps[:12]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. fp32 -> G8
# ---------------------------------------------------------------------------------------------------------------------
def _convert(lib, case, xptr, amax, out):
    if amax is None:
        return lib.mpg_f32_to_g8(_stream(), xptr, case.n, case.h, case.w, case.c, case.c_off, case.cin, 0, out.ptr)
    return lib.mpg_f32_to_g8_scaled(_stream(), xptr, case.n, case.h, case.w, case.c, case.c_off, case.cin, 0, ctypes.c_void_p(amax.data_ptr()),
                                    out.ptr)


@pytest.mark.parametrize("case", R.TO_G8_CASES, ids=repr)
def test_f32_to_g8_stores_the_canonical_split(lib, case):
    """unscaled through mpg_f32_to_g8, then mpg_f32_to_g8_scaled under every amax of the scale-law table (the scalar is
    written into a device float, no mpg_absmax here; the data is the case's tensor divided by the model's scale, so the
    scaled values stay within the contract).  amax = 1e-37 and 2^-120 .. 2^-140 gave NaN for every zero before the cap."""
    base = R.to_g8_data(case)
    shape = (case.n, R.groups(case.cin), 2, case.h, case.w, 8)
    words = int(np.prod(shape))
    assert lib.mpg_g8_bytes(case.n, case.h, case.w, case.cin) == 2 * words
    runs = [("unscaled", None)] + R.AMAX_TABLE
    keep = {}
    for name, amax in runs:
        scale = F32(1.0) if amax is None else R.pow2_scale(amax)
        if float(scale) not in keep:
            x = base if float(scale) == 1.0 else R.scaled_data(base, scale)
            keep[float(scale)] = (x,) + _upload(x, case.misalign)
        x, _, xptr = keep[float(scale)]
        assert xptr.value % 16 == case.misalign
        out = Guarded(words, 2)
        dev_amax = None if amax is None else torch.from_numpy(np.array([amax], F32)).to(DEV)
        _ok(_convert(lib, case, xptr, dev_amax, out), lib, "mpg_f32_to_g8")
        got = out.read("%s, amax %s" % (case, name))
        want = R.pack(x, case.c_off, case.cin, scale)
        assert np.isfinite(want.view(np.float16)).all()
        msg = _g8_report(got, want, shape, "%s, amax %s (scale 2^%d)" % (case, name, int(np.log2(float(scale)))))
        assert not msg, msg


NAN_CASES = [c for c in R.TO_G8_CASES if (c.n, c.h, c.w, c.c, c.c_off, c.cin) in ((2, 3, 11, 36, 4, 32), (2, 3, 5, 19, 2, 17))]


@pytest.mark.parametrize("case", NAN_CASES, ids=repr)
def test_f32_to_g8_nan_and_inf_stay_where_they_are(lib, case):
    """one NaN and one inf element, on the tiled and on the per-pixel kernel, unscaled and under amax = 1 (scale 2^8): hi of
    the NaN element is NaN, hi of the inf element is that inf, every other word is the model's (only finite values are the
    contract of include/mpgan.h; the payload of a NaN is not part of it)"""
    assert sorted(c.kernel for c in NAN_CASES) == ["pixel", "tiled"]
    rng = np.random.default_rng(11)
    special = {}
    for v in (np.nan, -np.inf):
        p = (int(rng.integers(case.n)), int(rng.integers(case.h)), int(rng.integers(case.w)), case.c_off + int(rng.integers(case.cin)))
        assert p not in special
        special[p] = v
    shape = (case.n, R.groups(case.cin), 2, case.h, case.w, 8)
    for amax in (None, F32(1.0)):
        scale = F32(1.0) if amax is None else R.pow2_scale(amax)
        clean = R.scaled_data(R.to_g8_data(case), scale)
        data = clean.copy()
        for p, v in special.items():
            data[p] = v
            clean[p] = 0.0
        keepalive, xptr = _upload(data, case.misalign)
        out = Guarded(int(np.prod(shape)), 2)
        dev_amax = None if amax is None else torch.from_numpy(np.array([amax], F32)).to(DEV)
        _ok(_convert(lib, case, xptr, dev_amax, out), lib, "mpg_f32_to_g8")
        got = out.read(repr(case)).reshape(shape).copy()
        for (b, y, xx, ch), v in special.items():
            cw = ch - case.c_off
            hi = got[b, cw // 8, 0, y, xx, cw % 8:cw % 8 + 1].view(np.float16)[0]
            assert np.isnan(hi) if np.isnan(v) else hi == v, (case, amax, v, hi)
            got[b, cw // 8, :, y, xx, cw % 8] = 0
        msg = _g8_report(got, R.pack(clean, case.c_off, case.cin, scale), shape, "%s with a NaN and an inf, scale %g" % (case, scale))
        assert not msg, msg


# ---------------------------------------------------------------------------------------------------------------------
# 2. G8 -> fp32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.FROM_G8_CHANNELS)
def test_g8_to_f32_adds_the_planes(lib, c):
    """planes that are no split of anything: random finite fp16 patterns in both, subnormals and both zeros among them; the
    padding lanes of the last group hold NaN patterns that must not reach the output"""
    n, h, w = R.FROM_G8_NHW
    img = R.poison_padding(R.fp16_patterns((n, R.groups(c), 2, h, w, 8), "from_g8 %d" % c), c)
    g = Guarded(img.size, 2, init=img)
    y = Guarded(n * h * w * c, 4)
    _ok(lib.mpg_g8_to_f32(_stream(), g.ptr, n, h, w, c, y.ptr), lib, "mpg_g8_to_f32")
    got = y.read("c %d" % c).reshape(n, h, w, c)
    want = R.unpack(img, c).view(np.uint32)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "c %d: %d of %d values differ, first at (n, y, x, c) = %s: got 0x%08x, expected 0x%08x" % (
        c, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(g.read("input c %d" % c), img.reshape(-1)), "the input was written"


# ---------------------------------------------------------------------------------------------------------------------
# 3. absmax
# ---------------------------------------------------------------------------------------------------------------------
def _absmax(lib, xptr, n):
    out = Guarded(1, 4, init=np.array([1e30], F32))          # proves that the result is reset, not only raised
    _ok(lib.mpg_absmax(_stream(), xptr, n, out.ptr), lib, "mpg_absmax")
    return int(out.read("absmax of %d" % n)[0])


@pytest.mark.parametrize("misalign", [0, 4])
@pytest.mark.parametrize("n", R.ABSMAX_SIZES)
def test_absmax_bits(lib, n, misalign):
    base = (R.normal(max(n, 1), "absmax %d" % n) * F32(0.25)).clip(-3.0, 3.0).astype(F32)[:n]
    variants = {"plain": base}
    for name, (i, v) in R.absmax_positions(n, misalign).items():
        variants[name] = base.copy()
        variants[name][i] = v
    if n:
        z = np.zeros(n, F32)
        z[n // 2] = -0.0
        variants["zeros with -0"] = z
        variants["all NaN"] = np.full(n, np.nan, F32)
        for name, v in (("NaN beside the maximum", np.nan), ("inf", -np.inf)):
            variants[name] = base.copy()
            variants[name][0] = 7.5
            variants[name][n - 1] = v
            if n > 4:
                variants[name][n // 2] = v
    for name, x in variants.items():
        keepalive, xptr = _upload(x, misalign)
        got = _absmax(lib, xptr, n)
        want = int(R.absmax(x).view(np.uint32))
        assert got == want, "n %d, +%d bytes, %s: got 0x%08x, expected 0x%08x" % (n, misalign, name, got, want)


def test_absmax_under_the_grid_cap(lib):
    """17 * 2^20 floats: 4352 blocks' worth of elements on 4096 blocks, so the grid-stride loop takes a second round; the
    maximum is the last element.  The tensor exists on the device only."""
    x = torch.zeros(R.ABSMAX_BIG, dtype=torch.float32, device=DEV)
    x[-1] = -3.0
    x[R.ABSMAX_BIG // 2] = 2.0
    assert _absmax(lib, ctypes.c_void_p(x.data_ptr()), R.ABSMAX_BIG) == int(F32(3.0).view(np.uint32))
    x[-1] = 0.0
    assert _absmax(lib, ctypes.c_void_p(x.data_ptr()), R.ABSMAX_BIG) == int(F32(2.0).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 4. pixel norm of a G8 tensor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.PN_HW, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("c", R.PN_CHANNELS)
def test_pixel_norm_g8_planes(lib, c, hw):
    """(a) the stored planes are g8_ref.pack of the returned fp32 y, byte for byte: the canonical split, zero padding
    included; (b) a call without y leaves the same bytes; (c) y is within PN_BOUND of the float64 pixel norm of the values
    the input holds; (d) NaN patterns in the input's padding lanes change nothing; (e) the guards of both buffers hold.
    Each figure is printed before it is asserted.  Measured on an MI355X, max |y - y64| / max |y64| (bound 2^-20 =
    9.54e-7): between 3.9e-8 (c 33, 1x1) and 1.18e-7 (c 264, 5x13) over the 30 cases; <4> at most 1.13e-7 (c 8, 7x9),
    <8> at most 1.18e-7.  Before the product was pinned in the kernel, (a) failed in 28 of the 30 cases: one lo word in
    eleven was an fp16 ulp off the split of y (c 512, 5x13: 11875 of 133120 words, all in the lo plane)."""
    h, w = hw
    n = R.PN_N
    x = R.pn_input(c, h, w)
    img = R.pack(x)
    shape = img.shape
    want64 = R.pixel_norm64(R.unpack(img, c))
    what = "c %d, %dx%d (<%d>)" % (c, h, w, R.pn_kernel(c))
    res = {}
    for name, planes, with_y in (("poisoned", R.poison_padding(img, c), True), ("clean", img, True), ("no y", R.poison_padding(img, c), False)):
        g = Guarded(img.size, 2, init=planes)
        y = Guarded(n * h * w * c, 4)
        _ok(lib.mpg_pixel_norm_g8(_stream(), g.ptr, n, h, w, c, R.PN_EPS, y.ptr if with_y else None), lib, "mpg_pixel_norm_g8")
        res[name] = (g.read(what + ", " + name), y.read(what + ", y, " + name) if with_y else None)
    got_g, got_y = res["poisoned"]
    y32 = got_y.view(F32).reshape(n, h, w, c)
    assert np.isfinite(y32).all(), what
    msg = _g8_report(got_g, R.pack(y32), shape, what + ": planes against the split of y")             # (a), (d): zero padding
    assert not msg, msg
    assert np.array_equal(res["clean"][0], got_g) and np.array_equal(res["clean"][1], got_y), what + ": the padding lanes were read"
    assert np.array_equal(res["no y"][0], got_g), what + ": the call without y stores other planes"       # (b)
    err = np.abs(y32.astype(np.float64) - want64).max() / np.abs(want64).max()                              # (c)
    print("pixel_norm_g8 %s: max |diff| / max |y| %.3e (bound %.3e)" % (what, err, PN_BOUND))
    assert err <= PN_BOUND, what


def test_pixel_norm_g8_refuses(lib):
    """c = 513, n = 65536 and a y 4 bytes off return MPG_ERR_ARG and launch nothing: both buffers keep their bytes"""
    for n, h, w, c, mis in ((2, 3, 5, 513, 0), (65536, 1, 1, 8, 0), (2, 3, 5, 40, 4)):
        img = R.pack(np.ones((1, 1, 1, 1), F32)).reshape(-1)
        words = n * R.groups(c) * 2 * h * w * 8
        g = Guarded(words, 2, init=np.resize(img, words))
        y = Guarded(n * h * w * c, 4, misalign=mis)
        rc = lib.mpg_pixel_norm_g8(_stream(), g.ptr, n, h, w, c, R.PN_EPS, y.ptr)
        assert rc == MPG_ERR_ARG and b"mpg_pixel_norm_g8" in lib.mpg_last_error(), (n, c, mis, rc)
        torch.cuda.synchronize()
        assert np.array_equal(g.read("refused"), np.resize(img, words))
        assert (y.read("refused y") == SENT32).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the other producers store the canonical split of their own fp32 output
# ---------------------------------------------------------------------------------------------------------------------
H5, W5 = 9, 33


def _general(name, shape, scale=1.0):
    return (R.normal(int(np.prod(shape)), "producer " + name).reshape(shape) * F32(scale)).astype(F32)


def _assert_canonical(y, g, what):
    y = y.cpu().numpy()
    got = g.buf.cpu().numpy().view(np.uint16)
    assert np.isfinite(y).all() and np.abs(y).max() > 0.1 and (y < 0).any(), what + ": degenerate output"
    msg = _g8_report(got, R.pack(y), got.shape, what + ": G8 planes against the split of the fp32 output")
    assert not msg, msg


def _both_paths(call, what):
    """the launch with both outputs (LDS-staged store) and the G8-only launch (register store, where the kernel has one)"""
    y, g = call(want_f32=True, want_g8=True)
    _assert_canonical(y, g, what)
    g2 = call(want_f32=False, want_g8=True)
    _assert_canonical(y, g2, what + ", G8-only launch")


@pytest.mark.parametrize("variant", ["plain", "pixel_norm", "in_amax"])
@pytest.mark.parametrize("prec", [1, 2, 3])
def test_fused_conv_stores_canonical_planes(gpu_ops, prec, variant):
    """csrc/mpgan_conv.h: 3x3x16->33 (a ragged last group, two column tiles) with a bias and lrelu(0.2) on Gaussian data"""
    ops = gpu_ops
    cin, cout = 16, 33
    # in_amax: activations of magnitude 2^12 under weights of 2^-12, so that the unscale is a factor other than 1 and the
    # outputs are of magnitude 1 like the others'
    e = 12 if variant == "in_amax" else 0
    x = _t(_general("x", (1, H5, W5, cin)) * F32(2.0 ** e))
    amax = ops.absmax(x) if variant == "in_amax" else None
    pk = ops.pack_conv_weights(_t(_general("w", (3, 3, cin, cout), 0.1 * 2.0 ** -e)), prec=prec)
    seg = ops.Segment(ops.to_g8(x, amax=amax), pk)
    kw = dict(bias=_t(_general("b", (cout,))), act="lrelu", leak=0.2, pixel_norm=variant == "pixel_norm", pn_eps=1e-8, in_amax=amax)
    _both_paths(lambda **o: ops.conv2d_fused([seg], (H5, W5), **kw, **o), "fused conv, prec %d, %s" % (prec, variant))


@pytest.mark.parametrize("prec", [1, 3])
def test_d2s_conv_stores_canonical_planes(gpu_ops, prec):
    """mpg_conv2d_fused_d2s: 1x1x16->32, stored as 8 channels at twice the resolution"""
    ops = gpu_ops
    seg = ops.Segment(ops.to_g8(_t(_general("x d2s", (1, H5, W5, 16)))), ops.pack_conv_weights(_t(_general("w d2s", (1, 1, 16, 32), 0.3)), prec=prec))
    bias = _t(_general("b d2s", (32,)))
    _both_paths(lambda **o: ops.conv2d_fused_d2s([([seg], 0)], (H5, W5), 32, bias=bias, act="lrelu", leak=0.2, **o), "d2s conv, prec %d" % prec)


@pytest.mark.parametrize("prec", [2, 3])
def test_window_conv_stores_canonical_planes(gpu_ops, prec):
    """mpg_conv2d_fused_window: 3x3x16->136 as windows of 72 and 64 channels of one tensor"""
    ops = gpu_ops
    c_total = 136
    xg = ops.to_g8(_t(_general("x window", (1, H5, W5, 16))))
    wt = _general("w window", (3, 3, 16, c_total), 0.1)
    chunks = [([ops.Segment(xg, ops.pack_conv_weights(_t(wt[..., co:co + cw]), prec=prec))], co) for co, cw in ops.wide_chunks(c_total)]
    assert [co for _, co in chunks] == [0, 72]
    bias = _t(_general("b window", (c_total,)))
    _both_paths(lambda **o: ops.conv2d_fused_wide(chunks, (H5, W5), c_total, bias=bias, act="lrelu", leak=0.2, **o), "window conv, prec %d" % prec)


@pytest.mark.parametrize("cout", [1, 5, 8])
def test_small_conv_stores_canonical_planes(gpu_ops, cout):
    """small_store of csrc/mpgan_conv_small.hip: 3x3x3->cout; the conversion follows the unscale, bias and lrelu arithmetic
    in registers"""
    ops = gpu_ops
    seg = ops.Segment(ops.to_g8(_t(_general("x small", (1, H5, 70, 3)))), ops.pack_conv_weights(_t(_general("w small %d" % cout, (3, 3, 3, cout), 0.3)), prec=3))
    bias = _t(_general("b small %d" % cout, (cout,)))
    _both_paths(lambda **o: ops.conv2d_fused([seg], (H5, 70), bias=bias, act="lrelu", leak=0.2, **o), "small conv, cout %d" % cout)


def test_small_pair_stores_canonical_planes(gpu_ops):
    """mpg_conv2d_small_pair: 1 -> 2 -> 8 channels, 5x5 filters and the 1x1 shortcut"""
    ops = gpu_ops
    pk = lambda name, shape: ops.pack_conv_weights(_t(_general(name, shape, 0.3)), prec=3)
    pa, pb, ps = pk("w pair a", (5, 5, 1, 2)), pk("w pair b", (5, 5, 2, 8)), pk("w pair s", (1, 1, 1, 8))
    xg = ops.to_g8(_t(_general("x pair", (1, H5, 70, 1))))
    kw = dict(bias_a=_t(_general("b pair a", (2,))), act_a="lrelu", leak_a=0.2, bias_b=_t(_general("b pair b", (8,))), act_b="lrelu", leak_b=0.2)
    _both_paths(lambda **o: ops.conv2d_small_pair(xg, 0, 0, pa, pb, ps, (H5, 70), **kw, **o), "small pair")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the scale law at its consumers
# ---------------------------------------------------------------------------------------------------------------------
def _bits_report(got, want, what):
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad) == 0:
        return ""
    i = tuple(int(v) for v in bad[0])
    return "%s: %d of %d values differ (%d NaN, %d zero); first at %s: got %r, expected %r" % (
        what, len(bad), got.size, int(np.isnan(got).sum()), int((got == 0).sum()), i, float(got[i]), float(want[i]))


@pytest.mark.parametrize("kind", ["fused", "small"])
def test_conv_of_tiny_activations(gpu_ops, kind):
    """activations of 2^-122, converted with the scale of their mpg_absmax and convolved with in_amax: the expectation times
    2^-122, bit for bit.  The uncapped scale was inf here: NaN planes (0 * inf in the zero padding at the least) and an
    unscale of 0."""
    ops = gpu_ops
    c = R.conv_consumer(kind)
    x = c.x * F32(2.0 ** R.CONSUMER_E)
    xt = _t(x)
    amax = ops.absmax(xt)
    assert float(amax) == float(R.absmax(x))
    xg = ops.to_g8(xt, amax=amax)
    msg = _g8_report(xg.buf.cpu().numpy().view(np.uint16), R.pack(x, scale=R.pow2_scale(R.absmax(x))), tuple(xg.buf.shape), kind + ": scaled planes")
    assert not msg, msg
    seg = ops.Segment(xg, ops.pack_conv_weights(_t(c.wt), prec=c.prec))
    y = ops.conv2d_fused([seg], (c.h, c.w), in_amax=amax).cpu().numpy()
    want = (c.expected64 * 2.0 ** R.CONSUMER_E).astype(F32)
    msg = _bits_report(y, want, "%s conv at 2^%d" % (kind, R.CONSUMER_E))
    assert not msg, msg


def test_wgrad_of_tiny_operands(gpu_ops):
    """x of 2^-55 and dy of 2^-60, each converted with its own scale (2^63 and 2^68): the gradient is WSCALE 2^-115 times the
    expectation, bit for bit.  The single factor wscale / (sx sd) was 0 here."""
    ops = gpu_ops
    from mpgan_amd import train_ops
    g = R.wgrad_consumer()
    x, d = _t(g.x * F32(2.0 ** R.WG_EX)), _t(g.d * F32(2.0 ** R.WG_ED))
    ax, ad = ops.absmax(x), ops.absmax(d)
    dw = train_ops.conv2d_wgrad_g8(ops.to_g8(x, amax=ax), ops.to_g8(d, amax=ad), g.k, g.k, R.WG_WSCALE, g.prec, ax, ad).cpu().numpy()
    want = (g.expected64 * 2.0 ** (R.WG_EX + R.WG_ED)).astype(F32)
    msg = _bits_report(dw, want, "wgrad at 2^%d x 2^%d" % (R.WG_EX, R.WG_ED))
    assert not msg, msg
    # the entry that converts inside, with both maxima computed there
    dw = train_ops.conv2d_wgrad_mfma(x, d, g.k, g.k, R.WG_WSCALE, g.prec).cpu().numpy()
    msg = _bits_report(dw, want, "wgrad at 2^%d x 2^%d, fp32 operands" % (R.WG_EX, R.WG_ED))
    assert not msg, msg
