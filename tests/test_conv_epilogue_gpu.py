"""The part of a fused convolution behind its K loop -- bias, activation, the zero beyond cout, pixel norm, in_amax,
post_add, the fp32 / G8 / depth-to-space stores -- held bit for bit against float64 on data for which it is exact.

All launches are small: n = 2, h = 19, w = 40, 3x3 over 16 channels, so rows and columns are ragged against the tiles
(16 or 8 rows by 32 columns: 8 or 12 blocks).  cout in {5, 32, 37, 100, 128} covers one, two and four cout tiles,
cout % 4 = 1, cout % 8 = 4 and a full tile.

Exactness.  The lo-exact data of conv_exact_ref.py gives sums e that are multiples of 2^-13 with |e| <= 144 (1 + 6 2^-13)
< 2^8 at K = 144.  The bias values are multiples of 1/4 in [-2, 2]: e + b is a multiple of 2^-13 below 2^8, 21 bits, an
fp32 number whether or not the multiply-add is contracted.  relu is exact.  lrelu with leak 1/4 is evaluated by the library
as (5/8) v + (3/8) |v| (GAN.py:733-737): 5 v and 3 |v| are multiples of 2^-13 below 2^11, 24 bits, their eighths and the
sum (v or v / 4) are exact too.  So the assertion is np.array_equal.  tanh is compared with float64 np.tanh at the
project's bound for elementwise fp32 kernels, relative L2 1e-6 (the table at the top of test_valu_paths_gpu.py).

A G8 tensor keeps hi = fp16(v) and lo = fp16(v - hi) of a value; v / 4 with 21 significant bits does not always fit in
both, so the G8 outputs are compared with that split of the fp32 output (conv_exact_ref.g8_roundtrip), bit for bit, and
the G8-only launch (no fp32 output: the store from registers) with the G8 output of the launch that has both.

conv_small_kernel and conv_small_pair_kernel multiply hi + lo in fp32: small integers, as in test_conv_exact_gpu.py
(|x| <= 2, |w| <= 1 here, so that the second stage of a pair and the eighths of lrelu stay below 24 bits).
"""
import numpy as np
import pytest
import torch

import conv_exact_ref as R
import pixel_shuffle_ref as PSR
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, H, W, CIN = 2, 19, 40, 16
COUTS = (5, 32, 37, 100, 128)
LEAK = 0.25
ACTS = (None, "relu", "lrelu")

_cases = {}


def _case(cout):
    """(case, data) of the shared shape at `cout`; made once, read only"""
    if cout not in _cases:
        case = R.Case("epilogue 3x3x%d->%d" % (CIN, cout), N, H, W, cout, [R.S(3, 3, CIN)], (1, 2, 3))
        assert not case.small and case.frac == 13
        _cases[cout] = (case, R.CaseData(case))
    return _cases[cout]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _bias(cout):
    return (np.random.default_rng(100 + cout).integers(-8, 9, size=cout) * 0.25).astype(np.float32)


def _act64(e, act):
    if act == "relu":
        return np.maximum(e, 0.0)
    if act == "lrelu":
        return np.where(e >= 0.0, e, LEAK * e)
    if act == "tanh":
        return np.tanh(e)
    assert act is None
    return e


def _segments(ops, d, prec):
    return [ops.Segment(_t(d.x[0]), ops.pack_conv_weights(_t(d.w[0]), prec=prec))]


def _three_outputs(ops, case, prec, segs, want, what, exact=True, **kw):
    """launch with both outputs and G8-only: the fp32 output is `want` (bit for bit, or to 1e-6 when not exact), the G8
    output is the split of the fp32 output, the G8-only launch writes the same bits, nothing is NaN and the channels
    of the last group beyond cout are zero"""
    th, tw = R.tile_hw(case, prec)
    y, g = ops.conv2d_fused(segs, (case.h, case.w), want_f32=True, want_g8=True, leak=LEAK, **kw)
    g2 = ops.conv2d_fused(segs, (case.h, case.w), want_f32=False, want_g8=True, leak=LEAK, **kw)
    y = y.cpu().numpy()
    if exact:
        msg = R.mismatch_report(y, want.astype(np.float32), th, tw, what)
        assert not msg, msg
    else:
        err = rel_l2(y, want)
        print("%s: relative L2 %.3e" % (what, err))
        assert err < 1e-6, (what, err)
    assert not np.isnan(y).any(), what
    msg = R.mismatch_report(ops.from_g8(g).cpu().numpy(), R.g8_roundtrip(y), th, tw, what + ", G8 output")
    assert not msg, msg
    assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16)), what + ": G8-only launch differs"
    assert not torch.isnan(g2.buf).any().item(), what + ": NaN in the G8 planes"
    assert g2.c == case.cout and g2.groups == (case.cout + 7) // 8
    if case.cout % 8:
        assert not g2.buf[:, -1, :, :, :, case.cout % 8:].any().item(), what + ": channels beyond cout are not zero"
    return y


@pytest.mark.parametrize("prec", (1, 2, 3))
@pytest.mark.parametrize("cout", COUTS)
def test_bias_and_activation_bit_for_bit(gpu_ops, cout, prec):
    case, d = _case(cout)
    segs = _segments(gpu_ops, d, prec)
    b = _bias(cout)
    for bias in (None, b):
        e = d.expected64(prec) + (0.0 if bias is None else bias.astype(np.float64))
        for act in ACTS:
            want = _act64(e, act)
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)      # an fp32 number
            _three_outputs(gpu_ops, case, prec, segs, want, "%s, prec %d, bias %s, act %s" % (case, prec, bias is not None, act),
                           bias=None if bias is None else _t(bias), act=act)


@pytest.mark.parametrize("prec", (1, 2, 3))
def test_tanh_against_float64(gpu_ops, prec):
    for cout in (5, 37, 128):
        case, d = _case(cout)
        b = _bias(cout)
        want = np.tanh(d.expected64(prec) + b.astype(np.float64))
        _three_outputs(gpu_ops, case, prec, _segments(gpu_ops, d, prec), want, "%s, prec %d, tanh" % (case, prec), exact=False,
                       bias=_t(b), act="tanh")


@pytest.mark.parametrize("prec", (1, 2, 3))
@pytest.mark.parametrize("cout", COUTS)
def test_bias_is_read_inside_its_extent_only(gpu_ops, cout, prec):
    """the bias is elements [1, 1 + cout) of a longer tensor -- 4-byte but not 16-byte aligned -- with NaN on both sides:
    the results are those of the aligned bias and no NaN appears in any output, padded channels included"""
    case, d = _case(cout)
    b = _bias(cout)
    buf = torch.full((cout + 9,), float("nan"), dtype=torch.float32, device=DEV)
    buf[1:1 + cout] = _t(b)
    view = buf[1:1 + cout]
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert torch.isnan(buf[0]).item() and torch.isnan(buf[1 + cout:]).all().item()
    segs = _segments(gpu_ops, d, prec)
    e = d.expected64(prec) + b.astype(np.float64)
    for act in (None, "relu"):
        _three_outputs(gpu_ops, case, prec, segs, _act64(e, act), "%s, prec %d, misaligned bias, act %s" % (case, prec, act),
                       bias=view, act=act)


# ---- the other epilogue paths, one case each at cout 37 -------------------------------------------------------------
@pytest.mark.parametrize("prec", (1, 2, 3))
def test_pixel_norm(gpu_ops, prec):
    """bound of test_kernels_gpu.test_conv2d_fused_single at MPG_PREC_F16X3, 2e-5; the convolution itself is exact at
    every precision on this data, so the same bound holds for all three"""
    case, d = _case(37)
    b = _bias(37)
    v = _act64(d.expected64(prec) + b.astype(np.float64), "lrelu")
    want = v / np.sqrt(np.mean(v * v, axis=3, keepdims=True) + 1e-8)
    segs = _segments(gpu_ops, d, prec)
    y, g = gpu_ops.conv2d_fused(segs, (H, W), bias=_t(b), act="lrelu", leak=LEAK, pixel_norm=True, want_f32=True, want_g8=True)
    g2 = gpu_ops.conv2d_fused(segs, (H, W), bias=_t(b), act="lrelu", leak=LEAK, pixel_norm=True, want_f32=False, want_g8=True)
    err = rel_l2(y.cpu().numpy(), want)
    print("pixel norm, prec %d: relative L2 %.3e" % (prec, err))
    assert err < 2e-5, err
    assert np.array_equal(gpu_ops.from_g8(g).cpu().numpy(), R.g8_roundtrip(y.cpu().numpy()))
    assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16))
    assert not g2.buf[:, -1, :, :, :, 37 % 8:].any().item()


@pytest.mark.parametrize("e", R.AMAX_EXPONENTS)
@pytest.mark.parametrize("prec", (1, 2, 3))
def test_in_amax(gpu_ops, prec, e):
    """as test_conv_exact_gpu.test_in_amax_undoes_the_power_of_two_scale (bit for bit), with a bias behind the scale:
    acc * 2^-k is exact, so y = fp32(e 2^e + b), one rounding of a sum that float64 holds exactly"""
    case, d = _case(37)
    b = _bias(37)
    amax = gpu_ops.absmax(_t(d.x[0] * np.float32(2.0 ** e)))
    xg = gpu_ops.to_g8(_t(d.x[0] * np.float32(2.0 ** e)), amax=amax)
    segs = [gpu_ops.Segment(xg, gpu_ops.pack_conv_weights(_t(d.w[0]), prec=prec))]
    s64 = d.expected64(prec) * 2.0 ** e + b.astype(np.float64)
    for act in (None, "relu"):
        want = _act64(s64, act).astype(np.float32)
        th, tw = R.tile_hw(case, prec)
        y, g = gpu_ops.conv2d_fused(segs, (H, W), bias=_t(b), act=act, in_amax=amax, want_f32=True, want_g8=True)
        g2 = gpu_ops.conv2d_fused(segs, (H, W), bias=_t(b), act=act, in_amax=amax, want_f32=False, want_g8=True)
        msg = R.mismatch_report(y.cpu().numpy(), want, th, tw, "in_amax 2^%d, prec %d, act %s" % (e, prec, act))
        assert not msg, msg
        assert np.array_equal(gpu_ops.from_g8(g).cpu().numpy(), R.g8_roundtrip(want))
        assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16))


@pytest.mark.parametrize("prec", (1, 2, 3))
def test_post_add_channel_window(gpu_ops, prec):
    """as test_conv_exact_gpu.test_post_add_into_a_channel_window (bit for bit): integer addends in channels [3, 40) of a
    45-channel tensor whose other channels are NaN; 32 x 37 and 8 x 37 values per tile row are no multiple of the 256
    the lanes of a wave fetch per round"""
    case, d = _case(37)
    stride, coff = 45, 3
    b = _bias(37)
    pa = np.random.default_rng(7).integers(-8, 9, size=(N, H, W, stride)).astype(np.float32)
    poisoned = np.full_like(pa, np.nan)
    poisoned[..., coff:coff + 37] = pa[..., coff:coff + 37]
    want = _act64(d.expected64(prec) + b.astype(np.float64), "relu") + pa[..., coff:coff + 37]
    segs = _segments(gpu_ops, d, prec)
    y, g = gpu_ops.conv2d_fused(segs, (H, W), bias=_t(b), act="relu", post_add=_t(poisoned), post_add_coff=coff, want_f32=True,
                                want_g8=True)
    th, tw = R.tile_hw(case, prec)
    msg = R.mismatch_report(y.cpu().numpy(), want.astype(np.float32), th, tw, "post_add, prec %d" % prec)
    assert not msg, msg
    msg = R.mismatch_report(gpu_ops.from_g8(g).cpu().numpy(), R.g8_roundtrip(want.astype(np.float32)), th, tw, "post_add G8, prec %d" % prec)
    assert not msg, msg
    g2 = gpu_ops.conv2d_fused(segs, (H, W), bias=_t(b), act="relu", post_add=_t(poisoned), post_add_coff=coff, want_f32=False,
                              want_g8=True)
    assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16))


@pytest.mark.parametrize("cw", (37, 40))
@pytest.mark.parametrize("prec", (1, 3))
def test_depth_to_space_store(gpu_ops, prec, cw):
    """four launches of cw output channels into a 4 cw-channel shuffle.  cw = 37: 37 channels per shuffled pixel, no float4
    store, no G8 output (the library refuses it).  cw = 40: whole G8 groups, so the launch also writes G8 through the
    staging rows and, without the fp32 output, from registers with the shuffled addresses.  Bound of
    test_pixel_shuffle_gpu.test_fused_store_is_bit_identical: the bits of the unfused launches followed by
    depth_to_space; on this data those are the float64 expectation as well."""
    case, d = _case(37)
    ops = gpu_ops
    rng = np.random.default_rng(cw)
    x = _t(d.x[0])
    chunks, unfused, want = [], [], []
    b_all = (rng.integers(-8, 9, size=4 * cw) * 0.25).astype(np.float32)
    for k in range(4):
        _, hi, lo = R.lo_exact(rng, (3, 3, CIN, cw), 13)
        xh, xl = d.parts[0][0]
        e = R.correlate(xh, hi) + (0.0 if prec == 1 else R.correlate(xl, hi) + R.correlate(xh, lo))
        want.append(e + b_all[cw * k:cw * k + cw].astype(np.float64))
        seg = ops.Segment(x, ops.pack_conv_weights(_t((hi + lo).astype(np.float32)), prec=prec))
        chunks.append(([seg], cw * k))
        unfused.append(ops.conv2d_fused([seg], (H, W), bias=_t(b_all[cw * k:cw * k + cw]), act="relu"))
    want = PSR.d2s_nhwc(np.maximum(np.concatenate(want, axis=3), 0.0)).astype(np.float32)
    ref = ops.depth_to_space(torch.cat(unfused, dim=3).contiguous(), 2)
    got = ops.conv2d_fused_d2s(chunks, (H, W), 4 * cw, bias=_t(b_all), act="relu")
    assert got.shape == (N, 2 * H, 2 * W, cw)
    assert torch.equal(got, ref)
    assert np.array_equal(got.cpu().numpy(), want)
    if cw % 8 == 0:
        assert np.array_equal(R.g8_roundtrip(want), want)
        y, g = ops.conv2d_fused_d2s(chunks, (H, W), 4 * cw, bias=_t(b_all), act="relu", want_f32=True, want_g8=True)
        g2 = ops.conv2d_fused_d2s(chunks, (H, W), 4 * cw, bias=_t(b_all), act="relu", want_f32=False, want_g8=True)
        assert torch.equal(y, ref)
        assert g2.c == cw and g2.groups == cw // 8
        assert np.array_equal(ops.from_g8(g).cpu().numpy(), want), "G8 beside the fp32 output"
        assert np.array_equal(ops.from_g8(g2).cpu().numpy(), want), "G8-only launch (stores from registers)"
        assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16))


# ---- the small-channel kernels ---------------------------------------------------------------------------------------
def _ints(rng, shape, m):
    return rng.integers(-m, m + 1, size=shape).astype(np.float64)


@pytest.mark.parametrize("cin,cout", [(1, 2), (8, 2), (2, 1), (8, 8)])
def test_conv_small_kernel(gpu_ops, cin, cout):
    rng = np.random.default_rng(10 * cin + cout)
    n, h, w = 2, 19, 70                                  # 64 x 16 tiles: ragged both ways, 8 blocks
    x, wt = _ints(rng, (n, h, w, cin), 2), _ints(rng, (3, 3, cin, cout), 1)
    b = (rng.integers(-8, 9, size=cout) * 0.25).astype(np.float32)
    e0 = R.correlate(x, wt)
    segs = [gpu_ops.Segment(_t(x), gpu_ops.pack_conv_weights(_t(wt), prec=3))]
    for bias in (None, b):
        e = e0 + (0.0 if bias is None else bias.astype(np.float64))
        for act in ACTS + ("tanh",):
            what = "small %d->%d, bias %s, act %s" % (cin, cout, bias is not None, act)
            y, g = gpu_ops.conv2d_fused(segs, (h, w), bias=None if bias is None else _t(bias), act=act, leak=LEAK, want_f32=True,
                                        want_g8=True)
            y = y.cpu().numpy()
            if act == "tanh":
                assert rel_l2(y, np.tanh(e)) < 1e-6, what
            else:
                msg = R.mismatch_report(y, _act64(e, act).astype(np.float32), 16, 64, what)
                assert not msg, msg
            assert np.array_equal(gpu_ops.from_g8(g).cpu().numpy(), R.g8_roundtrip(y)), what
            if cout % 8:
                assert not g.buf[:, -1, :, :, :, cout % 8:].any().item(), what


@pytest.mark.parametrize("cin,cmid,cout", [(1, 2, 8), (8, 2, 1)])
def test_conv_small_pair_kernel(gpu_ops, cin, cmid, cout):
    """act_b(conv5x5(act_a(conv5x5(x) + bias_a)) + conv1x1(x) + bias_b); the middle tensor is zero outside the image.
    |mid| <= 25 * 8 * 2 + 2 in sixteenths, the second stage below 2^15 in sixteenths: exact for the exact activations.
    tanh: 1e-6 as the last activation (elementwise), and the bound of test_kernels_gpu.test_conv2d_small_pair, 1e-5, as
    the first one (its rounding then runs through the second convolution)."""
    rng = np.random.default_rng(100 * cin + cout)
    n, h, w = 2, 19, 70
    x = _ints(rng, (n, h, w, cin), 2)
    wa, wb, ws = _ints(rng, (5, 5, cin, cmid), 1), _ints(rng, (5, 5, cmid, cout), 1), _ints(rng, (1, 1, cin, cout), 1)
    ba = (rng.integers(-8, 9, size=cmid) * 0.25).astype(np.float32)
    bb = (rng.integers(-8, 9, size=cout) * 0.25).astype(np.float32)
    pk = lambda t: gpu_ops.pack_conv_weights(_t(t), prec=3)
    pa, pb, ps = pk(wa), pk(wb), pk(ws)
    ea, es = R.correlate(x, wa), R.correlate(x, ws)
    combos = [(a1, a2, 1e-6 if a2 == "tanh" else 0.0) for a1 in ACTS for a2 in ACTS + ("tanh",)] + [("tanh", None, 1e-5), ("tanh", "relu", 1e-5)]
    for bias in (False, True):
        for act_a, act_b, tol in combos:
            what = "pair %d->%d->%d, biases %s, act %s / %s" % (cin, cmid, cout, bias, act_a, act_b)
            mid = _act64(ea + (ba.astype(np.float64) if bias else 0.0), act_a)
            e = _act64(R.correlate(mid, wb) + es + (bb.astype(np.float64) if bias else 0.0), act_b)
            y, g = gpu_ops.conv2d_small_pair(_t(x), 0, 0, pa, pb, ps, (h, w), bias_a=_t(ba) if bias else None, act_a=act_a, leak_a=LEAK,
                                             bias_b=_t(bb) if bias else None, act_b=act_b, leak_b=LEAK, want_f32=True, want_g8=True)
            y = y.cpu().numpy()
            if tol:
                assert rel_l2(y, e) < tol, (what, rel_l2(y, e))
            else:
                msg = R.mismatch_report(y, e.astype(np.float32), 16, 64, what)
                assert not msg, msg
            assert np.array_equal(gpu_ops.from_g8(g).cpu().numpy(), R.g8_roundtrip(y)), what
            if cout % 8:
                assert not g.buf[:, -1, :, :, :, cout % 8:].any().item(), what + ": channels beyond cout are not zero"
