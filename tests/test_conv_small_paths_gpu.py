"""The paths inside conv_small_kernel and conv_small_pair_kernel (mpgan_conv_small.hip): filter sizes known to the
compiler (5x5, 1x1) against the run-time form, a segment's own channel bound against the launch's, the pair launch
against two launches.

An output of these kernels is one chain of fmaf over segments, then filter columns, then filter rows, then input
channels, so two launches whose chains differ only by terms x * 0 (a zero weight) must agree BIT FOR BIT: such a term
leaves the sum as it is, and a sum that starts at +0 never becomes -0.  The same layers are also held to the float64
oracle at the 1e-5 of tests/test_kernels_gpu.py.

Every case has at least two 64 x 16 tiles in x and in y, both ragged.

The pair launch keeps its middle tensor in fp32; the two-launch form passes it on as G8 (fp16 hi + fp16 lo).  The two
can agree bit for bit only where the middle tensor is exact in G8, so in that comparison the input, filter A and bias
A lie on a grid of small integers (the middle values are integers / 8 below 2^11: exact in the hi plane alone), while
filter B, the shortcut and bias B are general.  General data for the same pair launches is in the oracle test below.
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import ops as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, H, W = 2, 19, 70
WS = 0.0625          # one power of two for every filter: a zero-embedded filter is packed with the same values


def _t(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device=DEV)      # (a copy: the shared arrays are read-only)


def _embed(w, kh, kw):
    """the filter centred in a kh x kw filter of zeros: the same SAME convolution"""
    out = np.zeros((kh, kw) + w.shape[2:], np.float32)
    oy, ox = (kh - w.shape[0]) // 2, (kw - w.shape[1]) // 2
    out[oy:oy + w.shape[0], ox:ox + w.shape[1]] = w
    return out


def _same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2100)
    d = dict(
        x8=rng.standard_normal((N, H, W, 8)).astype(np.float32),
        x2=rng.standard_normal((N, H, W, 2)).astype(np.float32),
        w82=rng.standard_normal((5, 5, 8, 2)).astype(np.float32),
        w21=rng.standard_normal((5, 5, 2, 1)).astype(np.float32),
        ws81=rng.standard_normal((1, 1, 8, 1)).astype(np.float32),
        b2=rng.standard_normal(2).astype(np.float32),
        b1=rng.standard_normal(1).astype(np.float32),
    )
    for v in d.values():
        v.setflags(write=False)
    return d


def _layer(ops, segs, bias, want_g8=True):
    """segs: [(x fp32 NHWC, w HWIO)]; relu(sum conv + bias) as (fp32, G8 as fp32)"""
    ss = [ops.Segment(_t(x), ops.pack_conv_weights(_t(w), wscale=WS, prec=2)) for x, w in segs]
    y, g = ops.conv2d_fused(ss, (H, W), bias=_t(bias), act="relu", want_f32=True, want_g8=True)
    return y, ops.from_g8(g)


def test_5x5_against_runtime_7x7_8to2(gpu_ops, data):
    y5, g5 = _layer(gpu_ops, [(data["x8"], data["w82"])], data["b2"])
    y7, g7 = _layer(gpu_ops, [(data["x8"], _embed(data["w82"], 7, 7))], data["b2"])
    assert _same(y5, y7) and _same(g5, g7)


def test_5x5_and_1x1_against_runtime_sizes_2to1_shortcut(gpu_ops, data):
    y5, g5 = _layer(gpu_ops, [(data["x2"], data["w21"]), (data["x8"], data["ws81"])], data["b1"])
    y7, g7 = _layer(gpu_ops, [(data["x2"], _embed(data["w21"], 7, 7)), (data["x8"], _embed(data["ws81"], 3, 3))], data["b1"])
    assert _same(y5, y7) and _same(g5, g7)


def test_segment_channel_bound_against_common_bound(gpu_ops, data):
    """2 -> 1 + shortcut from 8: the 2-channel input as an 8-channel tensor with six zero channels and zero weight rows
    runs every segment at the bound of 8"""
    x2w = np.concatenate([data["x2"], np.zeros((N, H, W, 6), np.float32)], axis=3)
    w2w = np.concatenate([data["w21"], np.zeros((5, 5, 6, 1), np.float32)], axis=2)
    ya, ga = _layer(gpu_ops, [(data["x2"], data["w21"]), (data["x8"], data["ws81"])], data["b1"])
    yb, gb = _layer(gpu_ops, [(x2w, w2w), (data["x8"], data["ws81"])], data["b1"])
    assert _same(ya, yb) and _same(ga, gb)


PAIR_UP = [(2, 0), (2, 1)]       # up_log2, up_x_only


@pytest.fixture(scope="module")
def pair_data():
    rng = np.random.default_rng(2101)
    d = dict(
        grid=dict(xl=rng.integers(-3, 4, (N, 20, 18, 1)).astype(np.float32),          # 20 x 18: rows stay, columns x4
                  wa=rng.integers(-3, 4, (5, 5, 1, 2)).astype(np.float32) * 2.0,       # times WS: integers / 8
                  ba=rng.integers(-8, 9, 2).astype(np.float32) / 8.0),
        general=dict(xl=rng.standard_normal((N, 20, 18, 1)).astype(np.float32),
                     wa=rng.standard_normal((5, 5, 1, 2)).astype(np.float32),
                     ba=rng.standard_normal(2).astype(np.float32)),
        wb=rng.standard_normal((5, 5, 2, 8)).astype(np.float32),
        wsc=rng.standard_normal((1, 1, 1, 8)).astype(np.float32),
        bb=rng.standard_normal(8).astype(np.float32),
    )
    return d


def _pair(ops, d, kind, up, xonly):
    h, w = 20, 72
    f = d[kind]
    xl = f["xl"] if xonly else f["xl"][:, :5]         # [N, 20, 18] or [N, 5, 18]
    pk = lambda t: ops.pack_conv_weights(_t(t), wscale=WS, prec=2)
    xg = ops.to_g8(_t(xl))
    y, g = ops.conv2d_small_pair(xg, 0, up, pk(f["wa"]), pk(d["wb"]), pk(d["wsc"]), (h, w), bias_a=_t(f["ba"]), act_a="relu",
                                 bias_b=_t(d["bb"]), act_b="relu", want_f32=True, want_g8=True, up_x_only=xonly)
    return xl, xg, y, ops.from_g8(g)


@pytest.mark.parametrize("up,xonly", PAIR_UP)
def test_pair_against_two_launches(gpu_ops, pair_data, up, xonly):
    d, f = pair_data, pair_data["grid"]
    h, w = 20, 72
    xl, xg, y, g = _pair(gpu_ops, d, "grid", up, xonly)
    pk = lambda t: gpu_ops.pack_conv_weights(_t(t), wscale=WS, prec=2)
    seg = lambda src, t: gpu_ops.Segment(src, pk(t), up_log2=up, up_x_only=xonly)
    mid = gpu_ops.conv2d_fused([seg(xg, f["wa"])], (h, w), bias=_t(f["ba"]), act="relu", want_f32=False, want_g8=True)
    y2, g2 = gpu_ops.conv2d_fused([gpu_ops.Segment(mid, pk(d["wb"])), seg(xg, d["wsc"])], (h, w), bias=_t(d["bb"]), act="relu",
                                  want_f32=True, want_g8=True)
    assert float(y.abs().max()) > 0
    assert _same(y, y2) and _same(g, gpu_ops.from_g8(g2))


def _ref_layer(segs, bias):
    acc = None
    for x, w in segs:
        c = O.conv2d_same(x, w * np.float32(WS)).astype(np.float64)
        acc = c if acc is None else acc + c
    return O.relu(O.bias_add(acc.astype(np.float32), bias))


ORACLE_LAYERS = ["8to2", "2to1_shortcut", "3x3", "1x7"]


@pytest.mark.parametrize("name", ORACLE_LAYERS)
def test_layers_against_oracle(gpu_ops, data, name):
    rng = np.random.default_rng(2102)
    if name == "8to2":
        segs, bias = [(data["x8"], data["w82"])], data["b2"]
    elif name == "2to1_shortcut":
        segs, bias = [(data["x2"], data["w21"]), (data["x8"], data["ws81"])], data["b1"]
    elif name == "3x3":
        segs, bias = [(data["x8"], rng.standard_normal((3, 3, 8, 2)).astype(np.float32))], data["b2"]
    else:
        segs, bias = [(data["x2"], rng.standard_normal((1, 7, 2, 1)).astype(np.float32))], data["b1"]
    y, g = _layer(gpu_ops, segs, bias)
    ref = _ref_layer(segs, bias)
    err_y, err_g = rel_l2(y.cpu().numpy(), ref), rel_l2(g.cpu().numpy(), ref)
    print("%s: rel L2 vs oracle fp32 %.3e, G8 %.3e" % (name, err_y, err_g))
    assert err_y < 1e-5 and err_g < 1e-5


@pytest.mark.parametrize("up,xonly", PAIR_UP)
def test_pair_against_oracle(gpu_ops, pair_data, up, xonly):
    d, f = pair_data, pair_data["general"]
    h, w = 20, 72
    xl, xg, y, g = _pair(gpu_ops, d, "general", up, xonly)
    x = O.resize_nearest_tf1(xl, h, w)
    mid = O.relu(O.bias_add(O.conv2d_same(x, f["wa"] * np.float32(WS)), f["ba"]))
    ref = _ref_layer([(mid, d["wb"]), (x, d["wsc"])], d["bb"])
    err_y, err_g = rel_l2(y.cpu().numpy(), ref), rel_l2(g.cpu().numpy(), ref)
    print("pair up %d x-only %d: rel L2 vs oracle fp32 %.3e, G8 %.3e" % (up, xonly, err_y, err_g))
    assert err_y < 1e-5 and err_g < 1e-5
