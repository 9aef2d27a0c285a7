"""The planner's fused-convolution step (Session._fused_step) on the MI355X against direct ops calls with the weights packed
by hand per output window, bit for bit: a plain store of two uneven windows (136 outputs = 72 + 64, two segments, batch norm
folded and its scale sliced per window) with pixel norm and with a post-add, a depth-to-space store of two windows
(160 = 128 + 32) and a narrow launch (<= 8 outputs, mpg_conv2d_fused and its small-channel kernel)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WSCALE, EPS = 0.25, 1e-3


def _t(rng, shape):
    return torch.as_tensor(rng.standard_normal(shape).astype(np.float32), device=DEV)


def _conv(G, x, name, k, cout, bn=False):
    """bn?(bias_add(conv2d(x))) with variables under `name`"""
    w = G.get_variable(name + "/weight", [k, k, x.shape[3], cout])
    y = G.bias_add(G.conv2d(x, w, (1, 1), WSCALE), G.get_variable(name + "/bias", [cout], "bias"))
    if bn:
        y = G.batch_norm(y, *[G.get_variable("%s/%s" % (name, kind), [cout], kind)
                              for kind in ("gamma", "beta", "moving_mean", "moving_variance")], eps=EPS)
    return y


def _session(out):
    from mpgan_amd import graph as G, session as S
    sess = S.Session(device=DEV, prec=3, graph=G.get_default_graph())
    sess.vars.ensure(sess.graph)
    return sess, [e for e in sess.plan_summary(out) if e["kind"].startswith("conv2d_")]


def _folded(sess, name, bn):
    """(weight, per-channel scale or None, effective bias in float64) of layer `name`: GAN.py:108-113"""
    v = sess.vars.get
    b = v(name + "/bias").double()
    if not bn:
        return v(name + "/weight"), None, b
    gamma, beta, mean, var = [v("%s/%s" % (name, kind)).double() for kind in ("gamma", "beta", "moving_mean", "moving_variance")]
    s = gamma / torch.sqrt(var + EPS)
    return v(name + "/weight"), s.float().contiguous(), s * (b - mean) + beta


def _window_segments(ops, srcs, layers, co, cw):
    segs = []
    for x8, (w, scale, _) in zip(srcs, layers):
        pk = ops.pack_conv_weights(w[..., co:co + cw].contiguous(), wscale=WSCALE, prec=3,
                                   cout_scale=scale[co:co + cw].contiguous() if scale is not None else None)
        segs.append(ops.Segment(x8, pk))
    return segs


@pytest.mark.parametrize("tail", ["pixel_norm", "post_add"])
def test_plain_step_of_two_uneven_windows(gpu_ops, tail):
    ops = gpu_ops
    from mpgan_amd import graph as G
    G.reset_default_graph()
    try:
        x, s, p = [G.placeholder([1, 8, 8, c], name=nm) for nm, c in (("x", 16), ("s", 8), ("p", 136))]
        out = G.lrelu(G.add(_conv(G, x, "c", 3, 136, bn=True), _conv(G, s, "sc", 1, 136)), leak=0.1)
        out = G.pixel_norm(out, 1e-6) if tail == "pixel_norm" else G.add(out, p)
        sess, plan = _session(out)
    finally:
        G.reset_default_graph()
    assert [(e["kind"], e["cout"], e["launches"], e["prec"], e["pixel_norm"], e["post_add"] is not None) for e in plan] == \
        [("conv2d_fused", 136, 2, 3, tail == "pixel_norm", tail == "post_add")]
    assert [(sg["cin"], sg["kernel"]) for sg in plan[0]["segments"]] == [(16, (3, 3)), (8, (1, 1))]
    rng = np.random.default_rng(136)
    tx, ts, tp = _t(rng, (1, 8, 8, 16)), _t(rng, (1, 8, 8, 8)), _t(rng, (1, 8, 8, 136))
    got = sess.run_device(out, {x: tx, s: ts, p: tp})
    layers = [_folded(sess, "c", True), _folded(sess, "sc", False)]
    srcs = [ops.to_g8(tx), ops.to_g8(ts)]
    windows = ops.wide_chunks(136)
    assert windows == [(0, 72), (72, 64)]
    launches = [(_window_segments(ops, srcs, layers, co, cw), co) for co, cw in windows]
    bias = (layers[0][2] + layers[1][2]).float().contiguous()
    kw = dict(pixel_norm=True, pn_eps=1e-6) if tail == "pixel_norm" else dict(post_add=tp)
    want = ops.conv2d_fused_wide(launches, (8, 8), 136, bias=bias, act="lrelu", leak=0.1, **kw)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (1, 8, 8, 136) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert torch.equal(got, want), "%d of %d values differ" % (int((got != want).sum()), want.numel())


def test_depth_to_space_step_of_two_windows(gpu_ops):
    ops = gpu_ops
    from mpgan_amd import graph as G
    G.reset_default_graph()
    try:
        x = G.placeholder([1, 4, 4, 16], name="x")
        out = G.depth_to_space(_conv(G, x, "ps", 1, 160), 2)
        sess, plan = _session(out)
    finally:
        G.reset_default_graph()
    assert [(e["kind"], e["cout"], e["conv_cout"], e["launches"], e["prec"]) for e in plan] == [("conv2d_fused_d2s", 40, 160, 2, 3)]
    tx = _t(np.random.default_rng(160), (1, 4, 4, 16))
    got = sess.run_device(out, {x: tx})
    layer = _folded(sess, "ps", False)
    chunks = [(_window_segments(ops, [ops.to_g8(tx)], [layer], co, cw), co) for co, cw in ((0, 128), (128, 32))]
    want = ops.conv2d_fused_d2s(chunks, (4, 4), 160, bias=layer[2].float().contiguous())
    torch.cuda.synchronize()
    assert got.shape == want.shape == (1, 8, 8, 40) and float(want.abs().max()) > 0
    assert torch.equal(got, want)


def test_narrow_step_is_one_plain_launch(gpu_ops):
    """<= 8 outputs: the step calls mpg_conv2d_fused (ops.conv2d_fused), the only entry point in front of the small-channel
    kernel, and the tap hands out that very call"""
    ops = gpu_ops
    from mpgan_amd import graph as G
    G.reset_default_graph()
    try:
        x = G.placeholder([1, 8, 8, 4], name="x")
        out = G.relu(_conv(G, x, "n", 3, 8, bn=True))
        sess, plan = _session(out)
    finally:
        G.reset_default_graph()
    assert [(e["kind"], e["cout"], e["prec"]) for e in plan] == [("conv2d_fused", 8, 3)] and "launches" not in plan[0]
    tx = _t(np.random.default_rng(8), (1, 8, 8, 4))
    sess.tap = "n/"
    got = sess.run_device(out, {x: tx})
    sess.tap = None
    layer = _folded(sess, "n", True)
    want = ops.conv2d_fused(_window_segments(ops, [ops.to_g8(tx)], [layer], 0, 8), (8, 8), bias=layer[2].float().contiguous(),
                            act="relu")
    assert sorted(sess.tapped) == sorted(["segments", "out_hw", "bias", "act", "leak", "pixel_norm", "pn_eps", "post_add",
                                          "want_f32", "want_g8"])
    again = ops.conv2d_fused(**sess.tapped)
    torch.cuda.synchronize()
    assert got.shape == (1, 8, 8, 8) and float(want.abs().max()) > 0
    assert torch.equal(got, want) and torch.equal(again, want)
