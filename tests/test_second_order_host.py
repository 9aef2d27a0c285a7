"""tests/second_order_ref.py against torch.autograd on float64 CPU tensors: the d_x formula of the pixel-norm backward, the
max-pool gather and the tanh term are what differentiating x * rsqrt(mean(x^2) + eps), F.max_pool2d and torch.tanh twice gives
(1e-12 relative); the fixed inputs of the end-to-end critic keep their margins; the C ABI and the autograd Functions of the
feature exist (these fail without it).  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elem_ref as E
import second_order_ref as R
from oracle import train_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
TOL = 1e-12


def _close(got, want, scale=None):
    """|got - want| <= 1e-12 of the largest |want|, or of `scale` where the terms of want cancel"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    scale = np.abs(want).max() if scale is None else float(np.max(scale))
    assert np.abs(got - want).max() <= TOL * max(scale, 1e-300), (np.abs(got - want).max(), scale)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=DT, requires_grad=grad)


# ---------------------------------------------------------------------------------------------- the three definitions
@pytest.mark.parametrize("c", R.PN2_C)
def test_pixel_norm_second_derivative_is_autograds(c):
    dy, x, g = R.pn2_data(5, c)
    eps = float(np.float32(R.PN_EPS))
    xt, dt = _t(x, True), _t(dy, True)
    y = xt * torch.rsqrt((xt * xt).mean(-1, keepdim=True) + eps)
    (dx,) = torch.autograd.grad(y, [xt], dt, create_graph=True)
    _close(dx.detach().numpy(), R.pixel_norm_bwd(dy, x))
    g_x, g_dy = torch.autograd.grad((dx * _t(g)).sum(), [xt, dt])
    _close(g_x.numpy(), R.pixel_norm_bwd2(dy, x, g), R.pixel_norm_bwd2_magnitude(dy, x, g))
    _close(g_dy.numpy(), R.pixel_norm_bwd(g, x))                 # the symmetric operator applied to g


def test_pixel_norm_zero_pixel_is_exact_zero_with_bound_zero():
    dy, x, g = R.pn2_data(5, 8)
    x[1] = 0
    ref, bound = R.pixel_norm_bwd2(dy, x, g), R.pixel_norm_bwd2_bound(dy, x, g)
    assert not ref[1].any() and not bound[1].any()
    assert np.all(bound[[0, 2, 3, 4]] > 0)
    assert R.worst_ratio(ref.astype(np.float32), ref, bound) <= 1.0
    with pytest.raises(AssertionError):
        bad = ref.copy()
        bad[1, 0] = 1e-30
        R.worst_ratio(bad, ref, bound)


def _pn2_float32(dy, x, g, eps):
    """the header's float32 order in numpy, with every fmaf as a rounded product and a rounded sum (one rounding more per
    term than the kernel makes)"""
    f = np.float32
    npix, c = x.shape
    lanes = E.pn_lanes(c)
    sums = np.zeros((4, npix, lanes), f)
    for i in range(c):
        l = i % lanes
        for k, (a, b) in enumerate(((x, x), (x, dy), (x, g), (dy, g))):
            sums[k, :, l] = sums[k, :, l] + a[:, i] * b[:, i]
    m = lanes // 2
    while m:
        sums = sums + sums[:, :, np.arange(lanes) ^ m]
        m //= 2
    sxx, sxd, sxg, sdg = (sums[k, :, :1] for k in range(4))
    r = (f(1) / np.sqrt((sxx / f(c) + f(eps)).astype(np.float64))).astype(f)
    s, t, u = sxd / f(c), sxg / f(c), sdg / f(c)
    r2 = r * r
    r3 = r2 * r
    k5 = (((f(3) * r3) * r2) * s) * t
    p = t * dy + (s * g + u * x)
    return k5 * x + -(r3 * p)


@pytest.mark.parametrize("c", R.PN2_C)
def test_pixel_norm_bound_holds_a_float32_evaluation(c):
    dy, x, g = R.pn2_data(257, c)
    y = _pn2_float32(dy, x, g, R.PN_EPS)
    assert y.dtype == np.float32
    ratio = R.worst_ratio(y, R.pixel_norm_bwd2(dy, x, g), R.pixel_norm_bwd2_bound(dy, x, g))
    assert 0.0 < ratio <= 1.0, ratio


def test_pixel_norm_roundings():
    assert [R.pn2_roundings(c) for c in (1, 2, 3, 63, 64, 65, 200)] == [2, 3, 4, 8, 8, 9, 11]


@pytest.mark.parametrize("ks", R.POOL_KS, ids=lambda ks: "k%d-s%d" % ks)
@pytest.mark.parametrize("hw", R.POOL_HW, ids=lambda s: "%dx%d" % s)
def test_max_pool_gather_is_autograds(hw, ks):
    (h, w), (k, s), c = hw, ks, 3
    x = E.normal(31 * h + w + k + s, (R.POOL_N, h, w, c))
    arg = E.max_pool_arg(x, k, s)
    xt = _t(x, True)
    y = F.max_pool2d(xt.permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1)
    dy = E.normal(5, tuple(y.shape))
    g = E.normal(6, x.shape)
    dt = _t(dy, True)
    (dx,) = torch.autograd.grad(y, [xt], dt, create_graph=True)
    assert np.array_equal(dx.detach().numpy(), R.max_pool_bwd(dy, arg, h, w, k, s))
    (g_dy,) = torch.autograd.grad((dx * _t(g)).sum(), [dt])
    assert np.array_equal(g_dy.numpy(), R.max_pool_gather(g, arg, k, s).astype(np.float64))
    # the adjoint identity on small integers, where both sides are exact
    gi, di = E.ints(1, x.shape), E.ints(2, tuple(y.shape))
    lhs = float((R.max_pool_gather(gi, arg, k, s).astype(np.float64) * di).sum())
    assert lhs == float((gi.astype(np.float64) * R.max_pool_bwd(di, arg, h, w, k, s)).sum())


def test_tanh_term_is_autograds():
    rng = np.random.default_rng(8)
    a, dy, g = (rng.standard_normal(1027) for _ in range(3))
    at, dt = _t(a, True), _t(dy, True)
    y = torch.tanh(at)
    (dx,) = torch.autograd.grad(y, [at], dt, create_graph=True)
    g_a, g_dy = torch.autograd.grad((dx * _t(g)).sum(), [at, dt])
    yn = y.detach().numpy()
    # the term reaches `a` through the first backward of tanh once more: d_y (1 - y^2)
    _close(g_a.numpy(), R.tanh_bwd2(dy, yn, g) * (1.0 - yn * yn))
    _close(g_dy.numpy(), g * (1.0 - yn * yn))


@pytest.mark.parametrize("n", R.ACT_N)
def test_tanh_term_float32_order(n):
    dy, y, g = R.act_data(n)
    got, want = R.tanh_bwd2_f32(dy, y, g), R.tanh_bwd2(dy, y, g)
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.all(np.abs(got - want) <= 2.0 * 2.0 ** -24 * np.abs(want) * (1 + 2.0 ** -23))      # two roundings


# ---------------------------------------------------------------------------------------------- the feature is there
def test_entries_are_declared(mpg):
    from mpgan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mpgan.h")).read()
    for name, nargs in (("mpg_act_bwd2", 8), ("mpg_pixel_norm_bwd2", 8), ("mpg_max_pool_gather", 10)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        assert ("int %s(" % name) in header


def test_function_pairs_exist(mpg):
    from mpgan_amd import train, train_ops
    for name in ("MaxPoolBwdFn", "MaxPoolGatherFn", "PixelNorm2Fn", "PixelNormBwdFn", "TanhBwd2Fn"):
        assert issubclass(getattr(train, name), torch.autograd.Function)
    assert "First-order only" in train_ops._MacCormackFn.__doc__


# ---------------------------------------------------------------------------------------------- the end-to-end case
def test_critic_graph_and_fixed_inputs(mpg):
    graph, x, out = R.build_critic()
    assert tuple(out.shape) == (R.CRITIC_SHAPE[0], 1)
    shapes = {n: tuple(s.shape) for n, s in graph.variables.items()}
    assert shapes == {"critic/c1/weight": (3, 3, 3, 8), "critic/c1/bias": (8,), "critic/c2/weight": (3, 3, 8, 12),
                      "critic/c2/bias": (12,), "critic/f1/weight": (48, 5), "critic/f1/bias": (5,),
                      "critic/f2/weight": (5, 1), "critic/f2/bias": (1,)}
    ops_used = set()
    stack = [out]
    while stack:
        n = stack.pop()
        ops_used.add(n.attrs.get("act") if n.op == "act" else n.op)
        stack.extend(n.inputs)
    assert {"tanh", "lrelu", "max_pool", "pixel_norm", "matmul", "conv2d"} <= ops_used
    p = TR.to_params(R.critic_params(graph))
    real, fake, lf = R.critic_inputs()
    assert real.shape == fake.shape == R.CRITIC_SHAPE and lf.shape == (4, 1)
    y_gp = lf.reshape(-1, 1, 1, 1) * real + (np.float32(1.0) - lf.reshape(-1, 1, 1, 1)) * fake
    for name, v in (("real", real), ("fake", fake), ("y_gp", y_gp)):
        gap, lin = R.critic_margins(p, _t(v))
        print("critic margins %-5s pooling %.3e lrelu %.3e" % (name, gap, lin))
        assert gap >= R.POOL_MARGIN and lin >= R.LRELU_MARGIN, (name, gap, lin)
    L = R.wgan_gp_losses(lambda t: R.critic(p, t), _t(real), _t(fake), _t(lf))
    grads = TR.grads(L["disc_loss"], p, "critic")
    assert sorted(grads) == sorted(n for n in shapes)
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in grads.values())
    assert float(L["grad_penalty_d"].detach()) > 0
