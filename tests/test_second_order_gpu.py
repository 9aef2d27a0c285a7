"""Gradient penalties through tanh, max pool and pixel norm: the kernels mpg_act_bwd2, mpg_pixel_norm_bwd2 and
mpg_max_pool_gather, the autograd Function pairs of train.py / train_ops.py that use them, and a critic of these layers built
with the public GAN builder and trained through TrainSession with the WGAN-GP loss, all against tests/second_order_ref.py
(checked on the CPU by test_second_order_host.py).

* exact: mpg_act_bwd2 against float32 numpy in the header's order, mpg_max_pool_gather against the restatement and in the
  adjoint identity on integers, the max-pool pair to third order on integer cotangents.
* bounded: mpg_pixel_norm_bwd2 elementwise within pixel_norm_bwd2_bound (derived next to the kernel).  Every case prints
  "second-order-error <case> <worst err / bound>"; profiles/second_order/errors.txt is their collection on an MI355X.  A ratio
  above 1 is a defect of the kernel or of the derivation, never a reason for a larger factor.
* the critic: loss and every parameter gradient against float64 autograd at the tolerances of
  test_train8x_gpu.py (test_growing_nets_forward :50, test_wgan_gp_gradients :76-79)."""
import math

import numpy as np
import pytest
import torch

import elem_ref as E
import second_order_ref as R
from oracle import train_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ZONE = 64               # floats of sentinel in front of and behind an output
SENTINEL = 12345.0


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _t_u8(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.uint8, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _at_offset(a, off):
    """a copy of `a` on the device whose first element lies 4 * off bytes behind a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=F32)
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off
    return v


def _guarded(shape, off):
    """(whole buffer, output view): the view full of NaN at 4 * off bytes behind a 16-byte boundary, ZONE sentinels on either
    side"""
    n = int(np.prod(shape))
    buf = torch.full((off + ZONE + n + ZONE,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[off + ZONE:off + ZONE + n].view(shape)
    out.fill_(float("nan"))
    return buf, out


def _check_guarded(buf, out, off):
    flat = _np(buf)
    n = out.numel()
    assert np.all(flat[:off + ZONE] == SENTINEL) and np.all(flat[off + ZONE + n:] == SENTINEL), "wrote outside the output"
    assert not np.isnan(flat[off + ZONE:off + ZONE + n]).any(), "an output element was not written"


def _bounded(name, y, ref, bound):
    assert y.shape == ref.shape == bound.shape, (name, y.shape, ref.shape, bound.shape)
    ratio = R.worst_ratio(y, ref, bound)
    print("second-order-error %-50s %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: worst err / bound %.3f" % (name, ratio)


@pytest.fixture(scope="module")
def tops(gpu_ops):
    from mpgan_amd import train_ops
    return train_ops


@pytest.fixture(scope="module")
def lib(gpu_ops):
    from mpgan_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------- mpg_pixel_norm_bwd2
@pytest.mark.parametrize("npix", R.PN2_NPIX)
@pytest.mark.parametrize("c", R.PN2_C, ids=lambda c: "c%d-lanes%d" % (c, E.pn_lanes(c)))
def test_pixel_norm_bwd2_bounded(tops, c, npix):
    dy, x, g = R.pn2_data(npix, c)
    got = _np(tops.pixel_norm_bwd2(_t(dy), _t(x), _t(g), R.PN_EPS))
    _bounded("pixel_norm_bwd2 c%d npix%d" % (c, npix), got, R.pixel_norm_bwd2(dy, x, g), R.pixel_norm_bwd2_bound(dy, x, g))


def test_pixel_norm_bwd2_of_zeros_is_zero(tops):
    """x = 0 throughout: r = rsqrt(eps) = 1e4 and r^5 = 1e20 stay finite, s = t = 0, and every term carries a factor 0"""
    dy, x, g = R.pn2_data(5, 8)
    x[:] = 0
    got = _np(tops.pixel_norm_bwd2(_t(dy), _t(x), _t(g), 1e-8))
    assert not got.any()
    _bounded("pixel_norm_bwd2 zeros", got, R.pixel_norm_bwd2(dy, x, g, 1e-8), R.pixel_norm_bwd2_bound(dy, x, g, 1e-8))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
@pytest.mark.parametrize("c", R.PN2_C, ids=lambda c: "c%d" % c)
def test_pixel_norm_bwd2_writes_its_output_only_and_repeats_its_bits(lib, tops, c, off):
    from mpgan_amd.ops import _ptr, _stream
    npix = 257
    dy, x, g = R.pn2_data(npix, c)
    dyt, xt, gt = (_at_offset(a, off) for a in (dy, x, g))
    outs = []
    for _ in range(2):
        buf, out = _guarded((npix, c), off)
        lib.check(lib.load().mpg_pixel_norm_bwd2(_stream(), _ptr(dyt), _ptr(xt), _ptr(gt), npix, c, R.PN_EPS, _ptr(out)),
                  "mpg_pixel_norm_bwd2")
        _check_guarded(buf, out, off)
        outs.append(_np(out))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.array_equal(_bits(outs[0]), _bits(_np(tops.pixel_norm_bwd2(_t(dy), _t(x), _t(g), R.PN_EPS))))


def test_pixel_norm_bwd2_refusals(lib):
    from mpgan_amd.ops import _ptr, _stream
    fn = lib.load().mpg_pixel_norm_bwd2
    a = torch.ones((4, 8), dtype=torch.float32, device=DEV)
    out = torch.full((4, 8), 7.0, dtype=torch.float32, device=DEV)
    for args in ((_ptr(None), _ptr(a), _ptr(a), 4, 8), (_ptr(a), _ptr(None), _ptr(a), 4, 8), (_ptr(a), _ptr(a), _ptr(None), 4, 8),
                 (_ptr(a), _ptr(a), _ptr(a), 0, 8), (_ptr(a), _ptr(a), _ptr(a), 4, 0)):
        with pytest.raises(lib.MpgError):
            lib.check(fn(_stream(), args[0], args[1], args[2], args[3], args[4], 1e-8, _ptr(out)), "mpg_pixel_norm_bwd2")
    with pytest.raises(lib.MpgError):
        lib.check(fn(_stream(), _ptr(a), _ptr(a), _ptr(a), 4, 8, 1e-8, _ptr(None)), "mpg_pixel_norm_bwd2")
    assert torch.all(out == 7.0)


# ---------------------------------------------------------------------------------------------- mpg_max_pool_gather
@pytest.mark.parametrize("c", R.POOL_C)
@pytest.mark.parametrize("ks", R.POOL_KS, ids=lambda ks: "k%d-s%d" % ks)
@pytest.mark.parametrize("hw", R.POOL_HW, ids=lambda s: "%dx%d" % s)
def test_max_pool_gather_exact_and_adjoint(lib, tops, hw, ks, c):
    from mpgan_amd.ops import _ptr, _stream
    (h, w), (k, s) = hw, ks
    arg = R.pool_arg(h, w, c, k, s)
    g = E.normal(3, (R.POOL_N, h, w, c))
    want = R.max_pool_gather(g, arg, k, s)
    gt, argt = _t(g), _t_u8(arg)
    assert np.array_equal(_bits(_np(tops.max_pool_gather(gt, argt, k, s))), _bits(want))
    buf, out = _guarded(arg.shape, 0)                    # the entry itself: every output written, nothing else
    lib.check(lib.load().mpg_max_pool_gather(_stream(), _ptr(gt), _ptr(argt), R.POOL_N, h, w, c, k, s, _ptr(out)),
              "mpg_max_pool_gather")
    _check_guarded(buf, out, 0)
    assert np.array_equal(_bits(_np(out)), _bits(want))
    # <gather(g), dy> == <g, max_pool_bwd(dy)> on small integers: every product and sum is exact
    gi, di = E.ints(1, (R.POOL_N, h, w, c)), E.ints(2, arg.shape)
    lhs = (_np(tops.max_pool_gather(_t(gi), _t_u8(arg), k, s)).astype(np.float64) * di).sum()
    rhs = (gi.astype(np.float64) * _np(tops.max_pool_bwd(_t(di), _t_u8(arg), h, w, k, s))).sum()
    assert lhs == rhs


def test_max_pool_gather_refusals(lib, tops):
    from mpgan_amd.ops import _ptr, _stream
    fn = lib.load().mpg_max_pool_gather
    g = torch.ones((1, 8, 8, 2), dtype=torch.float32, device=DEV)
    arg = torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device=DEV)              # room for every geometry below
    out = torch.full((1, 8, 8, 2), 7.0, dtype=torch.float32, device=DEV)
    for n, h, w, c, k, s in ((0, 8, 8, 2, 2, 2), (1, 8, 8, 0, 2, 2), (1, 8, 8, 2, 0, 2), (1, 8, 8, 2, 16, 1), (1, 8, 8, 2, 2, 0),
                             (1, 2, 8, 2, 3, 1), (1, 8, 2, 2, 3, 1)):
        with pytest.raises(lib.MpgError):
            lib.check(fn(_stream(), _ptr(g), _ptr(arg), n, h, w, c, k, s, _ptr(out)), "mpg_max_pool_gather")
    for ptrs in ((None, arg, out), (g, None, out), (g, arg, None)):
        with pytest.raises(lib.MpgError):
            lib.check(fn(_stream(), _ptr(ptrs[0]), _ptr(ptrs[1]), 1, 8, 8, 2, 2, 2, _ptr(ptrs[2])), "mpg_max_pool_gather")
    assert torch.all(out == 7.0)
    with pytest.raises(lib.MpgError):                           # the wrapper: an index plane of another geometry
        tops.max_pool_gather(g, arg, 2, 2)


# ---------------------------------------------------------------------------------------------- mpg_act_bwd2
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
@pytest.mark.parametrize("n", R.ACT_N)
def test_act_bwd2_tanh_exact(lib, tops, n, off):
    from mpgan_amd.ops import _ptr, _stream
    dy, y, g = R.act_data(n)
    want = R.tanh_bwd2_f32(dy, y, g)
    dyt, yt, gt = (_at_offset(a, off) for a in (dy, y, g))
    buf, out = _guarded((n,), off)
    lib.check(lib.load().mpg_act_bwd2(_stream(), _ptr(dyt), _ptr(yt), _ptr(gt), n, lib.ACT_TANH, 0.2, _ptr(out)), "mpg_act_bwd2")
    _check_guarded(buf, out, off)
    assert np.array_equal(_bits(_np(out)), _bits(want))
    assert np.array_equal(_bits(_np(tops.act_bwd2(_t(dy), _t(y), _t(g), "tanh"))), _bits(want))


@pytest.mark.parametrize("act", ["relu", "lrelu", None])
def test_act_bwd2_refuses_what_is_not_tanh(lib, tops, act):
    """MPG_ERR_ARG from the host before any launch: the output keeps what it held"""
    from mpgan_amd.ops import _ptr, _stream
    dy, y, g = (_t(a) for a in R.act_data(5))
    with pytest.raises(lib.MpgError):
        tops.act_bwd2(dy, y, g, act)
    out = torch.full((5,), 7.0, dtype=torch.float32, device=DEV)
    rc = lib.load().mpg_act_bwd2(_stream(), _ptr(dy), _ptr(y), _ptr(g), 5, lib.act_id(act), 0.2, _ptr(out))
    torch.cuda.synchronize()
    assert rc != lib.MPG_OK and torch.all(out == 7.0)
    assert lib.load().mpg_act_bwd2(_stream(), _ptr(dy), _ptr(y), _ptr(None), 5, lib.ACT_TANH, 0.2, _ptr(out)) != lib.MPG_OK


# ---------------------------------------------------------------------------------------------- the Functions
def _second(y, x, dy, w):
    """phi = sum w * (the backward of y in x for the upstream dy) -> (that backward, d phi / d x, d phi / d dy)"""
    (dx,) = torch.autograd.grad(y, [x], dy, create_graph=True)
    g_x, g_dy = torch.autograd.grad((dx * w).sum(), [x, dy], allow_unused=True)
    return dx.detach(), g_x, g_dy


@pytest.mark.parametrize("c", (3, 65))
def test_pixel_norm_function_second_order(gpu_ops, tops, c):
    from mpgan_amd.train import PixelNorm2Fn
    npix = 37
    dy, x, w = R.pn2_data(npix, c)
    xt, dyt = _t(x).requires_grad_(True), _t(dy).requires_grad_(True)
    dx, g_x, g_dy = _second(PixelNorm2Fn.apply(xt, R.PN_EPS), xt, dyt, _t(w))
    assert torch.equal(dx, tops.pixel_norm_bwd(_t(dy), _t(x), R.PN_EPS))               # the first-order step's own call
    _bounded("PixelNorm2Fn d/dx c%d" % c, _np(g_x), R.pixel_norm_bwd2(dy, x, w), R.pixel_norm_bwd2_bound(dy, x, w))
    _bounded("PixelNorm2Fn d/ddy c%d" % c, _np(g_dy), R.pixel_norm_bwd(w, x), E.pixel_norm_bwd_bound(w, x))


def test_pixel_norm_twin_has_the_bits_of_the_first_order_function(gpu_ops):
    """PixelNorm2Fn (inside higher_order_scopes) and PixelNormFn (everywhere else) call the same kernels: the same output and
    the same first gradient, bit for bit; and the twin's second-order term reaches an input that is a view"""
    from mpgan_amd.train import PixelNorm2Fn, PixelNormFn
    dy, x, w = R.pn2_data(37, 8)
    outs = []
    for fn in (PixelNormFn, PixelNorm2Fn):
        xt = _t(x).requires_grad_(True)
        y = fn.apply(xt, R.PN_EPS)
        (dx,) = torch.autograd.grad(y, [xt], _t(dy))
        outs.append((y.detach(), dx))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    base = _t(np.concatenate([x, x], axis=1)).requires_grad_(True)
    dyt = _t(dy).requires_grad_(True)
    view = base[:, :8]                                               # not contiguous
    (dx,) = torch.autograd.grad(PixelNorm2Fn.apply(view, R.PN_EPS), [view], dyt, create_graph=True)
    (g_base,) = torch.autograd.grad((dx * _t(w)).sum(), [base])
    _bounded("PixelNorm2Fn d/dx through a view", _np(g_base[:, :8]), R.pixel_norm_bwd2(dy, x, w), R.pixel_norm_bwd2_bound(dy, x, w))
    assert not g_base[:, 8:].any()


def test_pixel_norm_function_refuses_a_third_derivative(gpu_ops):
    """PixelNormBwdFn's backward is kernel calls without a tape: a third derivative raises, it does not read as zero (w is a
    variable too, so that the second gradient carries that backward's node)"""
    from mpgan_amd.train import PixelNorm2Fn
    dy, x, w = R.pn2_data(5, 8)
    xt, dyt, wt = (_t(a).requires_grad_(True) for a in (x, dy, w))
    (dx,) = torch.autograd.grad(PixelNorm2Fn.apply(xt, R.PN_EPS), [xt], dyt, create_graph=True)
    (g_x,) = torch.autograd.grad((dx * wt).sum(), [xt], create_graph=True)
    assert g_x.grad_fn is not None
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g_x.sum().backward()


def test_tanh_function_second_order(gpu_ops):
    """ActFn with tanh: d phi / d dy = w (1 - y^2), d phi / d a = (-2 y dy w)(1 - y^2) on the y the forward produced.
    Roundings: 1 - y^2 is off by at most 2^-24 absolute (y^2 + |1 - y^2| = 1), each product by 2^-24 relative, d_y carries
    two: |error| <= 2^-23 |w| and 2 x 2^-23 |d_y|"""
    from mpgan_amd.train import ActFn
    rng = np.random.default_rng(21)
    a, dy, w = (rng.standard_normal((2, 5, 7, 3)).astype(F32) for _ in range(3))
    at, dyt = _t(a).requires_grad_(True), _t(dy).requires_grad_(True)
    y = ActFn.apply(at, None, "tanh", 0.2)
    dx, g_a, g_dy = _second(y, at, dyt, _t(w))
    yn = _np(y).astype(np.float64)
    d = 1.0 - yn * yn
    d_y = R.tanh_bwd2(dy, _np(y), w)
    _bounded("ActFn tanh d/ddy", _np(g_dy), w * d, R.U23 * np.abs(w.astype(np.float64)))
    _bounded("ActFn tanh d/da", _np(g_a), d_y * d, 2.0 * R.U23 * np.abs(d_y))
    assert float(np.abs(_np(g_a)).max()) > 0


def test_tanh_function_refuses_a_third_derivative(gpu_ops):
    from mpgan_amd.train import ActFn
    rng = np.random.default_rng(22)
    a, dy, w = (rng.standard_normal((1, 4, 4, 2)).astype(F32) for _ in range(3))
    at, dyt = _t(a).requires_grad_(True), _t(dy).requires_grad_(True)
    (dx,) = torch.autograd.grad(ActFn.apply(at, None, "tanh", 0.2), [at], dyt, create_graph=True)
    (g_a,) = torch.autograd.grad((dx * _t(w)).sum(), [at], create_graph=True)
    with pytest.raises(NotImplementedError, match="third-order"):
        g_a.sum().backward()


@pytest.mark.parametrize("act", ["relu", "lrelu"])
def test_piecewise_linear_activations_send_nothing_to_y(gpu_ops, act):
    from mpgan_amd.train import ActBwdFn
    rng = np.random.default_rng(23)
    dy, y, w = (_t(rng.standard_normal((1, 4, 4, 2)).astype(F32)) for _ in range(3))
    dy.requires_grad_(True)
    y.requires_grad_(True)
    g_dy, g_y = torch.autograd.grad((ActBwdFn.apply(dy, y, act, 0.2) * w).sum(), [dy, y], allow_unused=True)
    assert g_y is None and g_dy is not None


@pytest.mark.parametrize("ks", ((2, 2), (3, 2)), ids=lambda ks: "k%d-s%d" % ks)
def test_max_pool_function_to_third_order(gpu_ops, tops, ks):
    """MaxPoolFn -> MaxPoolBwdFn -> MaxPoolGatherFn -> MaxPoolBwdFn on integer cotangents (overlapping windows add exactly)"""
    from mpgan_amd.train import MaxPoolFn
    (k, s), (n, h, w, c) = ks, (2, 7, 5, 3)
    x = E.normal(41, (n, h, w, c))
    arg = E.max_pool_arg(x, k, s)
    dy, wgt, z = E.ints(1, arg.shape), E.ints(2, x.shape), E.ints(3, arg.shape)
    xt, dyt, wt = _t(x).requires_grad_(True), _t(dy).requires_grad_(True), _t(wgt).requires_grad_(True)
    (dx,) = torch.autograd.grad(MaxPoolFn.apply(xt, k, s), [xt], dyt, create_graph=True)
    assert np.array_equal(_np(dx), R.max_pool_bwd(dy, arg, h, w, k, s))
    g_x, g_dy = torch.autograd.grad((dx * wt).sum(), [xt, dyt], create_graph=True, allow_unused=True)
    assert g_x is None                                              # the selection is fixed: nothing goes to x
    assert np.array_equal(_np(g_dy), R.max_pool_gather(wgt, arg, k, s))
    (g_w,) = torch.autograd.grad((g_dy * _t(z)).sum(), [wt])
    assert np.array_equal(_np(g_w), R.max_pool_bwd(z, arg, h, w, k, s))


# ---------------------------------------------------------------------------------------------- end to end
def test_critic_wgan_gp_loss_and_gradients(gpu_ops):
    """the critic of second_order_ref.build_critic under higher_order_scopes: tanh, both max pools (one with overlapping
    windows), lrelu, pixel norm and the two fully connected layers differentiated twice by the gradient penalty"""
    from mpgan_amd.session import VariableStore
    from mpgan_amd.train import TrainSession
    graph, x, out = R.build_critic()
    sess = TrainSession(VariableStore(DEV, seed=1), graph=graph, device=DEV, higher_order_scopes=("critic",))
    params = R.critic_params(graph)
    with torch.no_grad():
        for nme, t in sess.parameters().items():
            t.copy_(torch.as_tensor(params[nme], device=DEV))
    real, fake, lf = R.critic_inputs()
    L = R.wgan_gp_losses(lambda t: sess.run([out], {x: t})[0], _t(real), _t(fake), _t(lf))
    names = sorted(sess.trainable("critic"))
    got = torch.autograd.grad(L["disc_loss"], [sess.params[nme] for nme in names])
    p = TR.to_params(params)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)                    # noqa: E731
    Lr = R.wgan_gp_losses(lambda t: R.critic(p, t), t64(real), t64(fake), t64(lf))
    want = TR.grads(Lr["disc_loss"], p, "critic")
    assert sorted(want) == names and len(names) == 8
    for k in ("d_loss_y", "d_loss_g", "epsilon_penalty_d", "grad_penalty_d", "disc_loss"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        print("critic %-18s %.6f vs %.6f" % (k, a, b))
        assert abs(a - b) <= 2e-4 * max(abs(b), 1e-2), (k, a, b)
    tot_d = tot_r = 0.0
    for nme, g in zip(names, got):
        wnt = want[nme]
        gnp = _np(g).astype(np.float64)
        r = float(np.linalg.norm(gnp - wnt) / max(np.linalg.norm(wnt), 1e-30))
        print("critic gradient %-20s rel %.3e" % (nme, r))
        assert np.abs(wnt).max() > 0 and r < 5e-3, (nme, r)
        tot_d += float(((gnp - wnt) ** 2).sum())
        tot_r += float((wnt ** 2).sum())
    print("critic aggregate gradient error %.3e" % math.sqrt(tot_d / tot_r))
    assert math.sqrt(tot_d / tot_r) < 3e-4
