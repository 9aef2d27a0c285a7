"""Training-step kernels and the 4x GAN iteration against the float64 autograd restatement
(oracle/train_ref.py).  Tolerances: fp32 kernels 1e-5 relative L2 (accumulation order differs);
layers whose forward / data gradient run on the MFMA kernel at F16X3 2e-5; whole-network gradients
1e-3 per tensor (ReLU gates of near-zero pre-activations may flip), 1e-4 on the losses."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train_ref as TR
from oracle.nets import ParamSource
from oracle.ops import same_pad

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def ref_conv_grads(x, w, dy, stride, wscale):
    """float64 autograd of tf.nn.conv2d SAME: x NHWC, w HWIO, dy NHWC -> (dx, dw)"""
    xt = torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.tensor(w, dtype=torch.float64).requires_grad_(True)
    _, pt, pb = same_pad(x.shape[1], w.shape[0], stride)
    _, pl, pr = same_pad(x.shape[2], w.shape[1], stride)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), (wt * wscale).permute(3, 2, 0, 1).contiguous(), stride=stride)
    y.backward(torch.tensor(dy, dtype=torch.float64).permute(0, 3, 1, 2))
    return xt.grad.permute(0, 2, 3, 1).numpy(), wt.grad.numpy()


GRAD_CASES = [
    # n, h, w, cin, cout, k, stride
    (2, 16, 16, 4, 8, 5, 1),
    (2, 16, 16, 32, 128, 5, 1),
    (1, 24, 20, 128, 128, 3, 1),
    (3, 8, 8, 128, 32, 5, 1),
    (2, 16, 16, 8, 1, 5, 1),
    (2, 16, 16, 1, 2, 5, 1),
    (2, 12, 12, 9, 17, 1, 1),
    (2, 16, 16, 2, 32, 4, 2),
    (2, 16, 16, 32, 64, 4, 2),
    (2, 9, 7, 64, 128, 4, 2),
    (2, 8, 8, 128, 256, 4, 1),
    (4, 1, 1, 1024, 1, 1, 1),
]


@pytest.mark.parametrize("case", GRAD_CASES)
def test_conv_wgrad_dgrad(case):
    from mpgan_amd import train_ops
    n, h, w, cin, cout, k, s = case
    rng = np.random.default_rng(hash(case) % 2 ** 31)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = rng.standard_normal((k, k, cin, cout)).astype(np.float32)
    oh, ow = -(-h // s), -(-w // s)
    dy = rng.standard_normal((n, oh, ow, cout)).astype(np.float32)
    wscale = float(np.float32(math.sqrt(2.0) / math.sqrt(k * k * cin)))
    dx_ref, dw_ref = ref_conv_grads(x, wt, dy, s, wscale)
    dw = train_ops.conv2d_wgrad(dev(x), dev(dy), k, k, (s, s), wscale).cpu().numpy()
    dx = train_ops.conv2d_dgrad(dev(dy), dev(wt), (h, w), (s, s), wscale).cpu().numpy()
    assert dw.shape == dw_ref.shape and dx.shape == dx_ref.shape
    assert rel(dw, dw_ref) < 1e-5
    assert rel(dx, dx_ref) < 1e-5


WG_MFMA_CASES = [
    # n, h, w, cin, cout, k
    (2, 16, 16, 4, 8, 5), (2, 16, 16, 32, 128, 5), (1, 24, 20, 128, 128, 3), (3, 8, 8, 128, 32, 5),
    (2, 16, 16, 8, 1, 5), (2, 16, 16, 1, 2, 5), (2, 12, 12, 9, 17, 1), (2, 8, 8, 128, 256, 4),
    (1, 32, 64, 128, 128, 5), (2, 16, 40, 64, 96, 5), (1, 8, 300, 33, 65, 3), (2, 64, 64, 8, 32, 5),
    (2, 16, 16, 200, 40, 1), (1, 16, 16, 40, 72, 4),
    # the ring form (all filter rows of a tile in one block): ragged row ranges (20 rows in ranges of 10), ragged columns
    # (70 = one chunk of 64 + 6), channel groups and cout tiles that do not exist, a ring that wraps many times
    (1, 20, 70, 40, 40, 5), (1, 9, 17, 8, 8, 3), (2, 33, 65, 130, 70, 3), (1, 16, 48, 32, 64, 4), (1, 70, 20, 16, 96, 5),
    # shapes that stay on the one-filter-row kernel: 1 x 1 and non-square filters are not in this list (kh == kw here)
]


@pytest.mark.parametrize("prec", [3, 1])
@pytest.mark.parametrize("case", WG_MFMA_CASES)
def test_conv_wgrad_mfma(case, prec):
    """matrix-core weight gradient vs float64 autograd: 3-product mode fp32-grade, 1-product fp16-grade"""
    from mpgan_amd import train_ops
    n, h, w, cin, cout, k = case
    rng = np.random.default_rng(hash(case) % 2 ** 31)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = rng.standard_normal((k, k, cin, cout)).astype(np.float32)
    dy = (rng.standard_normal((n, h, w, cout)) * 1e-6).astype(np.float32)      # small gradients: exercises the scaling
    wscale = float(np.float32(math.sqrt(2.0) / math.sqrt(k * k * cin)))
    _, dw_ref = ref_conv_grads(x, wt, dy, 1, wscale)
    dw = train_ops.conv2d_wgrad_mfma(dev(x), dev(dy), k, k, wscale, prec).cpu().numpy()
    assert dw.shape == dw_ref.shape
    assert rel(dw, dw_ref) < (2e-6 if prec == 3 else 2e-3)
    # the training step's call: max |dy| handed in by the producer of dy, x (an O(1) activation) split unscaled
    from mpgan_amd import ops
    dyd = dev(dy)
    dw2 = train_ops.conv2d_wgrad_mfma(dev(x), dyd, k, k, wscale, prec, ops.absmax(dyd), train_ops.unit_amax(dyd.device))
    assert rel(dw2.cpu().numpy(), dw_ref) < (2e-6 if prec == 3 else 2e-3)


@pytest.mark.parametrize("prec", [3, 1])
@pytest.mark.parametrize("case", WG_MFMA_CASES)
def test_conv_wgrad_g8(case, prec):
    """the same kernel fed the G8 tensors a training step already holds (forward input unscaled, dy scaled by its maximum):
    bit-identical to the fp32 entry, which converts to the same G8 inside its workspace"""
    from mpgan_amd import ops, train_ops
    n, h, w, cin, cout, k = case
    rng = np.random.default_rng(hash(case) % 2 ** 31 + 1)
    x = dev(rng.standard_normal((n, h, w, cin)).astype(np.float32))
    dy = dev((rng.standard_normal((n, h, w, cout)) * 1e-6).astype(np.float32))
    wscale = float(np.float32(math.sqrt(2.0) / math.sqrt(k * k * cin)))
    am = ops.absmax(dy)
    ref = train_ops.conv2d_wgrad_mfma(x, dy, k, k, wscale, prec, am, train_ops.unit_amax(dy.device))
    got = train_ops.conv2d_wgrad_g8(ops.to_g8(x), ops.to_g8(dy, amax=am), k, k, wscale, prec, None, am)
    # the row ranges are combined with fp32 atomics in launch order: equal up to that reordering
    assert rel(got.cpu().numpy(), ref.cpu().numpy()) < 1e-6


@pytest.mark.parametrize("shape", [(3, 5), (7, 3), (1, 5), (5, 1), (2, 4), (6, 3)])
def test_conv_wgrad_mfma_other_filter_shapes(shape):
    """non-square and 1-wide filters stay on the one-filter-row kernel (square 3x3 / 4x4 / 5x5 run the ring form)"""
    from mpgan_amd import train_ops
    kh, kw = shape
    rng = np.random.default_rng(100 * kh + kw)
    x = rng.standard_normal((2, 18, 37, 24)).astype(np.float32)
    dy = (rng.standard_normal((2, 18, 37, 40)) * 1e-5).astype(np.float32)
    wt = rng.standard_normal((kh, kw, 24, 40)).astype(np.float32)
    _, dw_ref = ref_conv_grads(x, wt, dy, 1, 0.05)
    dw = train_ops.conv2d_wgrad_mfma(dev(x), dev(dy), kh, kw, 0.05, 3).cpu().numpy()
    assert dw.shape == dw_ref.shape and rel(dw, dw_ref) < 2e-6


def test_conv_wgrad_mfma_zero_and_constant():
    from mpgan_amd import train_ops
    x = np.ones((1, 8, 8, 3), np.float32)
    dy = np.zeros((1, 8, 8, 5), np.float32)
    assert np.array_equal(train_ops.conv2d_wgrad_mfma(dev(x), dev(dy), 3, 3).cpu().numpy(), np.zeros((3, 3, 3, 5), np.float32))
    dy[:] = 1.0
    dw = train_ops.conv2d_wgrad_mfma(dev(x), dev(dy), 3, 3).cpu().numpy()
    # number of valid (pixel, shifted pixel) pairs per tap of an 8x8 image: (8 - |dy|)(8 - |dx|)
    want = np.array([[(8 - abs(a)) * (8 - abs(b)) for b in (-1, 0, 1)] for a in (-1, 0, 1)], np.float32)
    assert np.array_equal(dw, np.broadcast_to(want[:, :, None, None], dw.shape))


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("case", [(2, 16, 16, 8, 32, 5, 1, "relu"), (2, 16, 16, 32, 8, 5, 1, None),
                                  (2, 16, 16, 16, 16, 1, 1, "lrelu"), (2, 16, 16, 2, 32, 4, 2, "lrelu"),
                                  (2, 8, 8, 128, 256, 4, 1, "lrelu")])
def test_conv_layer_fn(case, bn):
    """ConvLayerFn (fused forward, MFMA data gradient where the shape allows) vs float64 autograd"""
    from mpgan_amd import ops
    from mpgan_amd.train import ConvLayerFn
    n, h, w, cin, cout, k, s, act = case
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = rng.standard_normal((k, k, cin, cout)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    oh, ow = -(-h // s), -(-w // s)
    dy = rng.standard_normal((n, oh, ow, cout)).astype(np.float32)
    wscale = float(np.float32(math.sqrt(2.0) / math.sqrt(k * k * cin)))
    # reference
    p = {"L/weight": torch.tensor(wt, dtype=torch.float64, requires_grad=True),
         "L/bias": torch.tensor(b, dtype=torch.float64, requires_grad=True),
         "L/gamma": torch.tensor(gamma, dtype=torch.float64, requires_grad=True),
         "L/beta": torch.tensor(beta, dtype=torch.float64, requires_grad=True)}
    xr = torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    gain = wscale * math.sqrt(k * k * cin)
    yr, _ = TR.conv_layer(p, "L", xr, act, s, bn, gain=gain)
    yr.backward(torch.tensor(dy, dtype=torch.float64).permute(0, 3, 1, 2))
    # HIP
    xt = dev(x).requires_grad_(True)
    wd, bd, gd, bed = [dev(a).requires_grad_(True) for a in (wt, b, gamma, beta)]
    cfg = {"stride": (s, s), "wscale": wscale, "act": act, "leak": 0.2, "prec": ops.PREC_F16X3, "eps": 1e-3}
    y = ConvLayerFn.apply(xt, wd, bd, gd if bn else None, bed if bn else None, cfg)
    y.backward(dev(dy))
    tol = 2e-5
    assert rel(y.detach().cpu().numpy(), yr.detach().permute(0, 2, 3, 1).numpy()) < tol
    assert rel(xt.grad.cpu().numpy(), xr.grad.permute(0, 2, 3, 1).numpy()) < tol
    assert rel(wd.grad.cpu().numpy(), p["L/weight"].grad.numpy()) < tol
    if bn:
        assert rel(gd.grad.cpu().numpy(), p["L/gamma"].grad.numpy()) < tol
        assert rel(bed.grad.cpu().numpy(), p["L/beta"].grad.numpy()) < tol
        # the bias gradient under batch norm is zero up to rounding
        assert np.abs(bd.grad.cpu().numpy()).max() < 1e-3 * np.abs(dy).sum() / cout
        mean, var = cfg["batch_stats"]
        lin = TR.conv2d_same(xr, p["L/weight"] * wscale, s) + p["L/bias"].view(1, -1, 1, 1)
        assert rel(mean.cpu().numpy(), lin.mean(dim=(0, 2, 3)).detach().numpy()) < tol
        assert rel(var.cpu().numpy(), lin.var(dim=(0, 2, 3), unbiased=False).detach().numpy()) < 1e-4
    else:
        assert rel(bd.grad.cpu().numpy(), p["L/bias"].grad.numpy()) < tol


def test_elementwise_backward():
    from mpgan_amd import train_ops
    from mpgan_amd.train import ActFn, AvgPoolFn, LerpFn, PixelNormFn, ResizeNearestFn
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 6, 10, 12)).astype(np.float32)
    x2 = rng.standard_normal((2, 6, 10, 12)).astype(np.float32)

    def check(fn_hip, fn_ref, *arrs, tol=1e-6):
        th = [dev(a).requires_grad_(True) for a in arrs]
        tr = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in arrs]
        yh, yr = fn_hip(*th), fn_ref(*tr)
        g = rng.standard_normal(tuple(yr.shape)).astype(np.float32)
        yh.backward(dev(g))
        yr.backward(torch.tensor(g, dtype=torch.float64))
        assert rel(yh.detach().cpu().numpy(), yr.detach().numpy()) < tol
        for a, b in zip(th, tr):
            assert rel(a.grad.cpu().numpy(), b.grad.numpy()) < tol

    def check2(fn_hip, fn_ref, *arrs, tol=1e-6):
        """second derivative of an any-order Function: the first gradient is taken with create_graph=True for an upstream
        gradient g that is a variable itself, then a random projection of that gradient is differentiated back to g
        (J applied to the projection) and to the inputs (zero: the ops are linear, or piecewise linear away from 0)"""
        th = [dev(a).requires_grad_(True) for a in arrs]
        tr = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in arrs]
        yh, yr = fn_hip(*th), fn_ref(*tr)
        g = rng.standard_normal(tuple(yr.shape)).astype(np.float32)
        gh, gr = dev(g).requires_grad_(True), torch.tensor(g, dtype=torch.float64, requires_grad=True)
        dh = torch.autograd.grad(yh, th, gh, create_graph=True)
        dr = torch.autograd.grad(yr, tr, gr, create_graph=True)
        proj = [rng.standard_normal(tuple(d.shape)).astype(np.float32) for d in dr]
        for a, b in zip(dh, dr):
            assert rel(a.detach().cpu().numpy(), b.detach().numpy()) < tol
        sum((d * dev(q)).sum() for d, q in zip(dh, proj)).backward()
        sum((d * torch.tensor(q, dtype=torch.float64)).sum() for d, q in zip(dr, proj)).backward()
        assert float(gr.grad.norm()) > 0
        assert rel(gh.grad.cpu().numpy(), gr.grad.numpy()) < tol
        for a, b, arr in zip(th, tr, arrs):
            ga = np.zeros_like(arr) if a.grad is None else a.grad.cpu().numpy()
            gb = np.zeros_like(arr) if b.grad is None else b.grad.numpy(force=True)
            assert rel(ga, gb) < tol

    check(lambda a, b: ActFn.apply(a, b, "relu", 0.2), lambda a, b: torch.relu(a + b), x, x2)
    check(lambda a: ActFn.apply(a, None, "lrelu", 0.2), lambda a: TR.lrelu(a), x)
    check(lambda a: ActFn.apply(a, None, "tanh", 0.2), lambda a: torch.tanh(a), x)
    check(lambda a, b: ActFn.apply(a, b, None, 0.2), lambda a, b: a + b, x, x2)
    check(lambda a: PixelNormFn.apply(a, 1e-8), lambda a: a * torch.rsqrt((a * a).mean(dim=3, keepdim=True) + 1e-8), x)
    check(lambda a: ResizeNearestFn.apply(a, 24, 20),
          lambda a: a.repeat_interleave(4, 1).repeat_interleave(2, 2), x)
    check(lambda a: AvgPoolFn.apply(a),
          lambda a: F.avg_pool2d(a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), x)
    check(lambda a, b: LerpFn.apply(a, b, 0.3), lambda a, b: a + (b - a) * 0.3, x, x2)
    check(lambda b: LerpFn.apply(None, b, 1.7), lambda b: b * 1.0, x2)
    # the any-order Functions differentiated twice (seeded normal data: no pre-activation at or next to 0)
    check2(lambda a: ActFn.apply(a, None, "relu", 0.2), lambda a: torch.relu(a), x)
    check2(lambda a: ActFn.apply(a, None, "lrelu", 0.2), lambda a: TR.lrelu(a), x)
    check2(lambda a, b: ActFn.apply(a, b, "relu", 0.2), lambda a, b: torch.relu(a + b), x, x2)
    check2(lambda a, b: ActFn.apply(a, b, "lrelu", 0.2), lambda a, b: TR.lrelu(a + b), x, x2)
    check2(lambda a, b: ActFn.apply(a, b, None, 0.2), lambda a, b: a + b, x, x2)
    check2(lambda a: ResizeNearestFn.apply(a, 24, 20),
           lambda a: a.repeat_interleave(4, 1).repeat_interleave(2, 2), x)
    check2(lambda a: AvgPoolFn.apply(a),
           lambda a: F.avg_pool2d(a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), x)
    check2(lambda a, b: LerpFn.apply(a, b, 0.3), lambda a, b: a + (b - a) * 0.3, x, x2)
    check2(lambda b: LerpFn.apply(None, b, 1.7), lambda b: b * 1.0, x2)
    s = train_ops.channel_sum(dev(x)).cpu().numpy()
    assert rel(s, x.reshape(-1, 12).astype(np.float64).sum(0)) < 1e-6


def test_first_order_function_refuses_second_derivative():
    """PixelNormFn's backward is a kernel call without a tape: a second derivative through it has to raise, not read as
    zero.  The product with `a` gives the first gradient a grad_fn of its own, so nothing else can raise here."""
    from mpgan_amd.train import PixelNormFn
    rng = np.random.default_rng(4)
    a = dev(rng.standard_normal((2, 6, 10, 12)).astype(np.float32)).requires_grad_(True)
    z = PixelNormFn.apply(a, 1e-8) * a
    (g,) = torch.autograd.grad(z.sum(), a, create_graph=True)
    assert g.grad_fn is not None
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g.sum().backward()


def test_adam_step_matches_tf_formula():
    from mpgan_amd import train_ops
    rng = np.random.default_rng(9)
    n = 10007
    p = rng.standard_normal(n).astype(np.float32)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    pd, md, vd = dev(p), dev(m), dev(v)
    pr, mr, vr = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for t in range(1, 4):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n)).astype(np.float32)
        lr_t = dev(np.array([2e-4 * math.sqrt(1 - 0.999 ** t) / (1 - 0.5 ** t)]))
        train_ops.adam_step(pd, dev(g), md, vd, lr_t, 0.5, 0.999, 1e-8)
        pr, mr, vr = TR.adam_tf(pr, g.astype(np.float64), mr, vr, t)
    e_p = np.abs(pd.cpu().numpy() - pr).max()
    e_m, e_v = rel(md.cpu().numpy(), mr), rel(vd.cpu().numpy(), vr)
    assert e_p < 1e-6 and e_m < 1e-6 and e_v < 1e-6, (e_p, e_m, e_v)


BN_BIASES = {"generator/g_c%s%d/bias" % (k, i) for k in "AB" for i in range(3)} | \
    {"generator/g_s%d/bias" % i for i in range(3)} | {"discriminator/d_c%d/bias" % i for i in (2, 3, 4)}


def _trainer_and_oracle(tile, C, batch, bn, seed=5, prec=3):
    from mpgan_amd.train import Trainer4x
    tr = Trainer4x(tileSizeLow=tile, upRes=4, n_inputChannels=C, batch_norm=bn, device=DEV, seed=seed, prec=prec)
    ps = ParamSource(seed=seed)
    params = {}
    for name, spec in tr.graph.variables.items():
        params[name] = ps.get(name, spec.shape, spec.kind)
    with torch.no_grad():
        for name, t in tr.sess.params.items():
            t.copy_(dev(params[name]))
    rng = np.random.default_rng(77)
    xs = rng.random((batch, tile * tile * C)).astype(np.float32)
    ys = rng.random((batch, (tile * 4) ** 2)).astype(np.float32)
    return tr, TR.to_params(params), xs, ys


@pytest.mark.parametrize("C,bn", [(4, True), (1, True), (4, False)])
def test_gan4x_losses_and_gradients(C, bn):
    tile, batch = 8, 4
    tr, p, xs, ys = _trainer_and_oracle(tile, C, batch, bn)
    L = tr.losses(xs, ys)
    Lr = TR.losses_4x(p, xs, ys, tile, 4, C, batch_norm=bn)
    for k in ("disc_loss", "gen_loss", "gen_l1_loss", "gen_l2_loss", "disc_loss_layer", "gen_loss_complete"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), (k, a, b)
    assert rel(L["gen_part"].detach().cpu().numpy().reshape(batch, -1), Lr["gen_part"].detach().numpy().reshape(batch, -1)) < 1e-4
    rd = TR.grads(Lr["disc_loss"], p, "d_")
    rg = TR.grads(Lr["gen_loss_complete"], p, "g_")
    assert sorted(rd) == tr.opt_d.names and sorted(rg) == tr.opt_g.names

    def compare(L):
        gd = torch.autograd.grad(L["disc_loss"], tr.opt_d.params, allow_unused=True, retain_graph=True)
        gg = torch.autograd.grad(L["gen_loss_complete"], tr.opt_g.params, allow_unused=True)
        worst, total, off = 0.0, 0.0, []
        for names, got, want in ((tr.opt_d.names, gd, rd), (tr.opt_g.names, gg, rg)):
            tot_d = tot_r = 0.0
            for nme, g in zip(names, got):
                w = want[nme]
                gnp = g.cpu().numpy().astype(np.float64) if g is not None else np.zeros_like(w)
                if bn and nme in BN_BIASES:
                    # bias under batch norm: exact gradient is 0, both sides hold rounding noise only
                    assert np.abs(gnp).max() < 1e-4
                    continue
                r = rel(gnp, w)
                worst = max(worst, r)
                if r >= 1e-4:
                    off.append((nme, float("%.3g" % r)))
                tot_d += float(((gnp - w) ** 2).sum())
                tot_r += float((w ** 2).sum())
            total = max(total, math.sqrt(tot_d / tot_r))
        return worst, total, off

    # The gradient of a ReLU network is discontinuous where a pre-activation is zero, and with 5e5 activations in the widest
    # layer of this case the one nearest to zero sits ~2e-6 away.  While the batch statistics were combined with atomics
    # (1e-7 run-to-run variation) that element's mask came out on the other side than in the float64 oracle in ~3 % of the
    # evaluations, and ONE flipped element moves the gradients of everything upstream by 1 / sqrt(5e5) ~ 1e-3 -- always the
    # same alternative numbers (tools/experiments/grad_flake.py: the ReLU backward of generator/g_cA1, inputs 1e-6 apart,
    # outputs 9e-4 apart).  The statistics are now block sums added in a fixed order (mpg_bn_train_fwd_ordered): the forward
    # pass, and with it every mask, is the same bits on every run (0 deviations in 900 repetitions).
    worst, total, off = compare(L)
    assert total < 2e-4, off
    assert worst < 1e-3, off
    print("worst per-tensor gradient error", worst)


def test_gan4x_gradients_with_f16f6_convolutions():
    """the opt-in training precision 2: forward and data-gradient convolutions at MPG_PREC_F16F6 where the kernels cover the
    shape (here the 128-wide layers), weight gradients at three products: losses to 1e-3, the generator's gradient to 2e-2
    (measured 7e-3: gradient tensors are sparse behind the ReLUs and span decades inside a 32-value scale block)"""
    tile, C, batch = 8, 4, 4
    tr, p, xs, ys = _trainer_and_oracle(tile, C, batch, True, prec=2)
    L = tr.losses(xs, ys)
    Lr = TR.losses_4x(p, xs, ys, tile, 4, C, batch_norm=True)
    for k in ("disc_loss", "gen_loss_complete"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        assert abs(a - b) <= 1e-3 * max(abs(b), 1e-3), (k, a, b)
    gg = torch.autograd.grad(L["gen_loss_complete"], tr.opt_g.params, allow_unused=True)
    rg = TR.grads(Lr["gen_loss_complete"], p, "g_")
    tot_d = tot_r = 0.0
    for nme, g in zip(tr.opt_g.names, gg):
        if nme in BN_BIASES:
            continue
        w = rg[nme]
        gnp = g.cpu().numpy().astype(np.float64)
        tot_d += float(((gnp - w) ** 2).sum())
        tot_r += float((w ** 2).sum())
    err = math.sqrt(tot_d / tot_r)
    print("generator gradient error at training precision 2:", err)
    assert err < 2e-2


def test_gan4x_train_step_updates_parameters():
    tile, C, batch = 8, 4, 4
    tr, p, xs, ys = _trainer_and_oracle(tile, C, batch, True)
    before = {n: t.detach().cpu().numpy().copy() for n, t in tr.sess.params.items()}
    Lr = TR.losses_4x(p, xs, ys, tile, 4, C)
    rd = TR.grads(Lr["disc_loss"], p, "d_")
    stats = {}
    TR.losses_4x(p, xs, ys, tile, 4, C, stats=stats)
    Ld = tr.disc_step(xs, ys)
    lr = 2e-4
    bad = tot = 0
    for nme in tr.opt_d.names:
        delta = tr.sess.params[nme].detach().cpu().numpy() - before[nme]
        want, _, _ = TR.adam_tf(np.zeros_like(rd[nme]), rd[nme], np.zeros_like(rd[nme]), np.zeros_like(rd[nme]), 1)
        assert np.abs(delta).max() <= lr * 1.001
        strong = np.abs(rd[nme]) > 1e-6 * np.abs(rd[nme]).max()
        bad += int((np.abs(delta - want)[strong] > 0.05 * lr).sum())
        tot += int(strong.sum())
    assert bad <= 0.002 * tot, (bad, tot)
    # generator parameters untouched by the discriminator step, moving averages advanced
    for nme in tr.opt_g.names:
        assert np.array_equal(tr.sess.params[nme].detach().cpu().numpy(), before[nme])
    mm = "generator/g_cA1/moving_mean"
    want_mm = 0.999 * before[mm] + 0.001 * stats["generator/g_cA1"][0].numpy()
    assert rel(tr.sess.params[mm].detach().cpu().numpy(), want_mm) < 1e-5
    # a generator step moves the generator only and lowers the L1 term on the same batch over a few steps
    d_before = {n: tr.sess.params[n].detach().cpu().numpy().copy() for n in tr.opt_d.names}
    l1 = [float(tr.gen_step(xs, ys)["gen_l1_loss"].detach()) for _ in range(6)]
    for nme in tr.opt_d.names:
        assert np.array_equal(tr.sess.params[nme].detach().cpu().numpy(), d_before[nme])
    assert l1[-1] < l1[0]
    assert np.isfinite(float(Ld["disc_loss"].detach()))


def test_graphed_iteration_matches_eager():
    """the captured hipGraph of the iteration replays to the same parameters as the eager step"""
    tile, C, batch = 8, 4, 4
    tr_e, _, xs, ys = _trainer_and_oracle(tile, C, batch, True)
    tr_g, _, _, _ = _trainer_and_oracle(tile, C, batch, True)
    rng = np.random.default_rng(5)
    batches = [(xs, ys)] + [(rng.random(xs.shape).astype(np.float32), rng.random(ys.shape).astype(np.float32)) for _ in range(7)]
    # the graphed trainer spends one eager warm-up iteration on its first batch before capturing
    tr_e.train_step(dev(batches[0][0]), dev(batches[0][1]))
    for bx, by in batches:
        de, ge = tr_e.train_step(dev(bx), dev(by))
        d, g = tr_g.train_step_graphed(bx, by)
        # every replay reproduces the eager iteration (memset nodes of a captured graph did not: the
        # library zeroes its accumulators with a kernel, and the loss reductions are mpg_pair_reduce)
        assert abs(float(d) - float(de)) < 2e-3 and abs(float(g) - float(ge)) < 2e-3, (float(d), float(de), float(g), float(ge))
    torch.cuda.synchronize()
    assert tr_g.opt_d.t == tr_e.opt_d.t == 9
    for nme in tr_e.sess.params:
        a = tr_e.sess.params[nme].detach().cpu().numpy()
        b = tr_g.sess.params[nme].detach().cpu().numpy()
        if nme in BN_BIASES:
            continue        # zero gradient up to rounding: Adam turns the noise into +-lr steps on both sides
        # atomics make the weight-gradient sums order dependent: compare at Adam step size granularity
        diff = np.abs(a - b)
        assert (diff > 1e-4).mean() <= 0.01, (nme, float((diff > 1e-4).mean()))
        assert diff.mean() <= 2e-5, (nme, float(diff.mean()))
    assert np.isfinite(float(d)) and np.isfinite(float(g))


@pytest.mark.parametrize("clamp", [True, False])
def test_tensor_resample_forward_backward(clamp):
    """tensorResample (advection look-up of the temporal discriminator inputs) incl. positions outside the grid"""
    from mpgan_amd.train import ResampleFn
    rng = np.random.default_rng(21)
    n, h, w, c = 3, 12, 10, 2
    v = rng.standard_normal((n, h, w, c)).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    pos = np.stack([yy, xx], -1)[None] + rng.normal(0, 1.5, (n, h, w, 2))
    pos = pos.astype(np.float32)
    g = rng.standard_normal((n, h, w, c)).astype(np.float32)
    vr = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    outr = TR.tensor_resample(vr, pos, clamp)
    outr.backward(torch.tensor(g, dtype=torch.float64))
    vt = dev(v).requires_grad_(True)
    out = ResampleFn.apply(vt, dev(pos), clamp)
    out.backward(dev(g))
    assert rel(out.detach().cpu().numpy(), outr.detach().numpy()) < 1e-6
    assert rel(vt.grad.cpu().numpy(), vr.grad.numpy()) < 1e-6
    # identity positions return the field itself -- except in the last row / column when clamping: the ceil
    # index is clamped onto the floor index and both keep weight 1 (the reference computes the weights from
    # the clamped indices, multipassGAN-4x.py:408-430), so those samples are counted twice
    ident = np.broadcast_to(np.stack([yy, xx], -1)[None], (n, h, w, 2)).astype(np.float32)
    got = ResampleFn.apply(dev(v), dev(np.ascontiguousarray(ident)), clamp).cpu().numpy()
    assert np.allclose(got[:, :-1, :-1], v[:, :-1, :-1], atol=1e-6)
    if clamp:
        assert np.allclose(got[:, -1, :-1], 2 * v[:, -1, :-1], atol=1e-5) and np.allclose(got[:, -1, -1], 4 * v[:, -1, -1], atol=1e-5)


def test_temporal_discriminator_losses_and_gradients():
    """coherent triples from TileCreator.selectRandomTempoTiles -> advection -> disc_binclass_cond_tempo"""
    import contextlib
    import io
    import random
    from mpgan_amd import tilecreator_t as tc
    from mpgan_amd.train import Trainer4x
    tile, C, up = 8, 4, 4
    rng = np.random.default_rng(31)
    with contextlib.redirect_stdout(io.StringIO()):
        tiCr = tc.TileCreator(tileSizeLow=tile, simSizeLow=16, upres=up, dim=2, dim_t=3, densityMinimum=0.0,
                              channelLayout_low="d,vx,vy,vz", channelLayout_high="d")
        tiCr.addData(rng.random((4, 1, 16, 16, 12)).astype(np.float32), rng.random((4, 1, 64, 64, 3)).astype(np.float32))
    random.seed(1)
    xts, yts, ypos = tiCr.selectRandomTempoTiles(6, True, False, n_t=3, dt=0.5)
    assert xts.shape == (6, tile * tile * C) and yts.shape == (6, 32 * 32) and ypos.shape == (6, 2 * 32 * 32)
    tr = Trainer4x(tileSizeLow=tile, upRes=up, n_inputChannels=C, batch_norm=True, device=DEV, seed=5, use_tempo=True)
    ps = ParamSource(seed=5)
    params = {n: ps.get(n, s.shape, s.kind) for n, s in tr.graph.variables.items()}
    with torch.no_grad():
        for n, t in tr.sess.params.items():
            t.copy_(dev(params[n]))
    p = TR.to_params(params)
    L = tr.tempo_losses(xts, yts, ypos)
    Lr = TR.tempo_losses_4x(p, xts, yts, ypos, tile, up, C)
    for k in ("t_disc_loss", "t_gen_loss"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), (k, a, b)
    gt = torch.autograd.grad(L["t_disc_loss"], tr.opt_t.params, allow_unused=True, retain_graph=True)
    gg = torch.autograd.grad(L["t_gen_loss"], tr.opt_g.params, allow_unused=True)
    rt = TR.grads(Lr["t_disc_loss"], p, "t_")
    rt = {k: v for k, v in rt.items() if k.startswith("discriminatorTempo")}
    rg = TR.grads(Lr["t_gen_loss"], p, "g_")
    assert sorted(rt) == tr.opt_t.names
    bn_bias = BN_BIASES | {"discriminatorTempo/t_c%d/bias" % i for i in (2, 3, 4)}
    for names, got, want in ((tr.opt_t.names, gt, rt), (tr.opt_g.names, gg, rg)):
        for nme, g in zip(names, got):
            if nme in bn_bias:
                continue
            # one ReLU pre-activation of this batch sits within rounding of zero: fp32 and float64 disagree on its
            # gate, which moves every upstream gradient by ~1 / sqrt(pixels) (3e-3 here; batches without such a
            # pixel agree to 6e-6, see test_gan4x_losses_and_gradients).  The order of the atomics can flip it too.
            assert rel(g.cpu().numpy(), want[nme]) < 2e-2, nme
    # one full iteration with the temporal branch
    xs, ys = rng.random((4, tile * tile * C)).astype(np.float32), rng.random((4, 32 * 32)).astype(np.float32)
    before = {n: t.detach().clone() for n, t in tr.sess.params.items()}
    d, g = tr.train_step(xs, ys, tempo=(xts, yts, ypos))
    assert np.isfinite(float(d)) and np.isfinite(float(g))
    assert all(not torch.equal(tr.sess.params[n].detach(), before[n]) for n in tr.opt_t.names if n not in bn_bias)


def test_temporal_l2_loss_of_the_4x_generator():
    """lambda_t_l2 (useTempoL2, multipassGAN-4x.py:147-152,815-826): l2 distance of consecutive advected generator frames,
    without the temporal discriminator; loss value and generator gradients against the float64 restatement"""
    import contextlib
    import io
    import random
    from mpgan_amd import tilecreator_t as tc
    from mpgan_amd.train import Trainer4x
    tile, C, up = 8, 4, 4
    rng = np.random.default_rng(37)
    with contextlib.redirect_stdout(io.StringIO()):
        tiCr = tc.TileCreator(tileSizeLow=tile, simSizeLow=16, upres=up, dim=2, dim_t=3, densityMinimum=0.0,
                              channelLayout_low="d,vx,vy,vz", channelLayout_high="d")
        tiCr.addData(rng.random((4, 1, 16, 16, 12)).astype(np.float32), rng.random((4, 1, 64, 64, 3)).astype(np.float32))
    random.seed(2)
    xts, yts, ypos = tiCr.selectRandomTempoTiles(6, True, False, n_t=3, dt=0.5)
    tr = Trainer4x(tileSizeLow=tile, upRes=up, n_inputChannels=C, batch_norm=True, device=DEV, seed=5, use_tempo=False,
                   lambda_t_l2=0.5)
    assert not hasattr(tr, "opt_t") and not any(n.startswith("discriminatorTempo") for n in tr.graph.variables)
    ps = ParamSource(seed=5)
    params = {n: ps.get(n, s.shape, s.kind) for n, s in tr.graph.variables.items()}
    with torch.no_grad():
        for n, t in tr.sess.params.items():
            t.copy_(dev(params[n]))
    full = Trainer4x(tileSizeLow=tile, upRes=up, n_inputChannels=C, batch_norm=True, device=DEV, seed=5, use_tempo=True)
    pfull = {n: ps.get(n, s.shape, s.kind) for n, s in full.graph.variables.items()}
    p = TR.to_params(pfull)
    L = tr.tempo_losses(xts, yts, ypos)
    assert sorted(L) == ["tl_gen_loss"]
    Lr = TR.tempo_losses_4x(p, xts, yts, ypos, tile, up, C)
    a, b = float(L["tl_gen_loss"].detach()), float(Lr["tl_gen_loss"].detach())
    assert abs(a - b) <= 1e-4 * max(abs(b), 1e-6), (a, b)
    gg = torch.autograd.grad(L["tl_gen_loss"], tr.opt_g.params, allow_unused=True)
    rg = TR.grads(Lr["tl_gen_loss"], p, "g_")
    for nme, g in zip(tr.opt_g.names, gg):
        if nme in BN_BIASES:
            continue
        assert rel(g.cpu().numpy(), rg[nme]) < 2e-2, nme
    xs, ys = rng.random((4, tile * tile * C)).astype(np.float32), rng.random((4, 32 * 32)).astype(np.float32)
    Lg = tr.gen_step_tempo(xs, ys, xts, yts, ypos)
    want = float(Lg["gen_loss"].detach()) + float(Lg["gen_l1_loss"].detach()) * tr.k + float(Lg["disc_loss_layer"].detach()) * tr.k2 \
        + 0.5 * float(Lg["tl_gen_loss"].detach())
    assert abs(float(Lg["gen_loss_complete"].detach()) - want) <= 1e-5 * abs(want)


# ---------------------------------------------------------------------------------------------
# f4: GAN.advect (GAN.py:173-418) -- semi-Lagrangian / MacCormack gather kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hv", [8, 16])
def test_advect_kernels_vs_oracle(hv):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import train_ops
    from oracle import advect as A
    rng = np.random.default_rng(hv)
    n, h = 6, 16
    src = rng.random((n, h, h, 1)).astype(np.float32)
    vel = (rng.standard_normal((n, hv, hv, 3)) * 3.0).astype(np.float32)
    flags = (rng.random((n, h, h, 1)) < 0.25).astype(np.float32)
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    # the displacement field (bilinear resize, MAC -> centre, dt pattern)
    v = train_ops.advect_velocity(t(vel), h, h, 0.5).cpu().numpy()
    want_v = A.centred_velocity(vel, h, h, 0.5)
    assert np.abs(v - want_v).max() < 1e-5
    # semi-Lagrange: vectorised oracle and the scalar loop
    fwd = train_ops.advect(t(src), t(vel), t(flags), 0.5, 1).cpu().numpy()
    assert np.abs(fwd - A.advect(src, vel, flags, 0.5, 1)).max() < 2e-5
    assert np.abs(fwd - A.semi_lagrange_loop(src, want_v, A.positions(h, h))).max() < 2e-5
    # several channels
    src3 = rng.random((n, h, h, 3)).astype(np.float32)
    f3 = train_ops.advect(t(src3), t(vel), None, 0.5, 1).cpu().numpy()
    assert np.abs(f3 - A.advect(src3, vel, None, 0.5, 1)).max() < 2e-5
    # MacCormack with the reference's clamp
    mc = train_ops.advect(t(src), t(vel), t(flags), 0.5, 2, 1.0, start_bz=n).cpu().numpy()
    want = A.advect(src, vel, flags, 0.5, 2, 1.0, start_bz=n)
    bad = np.abs(mc - want) > 2e-5
    # a corrected value sitting exactly on its clamp bound may fall on either side in fp32 vs the oracle's float64 sums
    assert bad.mean() < 2e-3, bad.mean()
    # gradient of the order-1 look-up with respect to the source = the transposed gather
    s = t(src3).requires_grad_(True)
    out = train_ops.advect(s, t(vel), None, 0.5, 1)
    g = torch.randn_like(out)
    (ds,) = torch.autograd.grad(out, [s], g)
    s2 = torch.as_tensor(src3, dtype=torch.float64)
    basis = torch.as_tensor(A.semi_lagrange(np.ones_like(src3), want_v, A.positions(h, h)))   # column sums of the weights
    assert abs(float((ds.cpu().double().sum())) - float((g.cpu().double() * basis.double()).sum())) < 1e-2
    # adjoint identity <advect(x), g> = <x, advect^T(g)>
    lhs = float((out.detach().cpu().double() * g.cpu().double()).sum())
    rhs = float((s2 * ds.cpu().double()).sum())
    assert abs(lhs - rhs) < 1e-3 * max(abs(lhs), 1.0)


@pytest.mark.parametrize("order,n,h", [(1, 6, 16), (2, 6, 16), (2, 24, 16)])
def test_advect_gradient_vs_torch_restatement(order, n, h):
    """d advect / d source for both orders against autograd on the float64 restatement of the op graph; the last case has
    more batch rows than columns (the reference clips the batch index of three clamp corners to w-1)"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import train_ops
    from oracle import advect as A
    rng = np.random.default_rng(100 * order + n)
    src = rng.random((n, h, h, 1)).astype(np.float32)
    src[:, :5] = 0.0                                      # empty region: forward == corrected there, the mask still counts
    vel = (rng.standard_normal((n, 8, 8, 3)) * 2.0).astype(np.float32)
    flags = (rng.random((n, h, h, 1)) < 0.2).astype(np.float32)
    g = rng.standard_normal((n, h, h, 1))
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    s = t(src).requires_grad_(True)
    out = train_ops.advect(s, t(vel), t(flags), 0.5, order, 1.0, start_bz=n)
    (ds,) = torch.autograd.grad(out, [s], t(g.astype(np.float32)))
    s64 = torch.tensor(src, dtype=torch.float64, requires_grad=True)
    ref = A.advect_torch(s64, vel, flags, 0.5, order, 1.0, n)
    (dr,) = torch.autograd.grad(ref, [s64], torch.tensor(g))
    bad = np.abs(out.detach().cpu().numpy() - ref.detach().numpy()) > 2e-5
    assert bad.mean() < 2e-3, bad.mean()
    if bad.any():     # a clamp decision on the bound differs: compare the gradient away from those outputs only loosely
        assert rel(ds.cpu().numpy(), dr.numpy()) < 5e-2
    else:
        assert rel(ds.cpu().numpy(), dr.numpy()) < 1e-5, rel(ds.cpu().numpy(), dr.numpy())



def test_gan_advect_through_the_builder():
    """GAN(x).advect(...) as the reference's graph code calls it (multipassGAN-8x.py:1199), run by the session"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import graph as G
    from mpgan_amd.GAN import GAN
    from mpgan_amd.session import Session, VariableStore
    from oracle import advect as A
    n, h = 6, 16
    prev = G.get_default_graph()
    g = G.reset_default_graph()
    try:
        src_p = G.placeholder([None, h, h, 1])
        vel_p = G.placeholder([None, 4, 4, 3])
        flags_p = G.placeholder([None, h, h, 1])
        sl = GAN(src_p).advect(src_p, vel_p, flags_p, 0.5, 1, 1.0, startBz=n)
        mc = GAN(src_p).advect(src_p, vel_p, flags_p, 0.5, 2, 1.0, startBz=n)
    finally:
        G._default_graph[0] = prev
    rng = np.random.default_rng(8)
    src = rng.random((n, h, h, 1)).astype(np.float32)
    vel = (rng.standard_normal((n, 4, 4, 3)) * 0.7).astype(np.float32)
    flags = np.zeros((n, h, h, 1), np.float32)
    sess = Session(graph=g, variables=VariableStore("cuda:0"), device="cuda:0")
    got_sl, got_mc = sess.run([sl, mc], {src_p: src, vel_p: vel, flags_p: flags})
    assert np.abs(got_sl - A.advect(src, vel, flags, 0.5, 1)).max() < 2e-5
    bad = np.abs(got_mc - A.advect(src, vel, flags, 0.5, 2, 1.0, n)) > 2e-5
    assert bad.mean() < 2e-3


@pytest.mark.parametrize("rows,k,cout", [(3, 100, 1), (16, 20000, 1), (4, 40000, 5), (2, 16384, 70), (16, 262144, 1)])
def test_fc_forward_short_and_split_k(rows, k, cout):
    """GAN.fully_connected_layer (GAN.py:438-456); long contractions are split over K (atomic partial sums)"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import train_ops
    rng = np.random.default_rng(rows * 7 + cout)
    x = rng.standard_normal((rows, k)).astype(np.float32)
    w = rng.standard_normal((k, cout)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    ws = float(1.0 / math.sqrt(k))
    for act in (None, "lrelu"):
        y = train_ops.fc_forward(dev(x), dev(w), ws, dev(b), act).cpu().numpy()
        ref = x.astype(np.float64) @ w.astype(np.float64) * ws + b
        if act == "lrelu":
            ref = np.where(ref > 0, ref, 0.2 * ref)
        assert np.abs(y - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), np.abs(y - ref).max()
