"""WGAN-GP through batch-normalised critics with minibatch stddev (multipassGAN-8x.py:1123-1140 with batchNorm 1 /
use_mb_stddev 1): the double-backward kernels against float64 torch.autograd, the discriminator-step gradients of the 8x
trainer against a float64 restatement of the critics, the moving averages, and the training driver."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O
from oracle import train_ref as TR
from oracle import train_ref8x as TR8
from oracle.nets import ParamSource
# grad of <dx, gdx> + <dgamma, gdg> + <dbeta, gdb> with respect to (dz, x, gamma), float64 autograd
from valu_ref import bn_double_backward_64 as _bn_double_backward_64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _t64(t):
    return t.detach().to(DT)


# ---------------------------------------------------------------------------------------------- kernels


@pytest.mark.parametrize("m,c", [(37, 4), (37, 5), (37, 130), (4099, 32), (16 * 64 * 64, 130), (16 * 128 * 128, 32),
                                 (16 * 128 * 128, 4)])
@pytest.mark.parametrize("absent", [None, "gdx", "gdgamma", "gdbeta"])
def test_bn_train_bwd2_matches_float64_autograd(m, c, absent):
    from mpgan_amd import train_ops
    gen = torch.Generator(device=DEV).manual_seed(1000 * c + m % 997)
    x = torch.randn((m, c), device=DEV, generator=gen) * 1.7 + 0.4
    dz = torch.randn((m, c), device=DEV, generator=gen) * 1e-2
    gamma = torch.randn((c,), device=DEV, generator=gen)
    gamma[0] = 0.0
    gamma[1] = -abs(float(gamma[1])) - 0.5
    beta = torch.randn((c,), device=DEV, generator=gen)
    gdx = torch.randn((m, c), device=DEV, generator=gen) if absent != "gdx" else None
    gdg = torch.randn((c,), device=DEV, generator=gen) if absent != "gdgamma" else None
    gdb = torch.randn((c,), device=DEV, generator=gen) if absent != "gdbeta" else None
    eps = 1e-3
    _, mean, var = train_ops.bn_train_fwd(x, gamma, beta, eps)
    got = train_ops.bn_train_bwd2(dz, x, mean, var, gamma, eps, gdx, gdg, gdb)
    again = train_ops.bn_train_bwd2(dz, x, mean, var, gamma, eps, gdx, gdg, gdb)
    want = _bn_double_backward_64(dz, x, gamma, gdx, gdg, gdb, eps)
    for name, a, a2, b in zip(("g_dz", "g_x", "g_gamma"), got, again, want):
        assert torch.equal(a, a2), name                                   # block sums added in a fixed order
        assert torch.isfinite(a).all(), name
        r = rel(a.cpu().numpy(), b.cpu().numpy())
        assert r <= 1e-4, (name, r)


def _mbstd_64(x, group_size):
    """GAN.minibatch_stddev_layer (GAN.py:476-488) in float64, NHWC"""
    n, h, w, c = x.shape
    g = min(group_size, n)
    y = x.reshape(g, n // g, h, w, c)
    y = y - y.mean(0, keepdim=True)
    y = torch.sqrt((y * y).mean(0) + 1e-8)
    s = y.mean(dim=(1, 2, 3))                                             # [M]
    stat = s.repeat(g).reshape(n, 1, 1, 1).expand(n, h, w, 1)             # member g of group m is sample g * M + m
    return torch.cat([x, stat], dim=3)


def _mbstd_double_backward_64(x, dy, ggx, group_size):
    x, dy = _t64(x).requires_grad_(True), _t64(dy).requires_grad_(True)
    (dx,) = torch.autograd.grad(_mbstd_64(x, group_size), x, dy, create_graph=True)
    g_dy, g_x = torch.autograd.grad((dx * _t64(ggx)).sum(), (dy, x), allow_unused=True)
    return g_dy, (g_x if g_x is not None else torch.zeros_like(x))


@pytest.mark.parametrize("n,group,hwc", [(16, 4, (8, 8, 32)), (3, 4, (5, 7, 3)), (8, 4, (4, 4, 33)), (4, 1, (8, 8, 16)),
                                         (16, 4, (32, 32, 24))])
def test_minibatch_stddev_bwd2_matches_float64_autograd(n, group, hwc):
    from mpgan_amd import train_ops
    h, w, c = hwc
    gen = torch.Generator(device=DEV).manual_seed(n * 131 + c)
    x = torch.randn((n, h, w, c), device=DEV, generator=gen)
    dy = torch.randn((n, h, w, c + 1), device=DEV, generator=gen)
    ggx = torch.randn((n, h, w, c), device=DEV, generator=gen)
    g_dy, g_x = train_ops.minibatch_stddev_bwd2(ggx, dy, x, group)
    g_dy2, g_x2 = train_ops.minibatch_stddev_bwd2(ggx, dy, x, group)
    assert torch.equal(g_dy, g_dy2) and torch.equal(g_x, g_x2)
    assert torch.isfinite(g_x).all() and torch.isfinite(g_dy).all()
    w_dy, w_x = _mbstd_double_backward_64(x, dy, ggx, group)
    assert torch.equal(g_dy[..., :c], ggx)
    if min(group, n) == 1:
        # one member per group: u = 0, s = 1e-4; the statistic is a constant and every second derivative is exactly 0
        assert torch.equal(g_x, torch.zeros_like(g_x))
        assert torch.equal(g_dy[..., c], torch.zeros_like(g_dy[..., c]))
        assert float(w_x.abs().max()) == 0.0
        return
    assert rel(g_dy.cpu().numpy(), w_dy.cpu().numpy()) <= 1e-4
    assert rel(g_x.cpu().numpy(), w_x.cpu().numpy()) <= 1e-4


# ---------------------------------------------------------------------------------------------- trainer
def _mbstd_nchw(x, group):
    return _mbstd_64(x.permute(0, 2, 3, 1), group).permute(0, 3, 1, 2)


def _critic_64(p, scope, c, inp, percentage, first_gen, first_nn_arch, bn, mb_group, stats=None):
    """growing_disc / growing_disc_tempo (multipassGAN-8x.py:783-923) in float64 NCHW with the minibatch stddev layer
    (:847-848, :907-908) and batch norm in the tail convolutions (:850-854, :910-913)"""
    x = TR8.conv(p, scope + "%s_cfromDensity8" % c, inp)
    raw, top = inp, None
    for j in range(3, 0, -1):
        blk = scope + "%sBlock%d/" % (c, 2 ** j)
        if first_gen:
            raw = F.avg_pool2d(raw, 2)
        x1 = TR8.conv(p, blk + "%s_cA%d" % (c, 2 ** j), x, "lrelu")
        x2 = TR8.conv(p, blk + "%s_cB%d" % (c, 2 ** j), x1, "lrelu")
        top = F.avg_pool2d(x2, 2) if first_gen else x2
        old = TR8.conv(p, scope + "%s_cfromDensity%d" % (c, 2 ** (j - 1)), raw)
        x = TR8.lerp(old, top, percentage - (j - 1))
    head = top                                          # gan.layer: the last block's (pooled) x2
    if mb_group is not None:
        x = _mbstd_nchw(x, mb_group)
        head = x
    if not first_nn_arch:
        x1, _ = TR.conv_layer(p, scope + "%s_cA1" % c, x, "lrelu", batch_norm=bn, stats=stats)
        head, _ = TR.conv_layer(p, scope + "%s_cB1" % c, x1, None, batch_norm=bn, stats=stats)
    flat = head.permute(0, 2, 3, 1).reshape(head.shape[0], -1)
    w = p[scope + "%s_l61/weight" % c]
    return flat @ (w * TR8._ws(w, 1.0)) + p[scope + "%s_l61/bias" % c]


def _setup(cfg_kw, batch, seed, **kw):
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(**cfg_kw)
    tr = Trainer8x(cfg, device=DEV, seed=seed, **kw)
    ps = ParamSource(seed=seed)
    params = {n: ps.get(n, s.shape, s.kind) for n, s in tr.graph.variables.items()}
    with torch.no_grad():
        for n, t in tr.sess.params.items():
            t.copy_(torch.as_tensor(params[n], device=DEV))
    return tr, TR.to_params(params)


def _check_grads(names, got, want, bn_layers, prefix, cancel=None, agg=3e-4):
    """per tensor < 5e-3, aggregate < 3e-4 (the bounds of test_wgan_gp_gradients); the biases in front of a batch norm
    have an analytically zero gradient: compared absolutely, against the norm of the layer's weight gradient.
    cancel: name -> gradient of the real-sample term alone, for the offsets between the last normalisation and the score
    (<c>_cB1/beta, <c>_l61/bias): the same sum over every sample, so +1/B of the real and -1/B of the generated samples
    cancel and only the 1e-3 epsilon penalty is left (the d_l61/bias remark of test_wgan_gp_gradients); their error is
    held to 5e-3 of the terms that cancel.  agg: the aggregate bound (1e-3 for the second / third network's critics at
    tileSizeHigh, the bound of test_second_network_training_step)"""
    tot_d = tot_r = 0.0
    seen_bn = 0
    for nme, g in zip(names, got):
        if not nme.startswith(prefix):
            continue
        w = want[nme]
        gnp = g.cpu().numpy().astype(np.float64) if g is not None else np.zeros_like(w)
        layer = nme.rsplit("/", 1)[0]
        if nme.endswith("/bias") and layer.rsplit("/", 1)[-1] in bn_layers:
            wn = np.linalg.norm(want[layer + "/weight"])
            assert np.linalg.norm(gnp) <= 1e-4 * wn and np.linalg.norm(w) <= 1e-9 * wn, (nme, np.linalg.norm(gnp), wn)
            seen_bn += 1
            continue
        if np.abs(w).max() == 0.0:
            assert np.abs(gnp).max() < 1e-7, nme
            continue
        if cancel is not None and nme in cancel:
            err = np.linalg.norm(gnp - w) / np.linalg.norm(cancel[nme])
            assert err < 5e-3, (nme, err, rel(gnp, w))
        else:
            r = rel(gnp, w)
            assert r < 5e-3, (nme, r)
        tot_d += float(((gnp - w) ** 2).sum())
        tot_r += float((w ** 2).sum())
    assert seen_bn == 2 * bool(bn_layers)
    assert math.sqrt(tot_d / tot_r) < agg, math.sqrt(tot_d / tot_r)


def _spatial_disc_loss_64(p, xs, ys_nchw, gen_y_nchw, lf, percentage, tile, channels, first_gen, first_nn_arch, bn, mb,
                          stats=None):
    th = tile * 8
    low = torch.tensor(O.resize_nearest_tf1(np.asarray(xs, np.float32).reshape(-1, tile, tile, channels)[..., :1], th, th),
                       dtype=DT).permute(0, 3, 1, 2)
    mb_group = 4 if mb else None

    def critic(high):
        return _critic_64(p, "spatial-disc/", "d", torch.cat([low, high], dim=1), percentage, first_gen, first_nn_arch, bn,
                          mb_group, stats)

    disc, gen = critic(ys_nchw), critic(gen_y_nchw)
    loss = (-disc).mean() + gen.mean()
    lf = torch.tensor(np.asarray(lf), dtype=DT).reshape(-1, 1, 1, 1)
    y_gp = (lf * ys_nchw + (1 - lf) * gen_y_nchw).requires_grad_(True)
    (g,) = torch.autograd.grad(critic(y_gp).mean(), y_gp, create_graph=True)
    norm = torch.sqrt(((g.reshape(g.shape[0], -1) + 1e-4) ** 2).sum(dim=1))
    return loss + (disc ** 2).mean() * 1e-3 + (10.0 * (norm - 1.0) ** 2).mean(), disc


SPATIAL_CASES = {
    # first network, firstNNArch 0: BN in d_cA1 / d_cB1, statistic channel in front of them
    "first_nn0_bn_mb": (dict(tileSizeLow=8, upRes=8, n_inputChannels=4, first_nn_arch=False, start_fms=32, max_fms=32), 8,
                        True, True, 2.6),
    # first network, firstNNArch 1: the head reads the concatenated statistic channel
    "first_nn1_mb": (dict(tileSizeLow=8, upRes=8, n_inputChannels=4, first_nn_arch=True, use_mb_stddev=True, start_fms=32,
                          max_fms=32), 3, False, True, 3.0),
    # second / third network (upsampling_mode 1): no pooling, tail at tileSizeHigh
    "later_bn_mb": (dict(tileSizeLow=4, upRes=8, n_inputChannels=4, upsampling_mode=1, first_nn_arch=False, filterSize=5,
                         start_fms=32, max_fms=32), 4, True, True, 2.3),
}


@pytest.mark.parametrize("case", sorted(SPATIAL_CASES))
def test_spatial_critic_gp_gradients_with_bn_and_mb_stddev(case):
    cfg_kw, batch, bn, mb, percentage = SPATIAL_CASES[case]
    cfg_kw = dict(cfg_kw, use_mb_stddev=mb)
    tr, p = _setup(cfg_kw, batch, seed=11, batch_norm=bn)
    tile, C = cfg_kw["tileSizeLow"], cfg_kw["n_inputChannels"]
    th = tile * 8
    first_gen = cfg_kw.get("upsampling_mode", 2) == 2
    rng = np.random.default_rng(17)
    xs = rng.random((batch, tile * tile * C)).astype(np.float32)
    lf = rng.random((batch, 1)).astype(np.float32)
    if first_gen:
        ys = rng.random((batch, th * th)).astype(np.float32)
        ys_t = torch.tensor(ys, dtype=DT).reshape(-1, 1, th, th)
    else:
        ys = rng.random((batch, th * th * 2)).astype(np.float32)
        ys_t = torch.tensor(ys, dtype=DT).reshape(-1, th, th, 2)[..., 0:1].permute(0, 3, 1, 2).contiguous()
    L = tr.losses(xs, ys, percentage, lf)
    gd = torch.autograd.grad(L["disc_loss"], tr.opt_d.params, allow_unused=True)
    gen_y = L["gen_y"].detach().to("cpu", DT).reshape(-1, 1, th, th)
    loss, disc = _spatial_disc_loss_64(p, xs, ys_t, gen_y, lf, percentage, tile, C, first_gen, cfg_kw["first_nn_arch"], bn,
                                       mb)
    # the loss bounds of test_growing_nets_forward / test_second_network_training_step
    tol = 2e-4 if first_gen else 3e-4
    assert abs(float(L["disc_loss"].detach()) - float(loss)) <= tol * max(abs(float(loss)), 1e-2)
    want = TR.grads(loss, p, "d_")
    assert sorted(want) == tr.opt_d.names
    offsets = ["spatial-disc/d_l61/bias"] + (["spatial-disc/d_cB1/beta"] if bn else [])
    real = TR.grads((-disc).mean(), p, "d_")
    _check_grads(tr.opt_d.names, gd, want, ("d_cA1", "d_cB1") if bn else (), "spatial-disc/", {n: real[n] for n in offsets},
                 3e-4 if first_gen else 1e-3)
    d, g = tr.train_step(xs, ys, 3.0)
    assert np.isfinite(float(d)) and np.isfinite(float(g))


def test_temporal_critic_gp_gradients_with_bn_and_mb_stddev():
    """growing_disc_tempo with batch norm in t_cA1 / t_cB1 and the statistic of group size 1 (-8x.py:907-908: a constant
    channel of 1e-4), second network: the critic's gradients of t_disc_loss, penalty included"""
    import contextlib
    import io
    import random
    from mpgan_amd import tilecreator_t as tc
    tile, C = 4, 4
    th = tile * 8
    rng = np.random.default_rng(43)
    with contextlib.redirect_stdout(io.StringIO()):
        tiCr = tc.TileCreator(tileSizeLow=tile, simSizeLow=8, upres=8, dim=2, dim_t=3, densityMinimum=0.0,
                              channelLayout_low="d,vx,vy,vz", channelLayout_high="d,d")
        tiCr.addData(rng.random((4, 1, 8, 8, 12)).astype(np.float32), rng.random((4, 1, 64, 64, 6)).astype(np.float32))
    random.seed(5)
    xts, yts, ypos = tiCr.selectRandomTempoTiles(6, True, False, n_t=3, dt=0.5)
    cfg_kw = dict(tileSizeLow=tile, upRes=8, n_inputChannels=C, upsampling_mode=1, first_nn_arch=False, filterSize=5,
                  start_fms=32, max_fms=32, use_mb_stddev=True)
    tr, p = _setup(cfg_kw, 2, seed=4, batch_norm=True, use_tempo=True)
    packed = []
    frames = tr._frames_as_channels

    def record(*a, **k):
        out = frames(*a, **k)
        packed.append(out.detach().to("cpu", DT))
        return out

    tr._frames_as_channels = record
    lf_t = rng.random((2, 1)).astype(np.float32)
    L = tr.tempo_losses(xts, yts, ypos, 2.7, lf_t)
    gt = torch.autograd.grad(L["t_disc_loss"], tr.opt_t.params, allow_unused=True)
    fake, real = packed[0], packed[1]
    to_img = lambda v: v.reshape(-1, th, th, 3).permute(0, 3, 1, 2)           # noqa: E731

    def critic(v):
        return _critic_64(p, "tempo-disc/", "t", to_img(v), 2.7, False, False, True, 1)

    gen_s, disc_s = critic(fake), critic(real)
    loss = (-disc_s).mean() + gen_s.mean()
    lf = torch.tensor(lf_t, dtype=DT).reshape(-1, 1)
    y_gp = (lf * real + (1 - lf) * fake).requires_grad_(True)
    (g,) = torch.autograd.grad(critic(y_gp).mean(), y_gp, create_graph=True)
    norm = torch.sqrt(((g.reshape(-1, th * th, 3) + 1e-4) ** 2).sum(dim=1))
    loss = loss + (disc_s ** 2).mean() * 1e-3 + (10.0 * (norm - 1.0) ** 2).mean()
    assert abs(float(L["t_disc_loss"].detach()) - float(loss)) <= 3e-4 * max(abs(float(loss)), 1e-2)
    want = {k: v for k, v in TR.grads(loss, p, "t_").items() if k.startswith("tempo-disc")}
    assert sorted(want) == tr.opt_t.names
    real_g = TR.grads((-disc_s).mean(), p, "t_")
    offsets = ("tempo-disc/t_l61/bias", "tempo-disc/t_cB1/beta")
    _check_grads(tr.opt_t.names, gt, want, ("t_cA1", "t_cB1"), "tempo-disc/", {n: real_g[n] for n in offsets}, 1e-3)
    tr._frames_as_channels = frames
    xs = rng.random((2, tile * tile * C)).astype(np.float32)
    ys2 = rng.random((2, th * th * 2)).astype(np.float32)
    d, g = tr.train_step(xs, ys2, 3.0, tempo=(xts, yts, ypos))
    assert np.isfinite(float(d)) and np.isfinite(float(g))


def test_moving_averages_advance_once_per_critic_evaluation():
    """one losses() call evaluates the spatial critic three times (real, generated, y_gp): the moving averages of d_cA1 /
    d_cB1 take three steps moving = decay * moving + (1 - decay) * batch, with the batch moments of those evaluations"""
    cfg_kw = dict(tileSizeLow=4, upRes=8, n_inputChannels=4, upsampling_mode=1, first_nn_arch=False, filterSize=5,
                  start_fms=32, max_fms=32, use_mb_stddev=True)
    tr, p = _setup(cfg_kw, 4, seed=12, batch_norm=True)
    tile, C, th, batch = 4, 4, 32, 4
    rng = np.random.default_rng(23)
    xs = rng.random((batch, tile * tile * C)).astype(np.float32)
    ys = rng.random((batch, th * th * 2)).astype(np.float32)
    lf = rng.random((batch, 1)).astype(np.float32)
    names = ["spatial-disc/%s/moving_%s" % (l, k) for l in ("d_cA1", "d_cB1") for k in ("mean", "variance")]
    before = {n: tr.sess.params[n].detach().to("cpu", DT).clone() for n in names}
    L = tr.losses(xs, ys, 2.5, lf)
    after = {n: tr.sess.params[n].detach().to("cpu", DT) for n in names}
    gen_y = L["gen_y"].detach().to("cpu", DT).reshape(-1, 1, th, th)
    ys_t = torch.tensor(ys, dtype=DT).reshape(-1, th, th, 2)[..., 0:1].permute(0, 3, 1, 2).contiguous()
    seen = {}

    class Stats(dict):
        def __setitem__(self, k, v):
            seen.setdefault(k, []).append(v)

    _spatial_disc_loss_64(p, xs, ys_t, gen_y, lf, 2.5, tile, C, False, False, True, True, stats=Stats())
    decay = tr.sess.bn_decay
    for layer in ("d_cA1", "d_cB1"):
        sc = "spatial-disc/" + layer
        evals = seen[sc]
        assert len(evals) == 3
        for k, key in ((0, "mean"), (1, "variance")):
            m0 = before[sc + "/moving_" + key]
            want = m0.clone()
            for st in evals:
                want = decay * want + (1.0 - decay) * st[k]
            step = want - decay ** 3 * m0
            got = after[sc + "/moving_" + key] - decay ** 3 * m0
            assert rel(got.numpy(), step.numpy()) < 2e-3, (sc, key, rel(got.numpy(), step.numpy()))


# ---------------------------------------------------------------------------------------------- driver
def _run(script, args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_8x_training_driver_gp_with_batch_norm_and_mb_stddev(tmp_path):
    """multipassGAN-8x.py with use_wgan_gp 1, batchNorm 1, use_mb_stddev 1, firstNNArch 0 (reduced sizes, synthetic .uni
    data, spatial + temporal critics): it trains and writes finite checkpoints that hold the tail convolutions' BN"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import checkpoint, uniio
    from mpgan_amd.synthetic import synthetic_volume
    sim, frames = 8, 11
    d = tmp_path / "data" / "sim_1005"
    d.mkdir(parents=True)
    (tmp_path / "models").mkdir()
    for f in range(frames):
        v = synthetic_volume(sim, 4, f)
        uniio.writeUni(str(d / ("density_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim), v[..., 0:1] + 0.05)
        uniio.writeUni(str(d / ("velocity_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
        for up, nm in ((2, "density_low_2_%04d.uni"), (4, "density_low_4_%04d.uni"), (8, "density_high_%04d.uni")):
            hi = synthetic_volume(sim * up, 1, 100 * up + f) + 0.05
            uniio.writeUni(str(d / (nm % f)), uniio.make_header(sim * up, sim * up, sim * up), hi)
    args = ["randSeed", 16131119, "upRes", 8, "use_res_net", 1, "batchNorm", 1, "use_mb_stddev", 1, "pixelNorm", 1, "out", 0,
            "pretrain", 0, "pretrainDisc", 0, "tileSize", 8, "simSize", sim, "use_LSGAN", 0, "use_wgan_gp", 1, "lambda", 1.0,
            "lambda2", 0.0, "discRuns", 1, "genRuns", 1, "alwaysSave", 1, "fromSim", 1005, "toSim", 1005, "outputInterval", 2,
            "genTestImg", -1, "dropout", 0.5, "dataDim", 2, "batchSize", 4, "useVelocities", 1, "useVorticities", 0,
            "useK_Eps_Turb", 0, "useFlags", 0, "gif", 0, "genModel", "gen_resnet", "discModel", "disc_binclass",
            "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/", "lambda_t", 1.0,
            "lambda_t_l2", 0.0, "frame_max", 2, "frame_min", 0, "data_fraction", 1.0, "adv_flag", 1, "adv_mode", 0,
            "dataAugmentation", 0, "premadeTiles", 0, "rot", 1, "minScale", 0.85, "maxScale", 1.15, "flip", 1, "decayLR", 1,
            "adam_beta1", 0.0, "adam_beta2", 0.99, "learningRate", 0.0001, "lossScaling", 1, "stageIter", 1, "decayIter", 1,
            "maxFms", 32, "startFms", 32, "filterSize", 3, "upsamplingMode", 2, "upsampledData", 0, "load_model_test", -1,
            "load_model_no", -1, "firstNNArch", 0, "add_adj_idcs", 1, "usePixelShuffle", 0, "addBicubicUpsample", 1,
            "startingIter", 0, "useVelInTDisc", 0, "upsampleMode", 1, "gpu", 0, "saveInterval", 100]
    out = _run("multipassGAN-8x.py", args, str(tmp_path))
    assert "TRAINING FINISHED" in out
    test_dir = tmp_path / "models" / "test_0000"
    ckpts = sorted(f[:-len(".npz")] for f in os.listdir(str(test_dir)) if f.startswith("model_0") and f.endswith(".ckpt.npz"))
    assert ckpts, os.listdir(str(test_dir))
    last = checkpoint.load(str(test_dir / ckpts[-1]))
    assert all(np.isfinite(v).all() for v in last.values())
    for name in ("spatial-disc/d_cA1/gamma", "spatial-disc/d_cB1/beta", "spatial-disc/d_cA1/moving_mean",
                 "tempo-disc/t_cA1/gamma"):
        assert name in last, name
    assert not np.array_equal(last["spatial-disc/d_cA1/moving_mean"], np.zeros_like(last["spatial-disc/d_cA1/moving_mean"]))
