"""`useVelInTDisc` and `gDrop` of the 8x training on the GPU (multipassGAN-8x.py:1185,1204-1208,878 and :155,601-603,746-750):

* mpg_tempo_vel_pack / _bwd bit for bit against the unfused composition on the device (concat with scale *
  mpg_resize_bilinear, reshape, transpose) and its autograd gradient;
* the [filterSize + 2, filterSize] filters of the temporal critic on ConvFn / ConvDgradFn / ConvWgradFn, with the
  comparisons and bounds of test_conv_triad_gpu.py;
* Trainer8x(useVelInTDisc) against the float64 restatement tempo_vel_ref.tempo_losses_8x_vel, at the bounds of
  test_train8x_gpu.test_temporal_critic_losses_and_gradients;
* the gDrop noise: absent at strength 0 (bit-identical losses), N(0, (s sqrt(C))^2) otherwise;
* the 8x driver with both switches.
"""
import contextlib
import io
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_triad_ref as CT
import tempo_vel_ref as R
import test_conv_triad_gpu as TG
from oracle import train_ref as TR
from oracle.nets import ParamSource

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMS = [(1, 4, 32), (2, 4, 32), (3, 5, 40), (1, 8, 64)]


def _inputs(B, tl, th):
    """frames: every value its own index (no wrong permutation passes); x_t: random, the first and last source rows and
    columns (where the upper neighbour is clamped) set apart from the interior by +-8"""
    P = th * th
    frames = torch.arange(3 * B * P, dtype=torch.float32, device=DEV).reshape(3 * B, th, th, 1)
    rng = np.random.default_rng(1000 * B + th)
    x = rng.standard_normal((3 * B, tl, tl, 4)).astype(np.float32)
    x[:, 0] += 8
    x[:, -1] -= 8
    x[:, :, 0] += 8
    x[:, :, -1] -= 8
    return frames, torch.tensor(x, device=DEV)


def _composition(ops, frames, x_t, scale):
    th = frames.shape[1]
    vel = x_t[..., 1:4].contiguous()
    f4 = torch.cat([frames, scale * ops.resize_bilinear(vel, th, th)], -1)
    return f4.reshape(-1, 3, th * th).permute(0, 2, 1).reshape(frames.shape[0] // 3, -1)


# ---------------------------------------------------------------------------------------------------- the kernel pair
@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "B%d_%d_%d" % g)
def test_pack_forward_bit_for_bit(gpu_ops, geom, scale):
    from mpgan_amd import train_ops
    B, tl, th = geom
    frames, x_t = _inputs(B, tl, th)
    out = torch.full((B, 12 * th * th), float("nan"), device=DEV)
    got = train_ops.tempo_vel_pack(frames, x_t, float(scale), out=out)
    assert got is out and not torch.isnan(out).any()
    want = _composition(gpu_ops, frames, x_t, float(scale))
    assert torch.equal(out, want)
    # and the composition is the reference's: float32 numpy, every operation rounded where the kernel may fuse a
    # multiply-add.  Each of the three lerps a + (b - a) l differs by at most 2 ulp of max |v| between the two forms
    # (|b - a| <= 2 max |v|), the scaling is exact (a power of two): 8 * 2^-24 * scale * max |v|
    ref = R.pack_ref(frames.cpu().numpy(), x_t.cpu().numpy(), scale)
    _, _, _, c = R.index_map(B, th * th)
    g = out.cpu().numpy().reshape(-1)
    assert np.array_equal(g[c == 0], ref.reshape(-1)[c == 0])
    vmax = float(x_t[..., 1:4].abs().max())
    assert np.abs(g - ref.reshape(-1)).max() <= 8 * 2.0 ** -24 * scale * vmax


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "B%d_%d_%d" % g)
def test_pack_backward_bit_for_bit(gpu_ops, geom):
    from mpgan_amd import train_ops
    from mpgan_amd.train import TempoVelPackFn
    B, tl, th = geom
    frames, x_t = _inputs(B, tl, th)
    dout = torch.randn((B, 12 * th * th), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    fr = frames.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(_composition(gpu_ops, fr, x_t, 4.0), fr, dout)
    dframes = torch.full((3 * B, th, th, 1), float("nan"), device=DEV)
    got = train_ops.tempo_vel_pack_bwd(dout, th, out=dframes)
    assert got is dframes and not torch.isnan(dframes).any()
    assert torch.equal(dframes, want)
    # through the Function
    fr2 = frames.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad(TempoVelPackFn.apply(fr2, x_t, 4.0), fr2, dout)
    assert torch.equal(g2, want)
    # nothing in the velocity slots of dout reaches dframes
    _, _, _, c = R.index_map(B, th * th)
    poisoned = dout.clone().reshape(-1)
    poisoned[torch.as_tensor(c != 0, device=DEV)] = float("nan")
    assert torch.equal(train_ops.tempo_vel_pack_bwd(poisoned.reshape(dout.shape), th), want)


def test_pack_is_once_differentiable(gpu_ops):
    from mpgan_amd.train import TempoVelPackFn
    frames, x_t = _inputs(1, 4, 8)
    fr = frames.clone().requires_grad_(True)
    out = TempoVelPackFn.apply(fr, x_t, 2.0)
    # the square makes the upstream gradient 2 out depend on fr, so the first gradient carries the backward's own node and
    # nothing else can raise (as test_train_gpu.test_first_order_function_refuses_second_derivative does it)
    (g,) = torch.autograd.grad((out * out).sum(), fr, create_graph=True)
    assert g.grad_fn is not None
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g.sum().backward()


def test_pack_argument_checks(gpu_ops):
    from mpgan_amd import _lib, train_ops
    frames, x_t = _inputs(1, 4, 8)
    with pytest.raises(_lib.MpgError):                      # rows no multiple of 3
        train_ops.tempo_vel_pack(frames[:2], x_t[:2], 2.0)
    with pytest.raises(_lib.MpgError):                      # th % tl != 0
        train_ops.tempo_vel_pack(frames, torch.zeros((3, 3, 3, 4), device=DEV), 2.0)
    with pytest.raises(_lib.MpgError):                      # three channels: no velocity at 1..3
        train_ops.tempo_vel_pack(frames, x_t[..., :3].contiguous(), 2.0)
    with pytest.raises(_lib.MpgError):
        train_ops.tempo_vel_pack_bwd(torch.zeros((1, 12 * 64 + 1), device=DEV), 8)
    lib = _lib.load()
    assert lib.mpg_tempo_vel_pack(None, None, None, 1, 4, 8, 2.0, None) != 0
    assert lib.mpg_tempo_vel_pack_bwd(None, None, 1, 8, None) != 0


# ---------------------------------------------------------------------------------------------------- tall filters
@pytest.mark.parametrize("case", R.TALL_CASES, ids=repr)
def test_tall_filter_triad_exact(gpu_ops, case):
    got = TG.hip_outputs(case, "exact", gpu_ops.PREC_F16X3)
    want = CT.reference(case, "exact")
    problems = []
    for name in CT.OUTPUTS:
        w32 = want[name].astype(np.float32)
        msg = CT.mismatch_report(got[name], w32, name)
        TG.report(case, "exact", gpu_ops.PREC_F16X3, name, CT.rel_l2(got[name], want[name]) if msg else 0.0, 0.0)
        if msg:
            problems.append(msg)
    TG.check_zeros(got, problems)
    assert not problems, "\n".join([repr(case)] + problems)


@pytest.mark.parametrize("kind", ["normal", "small"])
@pytest.mark.parametrize("case", R.TALL_CASES, ids=repr)
def test_tall_filter_triad_rel_l2(gpu_ops, case, kind):
    got = TG.hip_outputs(case, kind, gpu_ops.PREC_F16X3)
    want = CT.reference(case, kind)
    problems = []
    for name in CT.OUTPUTS:
        assert got[name].shape == want[name].shape and got[name].dtype == np.float32, name
        err, bound = CT.rel_l2(got[name], want[name]), case.tol(name)
        TG.report(case, kind, gpu_ops.PREC_F16X3, name, err, bound)
        if not err < bound:
            problems.append("%s: relative L2 %.3e, bound %.1e" % (name, err, bound))
    TG.check_zeros(got, problems)
    assert not problems, "\n".join([repr(case), kind] + problems)


# ---------------------------------------------------------------------------------------------------- trainer parity
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _trainer(tile=8, fms=32, seed=9, cfg_kw=None, **kw):
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(tileSizeLow=tile, upRes=8, n_inputChannels=4, start_fms=fms, max_fms=fms, **(cfg_kw or {}))
    tr = Trainer8x(cfg, device=DEV, seed=seed, **kw)
    ps = ParamSource(seed=seed)
    params = {n: ps.get(n, s.shape, s.kind) for n, s in tr.graph.variables.items()}
    with torch.no_grad():
        for n, t in tr.sess.params.items():
            t.copy_(torch.as_tensor(params[n], device=DEV))
    return tr, params


def _tempo_batch(tile, up, rows=6):
    """coherent frame triples of the set-up of test_temporal_critic_losses_and_gradients, targets at tile * up"""
    from mpgan_amd import tilecreator_t as tc
    rng = np.random.default_rng(41)
    with contextlib.redirect_stdout(io.StringIO()):
        tiCr = tc.TileCreator(tileSizeLow=tile, simSizeLow=16, upres=up, dim=2, dim_t=3, densityMinimum=0.0,
                              channelLayout_low="d,vx,vy,vz", channelLayout_high="d")
        tiCr.addData(rng.random((4, 1, 16, 16, 12)).astype(np.float32),
                     rng.random((4, 1, 16 * up, 16 * up, 3)).astype(np.float32))
    random.seed(2)
    xts, yts, ypos = tiCr.selectRandomTempoTiles(rows, True, False, n_t=3, dt=0.5)
    n = xts.shape[0]
    return xts.reshape(n, -1), yts.reshape(n, -1), ypos.reshape(n, -1)


@pytest.mark.parametrize("adv_mode,first_nn_arch,percentage,fms", [(0, True, 3.0, 32), (1, True, 3.0, 32), (0, False, 3.0, 256),
                                                                   (1, False, 3.0, 256), (0, True, 1.5, 32)])
def test_trainer_with_velocity_in_the_temporal_critic(adv_mode, first_nn_arch, percentage, fms):
    """t_disc_loss / g_loss_t and their gradients with the 12-channel critic input, the [4B, 1] lerp factor and the
    tall filters; percentage 1.5: upresFac 4, the advection at 4 * tileSizeLow.

    Width: 32 as in test_train8x_gpu.make for firstNNArch.  Without firstNNArch the first network's generator divides
    startFms down to startFms / 16 channels, and at startFms 32 .. 128 its pixel norm (epsilon 1e-8) runs over 2 .. 8
    channels: pixels whose few channels are all next to zero make d g_loss_t / d generator ill-conditioned.  Measured on
    the restatement alone, float32 against float64 torch on the CPU, worst relative error of a generator gradient tensor
    on this test's data: 1e-2 (startFms 32, every one of six parameter seeds between 1e-2 and 1e-1), 4e-2 (64),
    2e-3 (128), 1.4e-6 (256); the t_ gradients stay at 1e-5 throughout.  No float32 evaluation holds 5e-3 on the narrow
    ones, so that case runs at the reference's own width, startFms = maxFms = 256 (the Cfg8x default)."""
    tile = 8
    up = 2 ** int(math.ceil(percentage))
    xts, yts, ypos = _tempo_batch(tile, up)
    tr, params = _trainer(tile=tile, fms=fms, cfg_kw=dict(useVelInTDisc=True, first_nn_arch=first_nn_arch), use_tempo=True,
                          adv_mode=adv_mode)
    p = TR.to_params(params)
    lf_t = np.random.default_rng(7).random((8, 1)).astype(np.float32)          # [4B, 1], B = 2
    L = tr.tempo_losses(xts, yts, ypos, percentage, lf_t)
    Lr = R.tempo_losses_8x_vel(p, xts, yts, ypos, tile, percentage, lf_t, first_nn_arch=first_nn_arch, adv_mode=adv_mode)
    for k in ("t_disc_loss", "g_loss_t"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        print("tempo-vel %s adv_mode %d first_nn_arch %d percentage %.1f: %.8g vs %.8g" % (k, adv_mode, first_nn_arch,
                                                                                        percentage, a, b))
        assert abs(a - b) <= 2e-4 * max(abs(b), 1e-2), (k, a, b)
    gt = torch.autograd.grad(L["t_disc_loss"], tr.opt_t.params, allow_unused=True, retain_graph=True)
    gg = torch.autograd.grad(L["g_loss_t"], tr.opt_g.params, allow_unused=True)
    rt = {k: v for k, v in TR.grads(Lr["t_disc_loss"], p, "t_").items() if k.startswith("tempo-disc")}
    rg = TR.grads(Lr["g_loss_t"], p, "g_")
    assert sorted(rt) == tr.opt_t.names
    worst = 0.0
    for names, got, want in ((tr.opt_t.names, gt, rt), (tr.opt_g.names, gg, rg)):
        for nme, g in zip(names, got):
            w = want[nme]
            gnp = g.cpu().numpy().astype(np.float64) if g is not None else np.zeros_like(w)
            if np.abs(w).max() == 0.0:
                assert np.abs(gnp).max() < 1e-7, nme
                continue
            worst = max(worst, rel(gnp, w))
            assert rel(gnp, w) < 5e-3, (nme, rel(gnp, w))
    print("tempo-vel worst per-tensor gradient error %.3e" % worst)
    rng = np.random.default_rng(3)
    xs = rng.random((2, tile * tile * 4)).astype(np.float32)
    ys = rng.random((2, (tile * up) ** 2)).astype(np.float32)
    d, g = tr.train_step(xs, ys, percentage, tempo=(xts, yts, ypos))
    assert np.isfinite(float(d)) and np.isfinite(float(g))


# ---------------------------------------------------------------------------------------------------- gDrop
def _gdrop_pair(first_nn_arch):
    """an LSGAN trainer with gDrop and one without on the same variables, with a spatial and a temporal batch"""
    kw = dict(use_wgan_gp=False, use_LSGAN=True, use_tempo=True, adv_mode=0)
    noisy, params = _trainer(cfg_kw=dict(gDrop=True, first_nn_arch=first_nn_arch), **kw)
    plain, params2 = _trainer(cfg_kw=dict(first_nn_arch=first_nn_arch), **kw)
    assert sorted(params) == sorted(params2)
    rng = np.random.default_rng(3)
    xs = rng.random((2, 8 * 8 * 4)).astype(np.float32)
    ys = rng.random((2, 64 * 64)).astype(np.float32)
    return noisy, plain, xs, ys, _tempo_batch(8, 8)


@pytest.mark.parametrize("first_nn_arch", [True, False])
def test_gdrop_at_strength_zero_changes_nothing(first_nn_arch):
    """bit for bit.  l1_loss, disc_loss_layer and with them gen_loss_complete are sums of mpg_pair_reduce, which adds its
    (at most 1024) block sums with float atomics in the order the blocks finish: two runs of ONE trainer differ in their
    last bits.  For those the tensors that enter the sums (generator output, every feature layer of both critic passes)
    are compared bit for bit, and the sums within 1024 roundings of a sum of non-negative terms, 1024 * 2^-24."""
    noisy, plain, xs, ys, tempo = _gdrop_pair(first_nn_arch)
    for kw in ({}, dict(gdrop_str_d=0.0)):
        a, b = noisy.losses(xs, ys, 3.0, **kw), plain.losses(xs, ys, 3.0)
        for k in ("disc_loss", "d_loss_y", "d_loss_g", "g_loss_d", "gen_y"):
            assert torch.equal(a[k].detach(), b[k].detach()), k
        for k in ("l1_loss", "disc_loss_layer", "gen_loss_complete"):
            assert abs(float(a[k].detach()) - float(b[k].detach())) <= 1024 * 2.0 ** -24 * abs(float(b[k].detach())), k
    feats = []
    for tr in (noisy, plain):
        feeds = {tr.x: xs, tr.x_disc: xs, tr.y_in: ys, tr.percentage: 3.0}
        if tr is noisy:
            feeds[tr.gdrop_str_d] = 0.0
        with torch.no_grad():
            feats.append(tr.sess.run(list(tr.f_y) + list(tr.f_g), feeds))
    assert len(feats[0]) == len(feats[1]) > 0 and all(torch.equal(u, v) for u, v in zip(*feats))
    a, b = noisy.tempo_losses(*tempo, 3.0, gdrop_str_t=0.0), plain.tempo_losses(*tempo, 3.0)
    for k in ("t_disc_loss", "g_loss_t", "t_loss_y", "t_loss_g"):
        assert torch.equal(a[k].detach(), b[k].detach()), k
    # and at a positive strength it changes the critic outputs, differently every run
    c = noisy.losses(xs, ys, 3.0, gdrop_str_d=0.1)
    d = noisy.losses(xs, ys, 3.0, gdrop_str_d=0.1)
    assert not torch.equal(c["d_loss_y"].detach(), plain.losses(xs, ys, 3.0)["d_loss_y"].detach())
    assert not torch.equal(c["d_loss_y"].detach(), d["d_loss_y"].detach())


def _first_noise_node(fetch, scope):
    """the gaussian_noise node feeding the first growing block (<p>_cA8) below `fetch`"""
    seen, stack = set(), [fetch]
    while stack:
        n = stack.pop()
        if n.id in seen:
            continue
        seen.add(n.id)
        if n.op == "conv2d" and n.inputs[0].op == "gaussian_noise" and n.inputs[1].attrs["var"].startswith(scope):
            return n.inputs[0]
        stack.extend(n.inputs)
    raise AssertionError("no noise node below %r" % (fetch,))


@pytest.mark.parametrize("s", [0.05, 0.3])
def test_gdrop_noise_statistics(s):
    """the first noisy conv input of the spatial critic minus its clean value: mean 0 within 4 sigma / sqrt(N) and
    standard deviation s sqrt(C) within 5 %, on N = 8 * 64 * 64 * 4 = 131072 elements"""
    noisy, _ = _trainer(cfg_kw=dict(gDrop=True), use_wgan_gp=False, use_LSGAN=True)
    rng = np.random.default_rng(3)
    xs = rng.random((8, 8 * 8 * 4)).astype(np.float32)
    ys = rng.random((8, 64 * 64)).astype(np.float32)
    node = _first_noise_node(noisy.disc, "spatial-disc/dBlock8/d_cA8")
    clean_node = node.inputs[0]
    feeds = {noisy.x_disc: xs, noisy.y_in: ys, noisy.percentage: 3.0}

    def strength(v):
        f = dict(feeds)
        f[noisy.gdrop_str_d] = v
        return f

    runs = []
    for _ in range(2):
        with torch.no_grad():
            x_noisy, x_clean = noisy.sess.run([node, clean_node], strength(s))
        runs.append((x_noisy - x_clean).double())
    diff = runs[0]
    C, N = x_clean.shape[-1], diff.numel()
    assert N >= 10 ** 5 and tuple(diff.shape) == tuple(x_clean.shape)
    sigma = s * math.sqrt(C)
    print("gdrop s %.2f C %d N %d: mean %.3e (bound %.3e) std %.5f (sigma %.5f)" % (
        s, C, N, float(diff.mean()), 4 * sigma / math.sqrt(N), float(diff.std()), sigma))
    assert abs(float(diff.mean())) <= 4 * sigma / math.sqrt(N)
    assert abs(float(diff.std()) - sigma) <= 0.05 * sigma
    assert not torch.equal(runs[0], runs[1])                # fresh values every run
    with torch.no_grad():                                   # strength 0: the clean tensor itself
        x0, xc = noisy.sess.run([node, clean_node], strength(0.0))
    assert x0 is xc


def test_gdrop_lsgan_steps_with_noise():
    noisy, plain, xs, ys, tempo = _gdrop_pair(False)
    L = noisy.losses(xs, ys, 3.0, gdrop_str_d=0.2)
    gd = torch.autograd.grad(L["disc_loss"], noisy.opt_d.params, allow_unused=True)
    assert all(g is None or torch.isfinite(g).all() for g in gd)
    assert sum(int(g is not None and float(g.abs().max()) > 0) for g in gd) >= len(gd) - 6
    Ld = noisy.disc_step(xs, ys, 3.0, gdrop_str_d=0.2)
    Lt = noisy.tempo_disc_step(*tempo, 3.0, gdrop_str_t=0.2)
    Lg = noisy.gen_step(xs, ys, 3.0, tempo)
    for v in (Ld["disc_loss"], Lt["t_disc_loss"], Lg["gen_loss_complete"], Lg["d_sig_g"], Lg["t_sig_g"]):
        assert np.isfinite(float(v.detach()))
    d, g = noisy.train_step(xs, ys, 3.0, tempo=tempo, gdrop_str_d=0.1, gdrop_str_t=0.1)
    assert np.isfinite(float(d)) and np.isfinite(float(g))
    out = noisy.evaluate(xs, ys, xs, ys, tempo=tempo, tempo_test=tempo, percentage=3.0, gdrop_str_d=0.1, gdrop_str_t=0.1)
    assert all(np.isfinite(float(v)) for v in out.values())


def test_gdrop_with_wgan_gp_is_refused():
    from mpgan_amd import _lib
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(tileSizeLow=8, upRes=8, n_inputChannels=4, start_fms=32, max_fms=32, gDrop=True)
    with pytest.raises(_lib.MpgError, match="use_LSGAN"):
        Trainer8x(cfg, device=DEV, use_wgan_gp=True, use_LSGAN=False)


# ---------------------------------------------------------------------------------------------------- driver
def _driver(args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", "multipassGAN-8x.py")] + [str(a) for a in args]
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_8x_driver_with_both_switches(tmp_path):
    """a short 8x training with useVelInTDisc 1 and gDrop 1 under LSGAN on the synthetic simulation of
    test_drivers_gpu.test_8x_training_driver: it trains through the three stages, prints both noise strengths, writes a
    checkpoint with the tall temporal filters; useVelInTDisc 1 without velocities is refused"""
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
    args = ["randSeed", 16131119, "upRes", 8, "use_res_net", 1, "batchNorm", 0, "pixelNorm", 1, "out", 0, "tileSize", 8,
            "simSize", sim, "use_LSGAN", 1, "use_wgan_gp", 0, "gDrop", 1, "useVelInTDisc", 1, "lambda", 1.0, "lambda2", 0.0,
            "discRuns", 1, "genRuns", 1, "fromSim", 1005, "toSim", 1005, "outputInterval", 1, "genTestImg", -1, "dataDim", 2,
            "batchSize", 3, "useVelocities", 1, "basePath", str(tmp_path / "models") + "/",
            "packedSimPath", str(tmp_path / "data") + "/", "lambda_t", 1.0, "lambda_t_l2", 0.0, "frame_max", 2, "frame_min", 0,
            "data_fraction", 1.0, "adv_flag", 1, "adv_mode", 1, "dataAugmentation", 0, "decayLR", 1, "adam_beta1", 0.0,
            "adam_beta2", 0.99, "learningRate", 0.0001, "lossScaling", 0, "stageIter", 1, "decayIter", 1, "maxFms", 32,
            "startFms", 32, "filterSize", 3, "upsamplingMode", 2, "upsampledData", 0, "firstNNArch", 1, "add_adj_idcs", 0,
            "addBicubicUpsample", 1, "startingIter", 0, "upsampleMode", 1, "gpu", 0, "saveInterval", 100]
    r = _driver(args, str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "TRAINING FINISHED" in out and "NEW UPRES: 8" in out
    assert "useVelInTDisc" in out and "gDrop" in out                       # the parameter listing
    strengths = re.findall(r"gdrop_strength_d: ([0-9.eE+-]+), gdrop_strength_t: ([0-9.eE+-]+)", out)
    assert len(strengths) == 7 and all(np.isfinite(float(a)) and np.isfinite(float(b)) for a, b in strengths)
    last = checkpoint.load(str(tmp_path / "models" / "test_0000" / "model_0002.ckpt"))
    assert all(np.isfinite(v).all() for v in last.values())
    assert last["tempo-disc/tBlock8/t_cA8/weight"].shape[:2] == (5, 3)
    assert last["tempo-disc/t_cfromDensity8/weight"].shape[:3] == (1, 1, 12)
    # refused without the velocity channels
    bad = list(args)
    bad[bad.index("useVelocities") + 1] = 0
    r = _driver(bad, str(tmp_path))
    assert r.returncode == 1 and "useVelInTDisc 1" in r.stdout and "useVelocities 1" in r.stdout
