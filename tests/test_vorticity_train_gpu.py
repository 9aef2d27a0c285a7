"""Training with the three vorticity input channels (useVorticities): Trainer4x and Trainer8x at 7 input channels against
the float64 restatements (oracle/train_ref.py, oracle/train_ref8x.py) at the bounds of the 4-channel parity tests
(test_train_gpu.py::test_gan4x_losses_and_gradients, test_train8x_gpu.py::test_growing_nets_forward and
::test_temporal_critic_losses_and_gradients), and the temporal step with adv_mode 1, whose advection must read the
velocity as channels 1..3 of the 7-channel tile."""
import contextlib
import io
import math
import random

import numpy as np
import pytest
import torch

import vorticity_ref as VR
import vorticity_train_cases as VC
from oracle import train_ref as TR
from oracle import train_ref8x as TR8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BN_BIASES = {"generator/g_c%s%d/bias" % (k, i) for k in "AB" for i in range(3)} | \
    {"generator/g_s%d/bias" % i for i in range(3)} | {"discriminator/d_c%d/bias" % i for i in (2, 3, 4)}


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _load(tr, params):
    with torch.no_grad():
        for name, t in tr.sess.params.items():
            t.copy_(torch.as_tensor(params[name], device=DEV))


def test_gan4x_losses_and_gradients_at_7_channels():
    """the case of vorticity_train_cases.py: test_vorticity_host.py shows that no pre-activation of its float64 oracle
    lies within 1e-5 of zero, so no ReLU mask can differ between the two sides"""
    from mpgan_amd.train import Trainer4x
    tile, batch, C = VC.TILE, VC.BATCH, VC.CHANNELS
    tr = Trainer4x(tileSizeLow=tile, upRes=4, n_inputChannels=C, batch_norm=True, device=DEV, seed=VC.SEED, prec=3)
    assert tuple(tr.graph.variables["generator/g_cA0/weight"].shape)[2] == 7
    params, p = VC.oracle_params(tr.graph.variables)
    _load(tr, params)
    xs, ys = VC.tiles_4x()
    L = tr.losses(xs, ys)
    Lr = TR.losses_4x(p, xs, ys, tile, 4, C, batch_norm=True)
    for k in ("disc_loss", "gen_loss", "gen_l1_loss", "gen_l2_loss", "disc_loss_layer", "gen_loss_complete"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        print(k, a, b)
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), (k, a, b)
    assert rel(L["gen_part"].detach().cpu().numpy().reshape(batch, -1), Lr["gen_part"].detach().numpy().reshape(batch, -1)) < 1e-4
    rd = TR.grads(Lr["disc_loss"], p, "d_")
    rg = TR.grads(Lr["gen_loss_complete"], p, "g_")
    assert sorted(rd) == tr.opt_d.names and sorted(rg) == tr.opt_g.names
    gd = torch.autograd.grad(L["disc_loss"], tr.opt_d.params, allow_unused=True, retain_graph=True)
    gg = torch.autograd.grad(L["gen_loss_complete"], tr.opt_g.params, allow_unused=True)
    worst, total, off = 0.0, 0.0, []
    for names, got, want in ((tr.opt_d.names, gd, rd), (tr.opt_g.names, gg, rg)):
        tot_d = tot_r = 0.0
        for nme, g in zip(names, got):
            w = want[nme]
            gnp = g.cpu().numpy().astype(np.float64) if g is not None else np.zeros_like(w)
            if nme in BN_BIASES:
                assert np.abs(gnp).max() < 1e-4        # bias under batch norm: the exact gradient is 0
                continue
            r = rel(gnp, w)
            worst = max(worst, r)
            if r >= 1e-4:
                off.append((nme, float("%.3g" % r)))
            tot_d += float(((gnp - w) ** 2).sum())
            tot_r += float((w ** 2).sum())
        total = max(total, math.sqrt(tot_d / tot_r))
    print("worst per-tensor gradient error", worst, "whole", total)
    assert total < 2e-4, off
    assert worst < 1e-3, off
    # the first layer's gradient reaches the three new input channels' weights
    g0 = gg[tr.opt_g.names.index("generator/g_cA0/weight")]
    assert float(g0[:, :, 6, :].abs().max()) > 0


def _trainer8x(tile, C, seed=9, fms=32, **kw):
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(tileSizeLow=tile, upRes=8, n_inputChannels=C, start_fms=fms, max_fms=fms)
    tr = Trainer8x(cfg, device=DEV, seed=seed, **kw)
    params, p = VC.oracle_params(tr.graph.variables, seed)
    _load(tr, params)
    return tr, p


def test_trainer8x_losses_at_7_channels():
    tile, C, batch = 8, 7, 3
    tr, p = _trainer8x(tile, C)
    rng = np.random.default_rng(3)
    xs = VR.append(rng.random((batch, 1, tile, tile, 4)).astype(np.float32)).reshape(batch, -1)
    ys = rng.random((batch, (tile * 8) ** 2)).astype(np.float32)
    lf = rng.random((batch, 1)).astype(np.float32)
    L = tr.losses(xs, ys, 3.0, lf)
    Lr = TR8.losses_8x(p, xs, ys, tile, C, 3.0, lf)
    assert rel(L["gen_y"].detach().cpu().numpy().reshape(batch, -1), Lr["gen_y"].detach().numpy().reshape(batch, -1)) < 1e-4
    for k in ("d_loss_y", "d_loss_g", "l1_loss", "g_loss_d", "disc_loss_layer", "epsilon_penalty_d", "grad_penalty_d",
              "disc_loss", "gen_loss_complete"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        print(k, a, b)
        assert abs(a - b) <= 2e-4 * max(abs(b), 1e-2), (k, a, b)
    d, g = tr.train_step(xs, ys, 3.0)
    assert np.isfinite(float(d)) and np.isfinite(float(g))


def test_temporal_step_with_advection_at_7_channels():
    """adv_mode 1 (GAN.advect inside the step): the 7-channel tiles are viewed with their own channel count and the
    velocity is channels 1..3 -- the same velocity the 4-channel view of the tiles holds, which is what the oracle
    advects with"""
    from mpgan_amd import tilecreator_t as tc
    tile, C = 8, 7
    rng = np.random.default_rng(41)
    with contextlib.redirect_stdout(io.StringIO()):
        tiCr = tc.TileCreator(tileSizeLow=tile, simSizeLow=16, upres=8, dim=2, dim_t=3, densityMinimum=0.0,
                              channelLayout_low="d,vx,vy,vz", channelLayout_high="d")
        tiCr.addData(rng.random((4, 1, 16, 16, 12)).astype(np.float32), rng.random((4, 1, 128, 128, 3)).astype(np.float32))
    random.seed(2)
    xts4, yts, ypos = tiCr.selectRandomTempoTiles(6, True, False, n_t=3, dt=0.5)
    xts4 = np.ascontiguousarray(xts4, np.float32)
    xts = VR.append(xts4.reshape(-1, 1, tile, tile, 4)).reshape(xts4.shape[0], -1)
    assert np.array_equal(xts.reshape(-1, tile, tile, C)[..., :4].reshape(xts4.shape), xts4)
    tr, p = _trainer8x(tile, C, use_tempo=True, adv_mode=1)
    lf_t = rng.random((2, 1)).astype(np.float32)
    L = tr.tempo_losses(xts, yts, ypos, 3.0, lf_t)
    Lr = TR8.tempo_losses_8x(p, xts, yts, ypos, tile, C, 3.0, lf_t, adv_mode=1)
    for k in ("t_disc_loss", "g_loss_t"):
        a, b = float(L[k].detach()), float(Lr[k].detach())
        print(k, a, b)
        assert abs(a - b) <= 2e-4 * max(abs(b), 1e-2), (k, a, b)
    xs = xts[:2]
    ys = np.ascontiguousarray(yts[:2])
    d, g = tr.train_step(xs, ys, 3.0, tempo=(xts, yts, ypos))
    assert np.isfinite(float(d)) and np.isfinite(float(g))
