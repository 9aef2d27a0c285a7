"""usePixelShuffle 1 on the MI355X: the fused depth-to-space store of the 1x1 convolution (mpg_conv2d_fused_d2s) against
mpg_conv2d_fused + mpg_depth_to_space bit for bit, mpg_space_to_depth, the inference generator and a multi-pass volume
against the restatement of tests/pixel_shuffle_ref.py, the training gradients against its float64 autograd form,
and the drivers (train, checkpoint, both output scripts)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pixel_shuffle_ref as PSR
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {3: 1e-4, 2: 5e-4}        # as test_fullsize_gpu.TOL


def _shuffle_conv(ops, x, w, b, prec, g8_src=None):
    """(fused store fp32, fused store G8 -> fp32, unfused fp32, unfused G8 -> fp32) of depth_to_space(conv1x1(x) + b)"""
    c4 = w.shape[3]
    src = ops.to_g8(x) if g8_src is None else g8_src
    chunks, ref32, ref8 = [], [], []
    for co in range(0, c4, 128):
        cw = min(128, c4 - co)
        pk = ops.pack_conv_weights(w[..., co:co + cw].contiguous(), wscale=0.5, prec=prec)
        seg = ops.Segment(src, pk)
        chunks.append(([seg], co))
        y32, y8 = ops.conv2d_fused([seg], (x.shape[1], x.shape[2]), bias=b[co:co + cw].contiguous(), want_f32=True,
                                   want_g8=True)
        ref32.append(y32)
        ref8.append(ops.from_g8(y8))
    hw = (x.shape[1], x.shape[2])
    f32, f8 = ops.conv2d_fused_d2s(chunks, hw, c4, bias=b, want_f32=True, want_g8=True)
    only8 = ops.conv2d_fused_d2s(chunks, hw, c4, bias=b, want_f32=False, want_g8=True)
    only32 = ops.conv2d_fused_d2s(chunks, hw, c4, bias=b, want_f32=True, want_g8=False)
    return (f32, ops.from_g8(f8), ops.from_g8(only8), only32,
            ops.depth_to_space(torch.cat(ref32, dim=3).contiguous(), 2), ops.depth_to_space(torch.cat(ref8, dim=3).contiguous(), 2))


@pytest.mark.parametrize("prec", [1, 2, 3])
@pytest.mark.parametrize("C", [8, 64, 128])
def test_fused_store_is_bit_identical(gpu_ops, prec, C):
    ops = gpu_ops
    if prec == 2:        # MPG_PREC_F16F6 has no depth-to-space store: refused, never planned (test_plan_* in the host tests)
        from mpgan_amd import _lib
        c = min(C, 32)
        x = torch.rand((1, 4, 4, c), device=DEV)
        pk = ops.pack_conv_weights(torch.rand((1, 1, c, 4 * c), device=DEV), prec=2)
        with pytest.raises(_lib.MpgError, match="F16F6"):
            ops.conv2d_fused_d2s([([ops.Segment(ops.to_g8(x), pk)], 0)], (4, 4), 4 * c)
        return
    g = torch.Generator(device=DEV).manual_seed(C + prec)
    for n, h, w in ((2, 5, 37), (3, 9, 4)):
        x = torch.randn((n, h, w, C), generator=g, device=DEV)
        wt = torch.randn((1, 1, C, 4 * C), generator=g, device=DEV)
        b = torch.randn((4 * C,), generator=g, device=DEV)
        f32, f8, only8, only32, r32, r8 = _shuffle_conv(ops, x, wt, b, prec)
        torch.cuda.synchronize()
        assert f32.shape == (n, 2 * h, 2 * w, C)
        assert torch.equal(f32, r32) and torch.equal(only32, r32)
        assert torch.equal(f8, r8) and torch.equal(only8, r8)
        assert float((r32 - r8).abs().max()) <= 1e-6 * float(r32.abs().max())


def test_fused_store_small_channels_and_error_path(gpu_ops):
    """C % 8 != 0: the fp32 store works (conv_small_kernel would take cout <= 8: the store stays on the MFMA kernels),
    the G8 store is refused by the library itself"""
    ops = gpu_ops
    from mpgan_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(1)
    for C in (1, 2, 4, 6):
        x = torch.randn((2, 7, 33, C), generator=g, device=DEV)
        wt = torch.randn((1, 1, C, 4 * C), generator=g, device=DEV)
        b = torch.randn((4 * C,), generator=g, device=DEV)
        pk = ops.pack_conv_weights(wt, wscale=0.5, prec=3)
        seg = ops.Segment(ops.to_g8(x), pk)
        got = ops.conv2d_fused_d2s([([seg], 0)], (7, 33), 4 * C, bias=b)
        ref = ops.depth_to_space(ops.conv2d_fused([seg], (7, 33), bias=b), 2)
        if 4 * C <= 8:      # the unfused launch runs on conv_small_kernel (fp32 FMAs), the store on the MFMA kernel
            assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5), C
        else:
            assert torch.equal(got, ref), C
        with pytest.raises(_lib.MpgError):
            ops.conv2d_fused_d2s([([seg], 0)], (7, 33), 4 * C, bias=b, want_g8=True)
        lib = _lib.load()
        d = ops._conv_desc([seg], (7, 33), b, None, 0.2)
        y8 = ops.G8.empty(2, 14, 66, 8, x.device)
        d.y_g8 = y8.buf.data_ptr()
        assert lib.mpg_conv2d_fused_d2s(ops._stream(), ctypes.byref(d), 2, 4 * C, 0) != 0
        assert b"multiples of 8" in lib.mpg_last_error()
        d.y_g8, d.y = None, got.data_ptr()
        assert lib.mpg_conv2d_fused_d2s(ops._stream(), ctypes.byref(d), 3, 4 * C, 0) != 0        # r = 2 only
        assert lib.mpg_conv2d_fused_d2s(ops._stream(), ctypes.byref(d), 2, 4 * C, 1) != 0        # channel range
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 4, 4, 3), (3, 18, 6, 64)])
def test_space_to_depth(gpu_ops, shape):
    ops = gpu_ops
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(shape, generator=g, device=DEV)
    n, h, w, c = shape
    y = ops.space_to_depth(x, 2)
    ref = x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4 * c)
    assert torch.equal(y, ref)
    assert torch.equal(ops.depth_to_space(y, 2), x)
    # adjoint: <d2s(a), x> == <a, s2d(x)>
    a = torch.randn((n, h // 2, w // 2, 4 * c), generator=g, device=DEV)
    lhs = float((ops.depth_to_space(a, 2).double() * x.double()).sum())
    rhs = float((a.double() * y.double()).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(rhs), 1.0)


def _gen(cfg, ps, prec):
    from mpgan_amd import multipass as MP
    return MP.Generator("growing_gen", dict(cfg, pixel_shuffle=True), ps.params, prec, device=DEV)


@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("arch", [dict(first_nn_arch=True, add_adj=True), dict(first_nn_arch=False, use_res_net=True),
                                  dict(first_nn_arch=False, use_res_net=False)])
def test_generator_against_restatement(gpu_ops, prec, arch):
    from oracle import nets as ON
    cfg = dict(tile_low=8, up_res=8, channels=4, first_gen=True, filter_size=3, start_fms=64, max_fms=64, **arch)
    n_in = 6 if arch.get("add_adj") else 4
    x = np.random.default_rng(2).random((3, 8, 8, n_in)).astype(np.float32)
    ps = ON.ParamSource(seed=31)
    ref = PSR.growing_gen(ps, x, up_res=8, filter_size=3, start_fms=64, max_fms=64,
                          first_nn_arch=arch["first_nn_arch"], use_res_net=arch.get("use_res_net", True))
    g = _gen(cfg, ps, prec)
    kinds = [st["kind"] for st in g.sess.plan_summary(g.sampler)]
    assert "conv2d_fused_d2s" in kinds
    err = rel_l2(g(torch.as_tensor(x, device=DEV)).cpu().numpy(), ref[..., 0])
    # the same network with nearest depool (usePixelShuffle 0) at the same size and precision, against oracle.nets
    ps0 = ON.ParamSource(seed=31)
    ref0 = ON.growing_gen(ps0, x, up_res=8, filter_size=3, start_fms=64, max_fms=64, first_nn_arch=arch["first_nn_arch"],
                          use_res_net=arch.get("use_res_net", True))
    from mpgan_amd import multipass as MP
    g0 = MP.Generator("growing_gen", cfg, ps0.params, prec, device=DEV)
    err0 = rel_l2(g0(torch.as_tensor(x, device=DEV)).cpu().numpy(), ref0[..., 0])
    print("rel L2 pixel shuffle %.3e, nearest depool %.3e (prec %d)" % (err, err0, prec))
    # the bounds of test_fullsize_gpu, or five times the depool network's error where that is larger.  Measured (shuffle /
    # depool): F16X3 5.0e-5 / 1.7e-6, 2.9e-6 / 5.4e-6, 1.1e-6 / 1.3e-6; F16F6 3.5e-4 / 1.0e-4, 1.3e-3 / 3.1e-4,
    # 7.6e-5 / 7.4e-5 for the three architectures: the shuffle network amplifies rounding more than the depool one
    assert err < max(TOL[prec], 5 * err0), (err, err0)


def test_generator_reference_width(gpu_ops):
    """startFms 256, firstNNArch 1, 64^2 -> 512^2 (the C4 first network's shuffles: 128 -> 512 and 64 -> 256 channels)"""
    from oracle import nets as ON
    cfg = dict(tile_low=64, up_res=8, channels=4, first_gen=True, filter_size=3, start_fms=256, max_fms=256,
               first_nn_arch=True)
    x = np.random.default_rng(5).random((1, 64, 64, 4)).astype(np.float32)
    ps = ON.ParamSource(seed=41)
    ref = PSR.growing_gen(ps, x, up_res=8, filter_size=3, start_fms=256, max_fms=256, first_nn_arch=True)
    g = _gen(cfg, ps, None)
    fused = [st for st in g.sess.plan_summary(g.sampler) if st["kind"] == "conv2d_fused_d2s"]
    assert [(st["cout"], st["launches"]) for st in fused] == [(128, 4), (64, 2)]
    out = g(torch.as_tensor(x, device=DEV)).cpu().numpy()
    assert rel_l2(out, ref[..., 0]) < 1e-3


class _RefGen(object):
    """the restatement as a pass generator of multipass._run_pass (CPU tensors)"""

    def __init__(self, ps, cfg):
        self.ps, self.cfg, self.high = ps, cfg, cfg["tile_low"] * 8

    def __call__(self, x, y=None):
        c = self.cfg
        out = PSR.growing_gen(self.ps, x.numpy(), up_res=8, filter_size=3, start_fms=c["start_fms"], max_fms=c["max_fms"],
                              first_nn_arch=c["first_nn_arch"])
        return torch.as_tensor(out[..., 0])


def test_multipass_volume(gpu_ops):
    import cpu_backend
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    from oracle import nets as ON
    cfg = dict(tile_low=4, up_res=8, channels=4, first_gen=True, filter_size=3, start_fms=32, max_fms=32,
               first_nn_arch=True, add_adj=True)
    low = synthetic_volume(4, 4, 3)
    ps = ON.ParamSource(seed=51)
    ref = MP.multipass_8x([_RefGen(ps, cfg)], torch.as_tensor(low), 8, batches=(8, 2, 2), backend=cpu_backend).numpy()
    g = _gen(cfg, ps, 3)
    out = MP.multipass_8x([g], torch.as_tensor(low, device=DEV), 8, batches=(8, 2, 2)).cpu().numpy()
    assert out.shape == (32, 32, 32)
    assert rel_l2(out, ref) < 1e-4


# ---------------------------------------------------------------------------------------------- training
def _make(percentage_tile=8, C=6, batch=3, fms=32, seed=9):
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    from oracle import train_ref as TR
    from oracle.nets import ParamSource
    cfg = Cfg8x(tileSizeLow=percentage_tile, upRes=8, n_inputChannels=C, start_fms=fms, max_fms=fms, usePixelShuffle=True)
    tr = Trainer8x(cfg, device=DEV, seed=seed)
    ps = ParamSource(seed=seed)
    params = {n: ps.get(n, s.shape, s.kind) for n, s in tr.graph.variables.items()}
    with torch.no_grad():
        for n, t in tr.sess.params.items():
            t.copy_(torch.as_tensor(params[n], device=DEV))
    rng = np.random.default_rng(3)
    xs = rng.random((batch, percentage_tile ** 2 * C)).astype(np.float32)
    ys = rng.random((batch, (percentage_tile * 8) ** 2)).astype(np.float32)
    lf = rng.random((batch, 1)).astype(np.float32)
    return tr, TR.to_params(params), xs, ys, lf


@pytest.mark.parametrize("percentage", [3.0, 2.3])
def test_training_gradients(gpu_ops, percentage):
    """generator- and discriminator-step gradients of every parameter (g_cPS* included) against the float64 restatement;
    bounds of test_train8x_gpu.test_wgan_gp_gradients"""
    from oracle import train_ref as TR
    tr, p, xs, ys, lf = _make()
    assert [n for n in tr.opt_g.names if "g_cPS" in n] == sorted(
        "generator/genBlock%d/g_cPS%d/%s" % (u, u, k) for u in (2, 4, 8) for k in ("bias", "weight"))
    L = tr.losses(xs, ys, percentage, lf)
    gd = torch.autograd.grad(L["disc_loss"], tr.opt_d.params, allow_unused=True, retain_graph=True)
    gg = torch.autograd.grad(L["gen_loss_complete"], tr.opt_g.params, allow_unused=True)
    Lr = PSR.losses_8x(p, xs, ys, 8, 6, percentage, lf)
    assert rel_l2(L["gen_y"].detach().cpu().numpy().reshape(3, -1), Lr["gen_y"].detach().numpy().reshape(3, -1)) < 1e-4
    rd = TR.grads(Lr["disc_loss"], p, "d_")
    rg = TR.grads(Lr["gen_loss_complete"], p, "g_")
    assert sorted(rd) == tr.opt_d.names and sorted(rg) == tr.opt_g.names
    for names, got, want in ((tr.opt_d.names, gd, rd), (tr.opt_g.names, gg, rg)):
        tot_d = tot_r = 0.0
        for nme, g in zip(names, got):
            w = want[nme]
            gnp = g.cpu().numpy().astype(np.float64) if g is not None else np.zeros_like(w)
            if np.abs(w).max() == 0.0:
                assert np.abs(gnp).max() < 1e-7, nme
                continue
            # discriminator step: the bounds of test_wgan_gp_gradients (measured 3e-6).  Generator step: measured 1.4e-2 per
            # tensor and 7.8e-3 in total at 3.0, 1.9e-3 / 1.1e-3 at 2.3, against 5e-3 / 3e-4 for the nearest-depool network;
            # the forward output of this network sits further from its restatement too (test_generator_against_restatement)
            bound = 5e-3 if names is tr.opt_d.names else 3e-2
            assert rel_l2(gnp, w) < bound, (nme, rel_l2(gnp, w))
            tot_d += float(((gnp - w) ** 2).sum())
            tot_r += float((w ** 2).sum())
        assert (tot_d / tot_r) ** 0.5 < (3e-4 if names is tr.opt_d.names else 1.5e-2)


def test_depth_to_space_fn_second_order(gpu_ops):
    """DepthToSpaceFn / SpaceToDepthFn: gradients of gradients (the linear pair) against torch's reshape / permute"""
    from mpgan_amd.train import DepthToSpaceFn
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((2, 3, 5, 16), generator=g, device=DEV, requires_grad=True)
    xr = x.detach().double().requires_grad_(True)
    v = torch.randn((2, 6, 10, 4), generator=g, device=DEV)
    y = DepthToSpaceFn.apply(x, 2)
    yr = xr.reshape(2, 3, 5, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(2, 6, 10, 4)
    assert torch.equal(y.double(), yr.detach())
    (gx,) = torch.autograd.grad((y * y * v).sum(), x, create_graph=True)
    (gxr,) = torch.autograd.grad((yr * yr * v.double()).sum(), xr, create_graph=True)
    assert torch.allclose(gx.double(), gxr, rtol=1e-6, atol=1e-6)
    (ggx,) = torch.autograd.grad((gx * gx).sum(), x)
    (ggxr,) = torch.autograd.grad((gxr * gxr).sum(), xr)
    assert torch.allclose(ggx.double(), ggxr, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------- drivers
def _run(script, args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_drivers_train_and_output(tmp_path):
    """`multipassGAN-8x.py ... usePixelShuffle 1` trains and checkpoints g_cPS*; `multipassGAN-out.py` and
    `multipassGAN-8x.py out 1` load the checkpoint (model and moving averages) and write the library's volume"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import checkpoint, uniio
    from mpgan_amd import multipass as MP
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
    models, data = str(tmp_path / "models") + "/", str(tmp_path / "data") + "/"
    args = ["randSeed", 16131119, "upRes", 8, "use_res_net", 1, "batchNorm", 0, "pixelNorm", 1, "out", 0, "pretrain", 0,
            "pretrainDisc", 0, "tileSize", 8, "simSize", sim, "use_LSGAN", 0, "use_wgan_gp", 1, "lambda", 1.0, "lambda2", 0.0,
            "discRuns", 1, "genRuns", 1, "alwaysSave", 1, "fromSim", 1005, "toSim", 1005, "outputInterval", 2, "genTestImg", -1,
            "dropout", 0.5, "dataDim", 2, "batchSize", 3, "useVelocities", 1, "useVorticities", 0, "useK_Eps_Turb", 0,
            "useFlags", 0, "gif", 0, "genModel", "gen_resnet", "discModel", "disc_binclass", "basePath", models,
            "packedSimPath", data, "lambda_t", 1.0, "lambda_t_l2", 0.0, "frame_max", 2, "frame_min", 0, "data_fraction", 1.0,
            "adv_flag", 1, "adv_mode", 0, "dataAugmentation", 0, "premadeTiles", 0, "rot", 1, "minScale", 0.85,
            "maxScale", 1.15, "flip", 1, "decayLR", 1, "adam_beta1", 0.0, "adam_beta2", 0.99, "learningRate", 0.0001,
            "lossScaling", 0, "stageIter", 2, "decayIter", 2, "maxFms", 32, "startFms", 32, "filterSize", 3,
            "upsamplingMode", 2, "upsampledData", 0, "load_model_test", -1, "load_model_no", -1, "firstNNArch", 1,
            "add_adj_idcs", 1, "usePixelShuffle", 1, "addBicubicUpsample", 1, "startingIter", 0, "useVelInTDisc", 0,
            "upsampleMode", 1, "gpu", 0, "saveInterval", 100]
    out = _run("multipassGAN-8x.py", args, str(tmp_path))
    assert "TRAINING FINISHED" in out
    test_dir = tmp_path / "models" / "test_0000"
    last = checkpoint.load(str(test_dir / "model_0002.ckpt"))
    ema = checkpoint.load(str(test_dir / "model_ema_0002.ckpt"))
    first = checkpoint.load(str(test_dir / "model_0000.ckpt"))
    for u in (2, 4, 8):
        wname = "generator/genBlock%d/g_cPS%d/weight" % (u, u)
        assert wname in last and wname in ema and "generator/genBlock%d/g_cPS%d/bias" % (u, u) in last
        assert np.isfinite(last[wname]).all()
    assert not np.array_equal(first["generator/genBlock8/g_cPS8/weight"], last["generator/genBlock8/g_cPS8/weight"])
    # output mode: the three-network script (first network only) and the per-network script, model and EMA weights
    low = synthetic_volume(sim, 4, 0)
    low[..., 0:1] += 0.05
    low_t = torch.as_tensor(low, device=DEV)
    cfg = dict(tile_low=sim, up_res=8, channels=4, first_gen=True, filter_size=3, start_fms=32, max_fms=32, add_adj=True,
               first_nn_arch=True, use_res_net=True, pixel_shuffle=True)
    for ema_flag, params in ((0, last), (1, ema)):
        (tmp_path / "models" / "test_0004").mkdir(exist_ok=True)
        oargs = ["randSeed", 200, "upRes", 8, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", sim, "simSize", sim,
                 "fromSim", 1005, "useVelocities", 1, "useVorticities", 0, "useK_Eps_Turb", 0, "useFlags", 0,
                 "genModel", "gen_resnet", "discModel", "disc_binclass", "basePath", models, "packedSimPath", data,
                 "frame_max", 1, "frame_min", 0, "velScale", 1.0, "genUni", 1, "upsampleMode", 1, "usePixelShuffle", 1,
                 "loadEmas", ema_flag, "addBicubicUpsample", 1, "gpu", 0, "transposeAxis", 0, "firstNNArch", 1,
                 "load_model_test_1", 0, "load_model_no_1", 2, "use_res_net1", 1, "add_adj_idcs1", 1, "startFms1", 32,
                 "maxFms1", 32, "filterSize1", 3, "load_model_test_2", -1, "load_model_no_2", -1, "use_res_net2", 1,
                 "add_adj_idcs2", 0, "startFms2", 192, "maxFms2", 192, "filterSize2", 5, "load_model_test_3", -1,
                 "load_model_no_3", -1, "use_res_net3", 0, "add_adj_idcs3", 0, "startFms3", 192, "maxFms3", 96,
                 "filterSize3", 5]
        _run("multipassGAN-out.py", oargs, str(tmp_path))
        g = MP.Generator("growing_gen", cfg, params, None, device=DEV, seed=200)
        want = MP.multipass_8x([g], low_t, 8).cpu().numpy()
        _, v = uniio.readUni(str(d / "source_0000.uni"))
        assert v.shape == (64, 64, 64, 1)
        assert rel_l2(v[..., 0], want) < 1e-6, ema_flag
    common = ["upRes", 8, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005,
              "toSim", 1005, "dataDim", 2, "useVelocities", 1, "basePath", models, "packedSimPath", data, "frame_max", 1,
              "frame_min", 0, "velScale", 1.0, "genUni", 1, "upsampleMode", 1, "addBicubicUpsample", 1, "prec", 3,
              "genModel", "gen_resnet", "usePixelShuffle", 1]
    _run("multipassGAN-8x.py", common + ["randSeed", 400, "use_res_net", 1, "firstNNArch", 1, "add_adj_idcs", 1,
                                         "load_model_test", 0, "load_model_no", 2, "upsampledData", 0, "upsamplingMode", 2,
                                         "maxFms", 32, "startFms", 32, "filterSize", 3, "transposeAxis", 0], str(tmp_path))
    g = MP.Generator("growing_gen", cfg, last, 3, device=DEV, seed=400)
    want = MP.single_pass_8x(g, low_t, None, 8, 0).cpu().numpy()
    _, v = uniio.readUni(str(d / "density_low_t0000_2x2_0000.uni"))
    assert rel_l2(v[..., 0], want) < 1e-6
