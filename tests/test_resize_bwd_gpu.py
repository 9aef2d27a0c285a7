"""The adjoints of the bilinear / bicubic resize (mpg_resize_bilinear_bwd, mpg_resize_bicubic_bwd) and what they open:
training the first 8x generator with upsampleMode 0 / 2.

* the kernels against tests/resize_bwd_ref.py (checked on the CPU by test_resize_bwd_host.py): |dx - ref| <= bound for every
  element, the bound array of resize_bwd_bound.  Every case prints "elem-error <case> <worst err / bound>"; a ratio above 1 is
  a defect of the kernel or of the bound's derivation, never a reason for a larger factor.
* exact: every element of dx written (NaN-filled buffers), the same bits twice, autograd against the direct calls.
* Trainer8x with upsampleMode 0 / 2 against the float64 restatement of tests/upsample_mode_ref.py, with the tolerances of
  test_train8x_gpu.py (test_growing_nets_forward :46-50, test_wgan_gp_gradients :71-79), and the 8x training driver."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import elem_ref as E
import resize_bwd_ref as B
import upsample_mode_ref as M
from oracle import train_ref as TR
from oracle import train_ref8x as TR8
from oracle.nets import ParamSource

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 2
# h, w -> oh, ow.  2x6 -> 82x74: the float32 coordinate below an integer (elem_ref.F32_EDGE); 7x9 -> 3x4 leaves sources that no
# output reads; 5x3 -> 5x3 the identity; 1x1 -> 4x4 every tap clamped to the one source
GEOMS = [(3, 5, 6, 10), (4, 4, 32, 32), (5, 3, 5, 3), (2, 6, 82, 74), (7, 9, 3, 4), (1, 1, 4, 4)]
# c = 12 needs more than one block of 256 threads from 3x5 on (elem_ref.NEAREST_BWD_C); 16x16 -> 32x32 at c = 33: 66 blocks
CASES = [(g, c) for g in GEOMS for c in (1, 12)] + [((16, 16, 32, 32), 33)]
METHODS = {0: "bilinear", 2: "bicubic"}


def _case_id(case):
    return "%dx%d-%dx%d-c%d" % (case[0] + (case[1],))


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _dy(case):
    (h, w, oh, ow), c = case
    return E.normal(1000 + 7 * oh + ow + c, (N, oh, ow, c))


@pytest.fixture(scope="module")
def tops(gpu_ops):
    from mpgan_amd import train_ops
    return train_ops


@pytest.fixture(scope="module")
def lib(gpu_ops):
    from mpgan_amd import _lib
    return _lib


def _bounded(name, y, ref, bound):
    assert y.shape == ref.shape == bound.shape, (name, y.shape, ref.shape, bound.shape)
    ratio = E.worst(y, ref, bound)
    print("elem-error %-58s %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: worst err / bound %.3f at %s" % (
        name, ratio, np.unravel_index(np.argmax(np.abs(y - ref) / bound), y.shape))


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_resize_bwd_bounded(tops, case, method):
    (h, w, oh, ow), c = case
    dy = _dy(case)
    dx = _np(tops.resize_bwd(_t(dy), h, w, method))
    ref = B.resize_bwd(dy, h, w, method)
    _bounded("%s bwd %s" % (METHODS[method], _case_id(case)), dx, ref, B.resize_bwd_bound(dy, h, w, method))


def test_resize_bwd_unread_sources_are_zero(tops):
    """7x9 -> 3x4 bilinear: the three output rows read source rows 0 .. 5, the four output columns source columns 0 .. 7; the
    elements nothing reads are exactly 0"""
    dy = _dy(((7, 9, 3, 4), 12))
    dx = _np(tops.resize_bwd(_t(dy), 7, 9, 0))
    idx_y, _ = B.axis_taps(3, 7, 0)
    idx_x, _ = B.axis_taps(4, 9, 0)
    rows = sorted(set(range(7)) - set(idx_y.ravel().tolist()))
    cols = sorted(set(range(9)) - set(idx_x.ravel().tolist()))
    assert rows == [6] and cols == [8]
    assert np.all(dx[:, rows] == 0.0) and np.all(dx[:, :, cols] == 0.0)
    assert np.abs(dx[:, 0, 0]).min() > 0


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_resize_bwd_writes_every_element_and_repeats_its_bits(lib, tops, case, method):
    """the C entry with dx and tmp full of NaN: no NaN is left in dx (every element is overwritten, nothing of tmp is read
    before it is written), a second call gives the same bits, and they are the bits train_ops.resize_bwd returns"""
    from mpgan_amd.ops import _ptr, _stream
    (h, w, oh, ow), c = case
    dy = _t(_dy(case))
    fn = getattr(lib.load(), "mpg_resize_%s_bwd" % METHODS[method])
    outs = []
    for _ in range(2):
        dx = torch.full((N, h, w, c), float("nan"), dtype=torch.float32, device=DEV)
        tmp = torch.full((N, h, ow, c), float("nan"), dtype=torch.float32, device=DEV)
        lib.check(fn(_stream(), _ptr(dy), N, oh, ow, c, _ptr(dx), h, w, _ptr(tmp)), "resize_bwd")
        outs.append(_np(dx))
    assert not np.isnan(outs[0]).any()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), _np(tops.resize_bwd(dy, h, w, method)).view(np.uint32))


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("case", [(g, 12) for g in GEOMS], ids=_case_id)
def test_adjoint_identity_on_the_device_forward(gpu_ops, tops, case, method):
    """<resize(x), dy> = <x, resize_bwd(dy)>, both sides from the GPU results, summed in float64.  Each side is off its exact
    value by at most its elementwise bound summed against the other factor: the forward's bilinear_bound / bicubic_bound
    against |dy|, resize_bwd_bound against |x|"""
    (h, w, oh, ow), c = case
    x = E.normal(77 + h + 3 * w, (N, h, w, c))
    dy = _dy(case)
    y = _np(gpu_ops.resize_images(_t(x), oh, ow, method)).astype(np.float64)
    dx = _np(tops.resize_bwd(_t(dy), h, w, method)).astype(np.float64)
    lhs, rhs = float((y * dy).sum()), float((x.astype(np.float64) * dx).sum())
    fwd_bound = (E.bilinear_bound if method == 0 else E.bicubic_bound)(x, oh, ow)
    slack = float((fwd_bound * np.abs(dy)).sum()) + float((B.resize_bwd_bound(dy, h, w, method) * np.abs(x)).sum())
    print("adjoint-identity %-50s %.3f" % ("%s %s" % (METHODS[method], _case_id(case)), abs(lhs - rhs) / slack))
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


# ---------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("method", sorted(METHODS))
def test_autograd_pair_is_the_direct_calls(gpu_ops, tops, method):
    from mpgan_amd.train import ResizeBwdFn, ResizeFn
    h, w, oh, ow, c = 3, 5, 6, 10, 12
    dy = _t(E.normal(5, (N, oh, ow, c)))
    x = _t(E.normal(6, (N, h, w, c))).requires_grad_(True)
    y = ResizeFn.apply(x, oh, ow, method)
    assert torch.equal(y.detach(), gpu_ops.resize_images(x.detach(), oh, ow, method))
    (dx,) = torch.autograd.grad(y, [x], dy)
    assert torch.equal(dx, tops.resize_bwd(dy, h, w, method))
    # the backward of the backward is the forward again
    g = _t(E.normal(7, (N, h, w, c)))
    dyv = dy.clone().requires_grad_(True)
    (gg,) = torch.autograd.grad(ResizeBwdFn.apply(dyv, (h, w), method), [dyv], g)
    assert torch.equal(gg, gpu_ops.resize_images(g, oh, ow, method))
    # the same through the tape of a first backward pass (what the gradient penalty does): d/d dy of <R^T dy, g> is R g
    (d1,) = torch.autograd.grad(ResizeFn.apply(x, oh, ow, method), [x], dyv, create_graph=True)
    (d2,) = torch.autograd.grad(d1, [dyv], g)
    assert torch.equal(d2, gg)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_resize_node_without_grad_makes_no_graph_node(gpu_ops, method):
    """the lowering of a `resize` node: a tensor that needs no gradient (network inputs, the critic's low-res condition) takes
    the plain forward call; one that does goes through ResizeFn"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import graph as G
    from mpgan_amd.session import VariableStore
    from mpgan_amd.train import TrainSession
    g = G.reset_default_graph()
    x = G.placeholder([None, 3, 5, 2], name="x")
    node = G.resize_images(x, [6, 10], method)
    sess = TrainSession(VariableStore(DEV, seed=1), graph=g, device=DEV)
    data = _t(E.normal(9, (N, 3, 5, 2)))
    (out,) = sess.run([node], {x: data})
    assert out.grad_fn is None and not out.requires_grad
    assert torch.equal(out, gpu_ops.resize_images(data, 6, 10, method))
    live = data.clone().requires_grad_(True)
    (out,) = sess.run([node], {x: live})
    assert out.grad_fn is not None and "ResizeFn" in type(out.grad_fn).__name__
    (dx,) = torch.autograd.grad(out, [live], torch.ones_like(out))
    assert dx.shape == live.shape


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("method", sorted(METHODS))
def test_refusals_come_before_any_launch(lib, tops, method):
    """null pointers and non-positive sizes are refused by the entry itself (MPG_REQUIRE): MpgError, nothing launched.  Every
    buffer handed over is valid and large enough, so nothing here could fault even if a check were missing"""
    from mpgan_amd.ops import _ptr, _stream
    name = "mpg_resize_%s_bwd" % METHODS[method]
    fn = getattr(lib.load(), name)
    dy = _t(E.normal(1, (N, 6, 10, 3)))
    dx = torch.zeros((N, 6, 10, 3), dtype=torch.float32, device=DEV)
    tmp = torch.zeros((N, 6, 10, 3), dtype=torch.float32, device=DEV)
    good = (N, 6, 10, 3, 3, 5)
    lib.check(fn(_stream(), _ptr(dy), good[0], good[1], good[2], good[3], _ptr(dx), good[4], good[5], _ptr(tmp)), name)
    for missing in range(3):
        ptrs = [_ptr(dy), _ptr(dx), _ptr(tmp)]
        ptrs[missing] = _ptr(None)
        with pytest.raises(lib.MpgError, match="null pointer"):
            lib.check(fn(_stream(), ptrs[0], N, 6, 10, 3, ptrs[1], 3, 5, ptrs[2]), name)
    for pos in range(6):
        for bad in (0, -1):
            a = list(good)
            a[pos] = bad
            with pytest.raises(lib.MpgError, match="bad shape"):
                lib.check(fn(_stream(), _ptr(dy), a[0], a[1], a[2], a[3], _ptr(dx), a[4], a[5], _ptr(tmp)), name)
    for h, w in ((0, 5), (3, 0), (-1, 5), (3, -2)):
        with pytest.raises(lib.MpgError):
            tops.resize_bwd(dy, h, w, method)
    with pytest.raises(lib.MpgError):
        tops.resize_bwd(dy, 3, 5, 3)
    with pytest.raises(lib.MpgError):
        tops.resize_bwd(dy.cpu(), 3, 5, method)


# ---------------------------------------------------------------------------------------------- Trainer8x, upsampleMode 0 / 2
def make(mode, data_seed=3, tile=M.TILE, C=M.CHANNELS, fms=32, seed=9):
    """the make() of test_train8x_gpu.py with the option; the data of upsample_mode_ref.parity_data"""
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(tileSizeLow=tile, upRes=8, n_inputChannels=C, start_fms=fms, max_fms=fms, upsampleMode=mode)
    tr = Trainer8x(cfg, device=DEV, seed=seed)
    ps = ParamSource(seed=seed)
    params = {n: ps.get(n, s.shape, s.kind) for n, s in tr.graph.variables.items()}
    with torch.no_grad():
        for n, t in tr.sess.params.items():
            t.copy_(torch.as_tensor(params[n], device=DEV))
    xs, ys, lf = M.parity_data(data_seed)
    return tr, TR.to_params(params), xs, ys, lf


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


SCALARS = ("d_loss_y", "d_loss_g", "l1_loss", "g_loss_d", "disc_loss_layer", "epsilon_penalty_d", "grad_penalty_d", "disc_loss",
           "gen_loss_complete")


@pytest.fixture(scope="module")
def nearest_losses(gpu_ops):
    """the mode 1 losses of the same parameters and data, once per (percentage, data seed)"""
    out = {}
    for percentage, seed in sorted(set((q, sd) for _, q, sd in M.PARITY_CASES)):
        tr, p, xs, ys, lf = make(1, seed)
        L = tr.losses(xs, ys, percentage, lf)
        out[percentage, seed] = {k: float(L[k].detach()) for k in SCALARS}
    return out


@pytest.mark.parametrize("mode,percentage,data_seed", M.PARITY_CASES, ids=lambda v: str(v))
def test_trainer8x_parity_with_upsample_mode(monkeypatch, nearest_losses, mode, percentage, data_seed):
    """losses, gen_y and the gradient of every parameter of the discriminator step (gradient penalty included) and of the
    generator step against float64 autograd; tolerances copied from test_train8x_gpu.py: 1e-4 on gen_y and
    2e-4 max(|b|, 1e-2) on the scalars (test_growing_nets_forward), 5e-3 per tensor and 3e-4 overall on the gradients
    (test_wgan_gp_gradients).  The data seed of each case: upsample_mode_ref.PARITY_CASES"""
    monkeypatch.setattr(TR8, "growing_gen", M.growing_gen_for(mode))
    monkeypatch.setattr(TR8, "growing_disc", M.growing_disc_for(mode))
    tr, p, xs, ys, lf = make(mode, data_seed)
    L = tr.losses(xs, ys, percentage, lf)
    gd = torch.autograd.grad(L["disc_loss"], tr.opt_d.params, allow_unused=True, retain_graph=True)
    gg = torch.autograd.grad(L["gen_loss_complete"], tr.opt_g.params, allow_unused=True)
    Lr = TR8.losses_8x(p, xs, ys, M.TILE, M.CHANNELS, percentage, lf)
    r_gen = rel(L["gen_y"].detach().cpu().numpy().reshape(M.BATCH, -1), Lr["gen_y"].detach().numpy().reshape(M.BATCH, -1))
    print("upsampleMode %d percentage %.1f gen_y %.3e" % (mode, percentage, r_gen))
    assert r_gen < 1e-4
    for k in SCALARS:
        a, b = float(L[k].detach()), float(Lr[k].detach())
        assert abs(a - b) <= 2e-4 * max(abs(b), 1e-2), (k, a, b)
    # the option is live: the generator's output and the critic's condition both change, so the losses do
    near = nearest_losses[percentage, data_seed]
    for k in ("l1_loss", "d_loss_y", "d_loss_g", "gen_loss_complete"):
        assert abs(float(L[k].detach()) - near[k]) > 1e-5 * max(abs(near[k]), 1e-2), (k, float(L[k].detach()), near[k])
    rd = TR.grads(Lr["disc_loss"], p, "d_")
    rg = TR.grads(Lr["gen_loss_complete"], p, "g_")
    assert sorted(rd) == tr.opt_d.names and sorted(rg) == tr.opt_g.names
    worst = 0.0
    for names, got, want in ((tr.opt_d.names, gd, rd), (tr.opt_g.names, gg, rg)):
        tot_d = tot_r = 0.0
        for nme, g in zip(names, got):
            w = want[nme]
            gnp = g.cpu().numpy().astype(np.float64) if g is not None else np.zeros_like(w)
            if np.abs(w).max() == 0.0:
                assert np.abs(gnp).max() < 1e-7, nme       # heads faded out completely (t = 1)
                continue
            r = rel(gnp, w)
            worst = max(worst, r)
            assert r < 5e-3, (nme, r)      # d_l61/bias: +1/B and -1/B cancel, the 1e-3 epsilon penalty is left
            tot_d += float(((gnp - w) ** 2).sum())
            tot_r += float((w ** 2).sum())
        print("upsampleMode %d percentage %.1f %s aggregate gradient error %.3e" % (
            mode, percentage, names[0].split("/")[0], math.sqrt(tot_d / tot_r)))
        assert math.sqrt(tot_d / tot_r) < 3e-4
    print("upsampleMode %d percentage %.1f worst per-tensor gradient error %.3e" % (mode, percentage, worst))


def test_train_steps_with_bicubic_upsampling():
    """the shape of test_train8x_gpu.test_train_step_runs_and_moves_both_networks at upsampleMode 2, eight steps"""
    tr, p, xs, ys, lf = make(2)
    before = {n: t.detach().clone() for n, t in tr.sess.params.items()}
    for _ in range(8):
        d, g = tr.train_step(xs, ys, 3.0)
        assert np.isfinite(float(d)) and np.isfinite(float(g))
    moved_d = sum(int(not torch.equal(tr.sess.params[n].detach(), before[n])) for n in tr.opt_d.names)
    moved_g = sum(int(not torch.equal(tr.sess.params[n].detach(), before[n])) for n in tr.opt_g.names)
    assert moved_d >= len(tr.opt_d.names) - 6      # the faded-out d_cfromDensity{4,2,1} convs keep zero gradients
    assert moved_g >= len(tr.opt_g.names) - 6      # the three faded-out density heads keep zero gradients
    assert all(torch.isfinite(t).all() for t in tr.sess.params.values())
    l1 = [float(tr.gen_step(xs, ys, 3.0)["l1_loss"].detach()) for _ in range(8)]
    assert l1[-1] < l1[0]


# ---------------------------------------------------------------------------------------------- the driver
def _run(script, args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_8x_training_driver_with_bicubic_upsampling(tmp_path):
    """the 8x training run of test_drivers_gpu.test_8x_training_driver (adv_mode 0) with `upsampleMode 2`: it trains through
    the three growing stages and writes checkpoints, and `out 1` with `upsampleMode 2` loads the last one and writes a volume"""
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
    args = ["randSeed", 16131119, "upRes", 8, "use_res_net", 1, "batchNorm", 0, "pixelNorm", 1, "out", 0, "pretrain", 0,
            "pretrainDisc", 0, "tileSize", 8, "simSize", sim, "use_LSGAN", 0, "use_wgan_gp", 1, "lambda", 1.0, "lambda2", 0.0,
            "discRuns", 1, "genRuns", 1, "alwaysSave", 1, "fromSim", 1005, "toSim", 1005, "outputInterval", 2, "genTestImg", -1,
            "dropout", 0.5, "dataDim", 2, "batchSize", 3, "useVelocities", 1, "useVorticities", 0, "useK_Eps_Turb", 0,
            "useFlags", 0, "gif", 0, "genModel", "gen_resnet", "discModel", "disc_binclass",
            "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/", "lambda_t", 1.0,
            "lambda_t_l2", 0.0, "frame_max", 2, "frame_min", 0, "data_fraction", 1.0, "adv_flag", 1, "adv_mode", 0,
            "dataAugmentation", 0, "premadeTiles", 0, "rot", 1, "minScale", 0.85, "maxScale", 1.15, "flip", 1, "decayLR", 1,
            "adam_beta1", 0.0, "adam_beta2", 0.99, "learningRate", 0.0001, "lossScaling", 1, "stageIter", 2, "decayIter", 2,
            "maxFms", 32, "startFms", 32, "filterSize", 3, "upsamplingMode", 2, "upsampledData", 0, "load_model_test", -1,
            "load_model_no", -1, "firstNNArch", 1, "add_adj_idcs", 1, "usePixelShuffle", 0, "addBicubicUpsample", 1,
            "startingIter", 0, "useVelInTDisc", 0, "upsampleMode", 2, "gpu", 0, "saveInterval", 100]
    out = _run("multipassGAN-8x.py", args, str(tmp_path))
    assert "TRAINING FINISHED" in out and "NEW UPRES: 4" in out and "NEW UPRES: 8" in out
    test_dir = tmp_path / "models" / "test_0000"
    first = checkpoint.load(str(test_dir / "model_0000.ckpt"))
    last = checkpoint.load(str(test_dir / "model_0002.ckpt"))
    wname = "generator/genBlock8/g_cA_first/weight"
    assert wname in last and all(np.isfinite(v).all() for v in last.values())
    assert not np.array_equal(first[wname], last[wname])
    (tmp_path / "models" / "test_0004").mkdir()
    oargs = ["randSeed", 200, "upRes", 8, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", sim, "simSize", sim,
             "fromSim", 1005, "useVelocities", 1, "useVorticities", 0, "useK_Eps_Turb", 0, "useFlags", 0,
             "genModel", "gen_resnet", "discModel", "disc_binclass", "basePath", str(tmp_path / "models") + "/",
             "packedSimPath", str(tmp_path / "data") + "/", "frame_max", 1, "frame_min", 0, "velScale", 1.0, "genUni", 1,
             "upsampleMode", 2, "usePixelShuffle", 0, "loadEmas", 0, "addBicubicUpsample", 1, "gpu", 0, "transposeAxis", 0,
             "firstNNArch", 1, "load_model_test_1", 0, "load_model_no_1", 2, "use_res_net1", 1, "add_adj_idcs1", 1,
             "startFms1", 32, "maxFms1", 32, "filterSize1", 3, "load_model_test_2", -1, "load_model_no_2", -1,
             "use_res_net2", 1, "add_adj_idcs2", 0, "startFms2", 192, "maxFms2", 192, "filterSize2", 5,
             "load_model_test_3", -1, "load_model_no_3", -1, "use_res_net3", 0, "add_adj_idcs3", 0, "startFms3", 192,
             "maxFms3", 96, "filterSize3", 5]
    out = _run("multipassGAN-out.py", oargs, str(tmp_path))
    assert "stored .uni file" in out
    h, v = uniio.readUni(str(d / "source_0000.uni"))
    assert v.shape == (64, 64, 64, 1) and np.isfinite(v).all()
