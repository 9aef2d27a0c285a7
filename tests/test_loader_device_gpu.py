"""The slice-mode kernels of the training-set loader (csrc/mpgan_loader.hip: mpg_slice_zoom_means, mpg_slice_zoom_gather)
against the float64 restatement of tests/loader_device_ref.py (proven against scipy by test_loader_device_host.py), the
DeviceFluidDataLoader against the host FluidDataLoader on the drivers' argument sets, and the drivers' deviceLoader switch.

Elementwise bound: 2^-19 * max |the 8 corner values|.  Three fp32 weights from float64 coordinates, their products and
eight multiply-adds are at most 14 roundings of 2^-24 on a convex combination, scipy's own cast of its float64 result to
fp32 is one more; the bound is twice that total."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import loader_device_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _source(shape, seed):
    return (np.random.default_rng(seed).random(shape) * 2 - 0.5).astype(np.float32)


def _gather(src, conv_axis, out3, table, out_c=None, c_off=0, adj=False):
    from mpgan_amd.fluiddataloader_device import slice_view_plan, slice_zoom_gather
    perm, cmap = slice_view_plan(conv_axis, True, src.shape[3])
    n_out = src.shape[3] + (6 if adj else 0)
    out = torch.full((len(table), out3[1], out3[2], out_c or n_out), float("nan"), dtype=torch.float32, device=DEV)
    tbl = torch.as_tensor(np.asarray(table, dtype=np.int32)).to(DEV)
    d_src = torch.as_tensor(src).to(DEV)
    slice_zoom_gather(d_src, perm, out3, tbl, cmap, out, c_off, adj)
    first = out.cpu().numpy()
    out2 = torch.full_like(out, float("nan"))
    slice_zoom_gather(d_src, perm, out3, tbl, cmap, out2, c_off, adj)
    assert np.array_equal(_bits(first), _bits(out2.cpu().numpy())), "a second launch returned other bits"
    return first


# source shape, factors, conv_axis, adj, (out_c, c_off) or None.  c % 4 == 0 with aligned windows takes the 16-byte kernel,
# everything else (3 channels, adj, a window that starts at channel 1) the one-channel kernel
GATHER_CASES = [
    ((5, 6, 7, 4), (2, 3, 1), 0, False, None),
    ((4, 4, 4, 12), (4, 4, 4), 0, False, None),
    ((4, 4, 4, 12), (4, 4, 4), 1, False, None),
    ((4, 4, 4, 12), (4, 4, 4), 2, False, None),
    ((4, 4, 4, 12), (4, 4, 4), 2, False, (13, 1)),
    ((8, 6, 7, 3), (0.25, 1, 1), 0, False, None),
    ((1, 6, 7, 4), (1, 2, 2), 0, False, None),
    ((3, 5, 5, 4), (8, 1, 1), 0, False, None),
    ((3, 5, 5, 3), (8, 1, 1), 0, True, None),
    ((3, 5, 5, 12), (8, 1, 1), 2, True, None),
]


@pytest.mark.parametrize("shape,factors,conv_axis,adj,window", GATHER_CASES)
def test_gather_against_the_restatement(gpu_ops, shape, factors, conv_axis, adj, window):
    src = _source(shape, 11)
    view = R.slice_view(src, conv_axis, True)
    out3 = [R.out_size(n, f) for n, f in zip(view.shape[:3], factors)]
    want, scale = R.zoom_ref(view, out3), R.corner_max(view, out3)
    if adj:
        want, scale = R.add_adj_ref(want), R.add_adj_ref(scale)
    # every slice, in an order that is not the array's, one of them twice
    table = list(np.random.default_rng(12).permutation(out3[0])) + [out3[0] - 1]
    out_c, c_off = window or (want.shape[3], 0)
    got = _gather(src, conv_axis, out3, table, out_c, c_off, adj)
    win = got[..., c_off:c_off + want.shape[3]]
    assert not np.isnan(win).any(), "output elements were not written"
    if window:       # and nothing outside the window was
        rest = np.delete(got, np.s_[c_off:c_off + want.shape[3]], axis=3)
        assert np.isnan(rest).all()
    err = np.abs(win.astype(np.float64) - want[table])
    bound = R.BOUND * scale[table]
    print("max err %.3e, max err / bound %.3f" % (err.max(), np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)


@pytest.mark.parametrize("conv_axis", [0, 1, 2])
@pytest.mark.parametrize("channels", [3, 12])
def test_factor_one_returns_the_sources_bits(gpu_ops, conv_axis, channels):
    src = _source((5, 6, 7, channels), 13)
    src[0, 0, 0, 0], src[1, 2, 3, 1], src[4, 5, 6, 2] = -0.0, np.inf, -np.inf      # no blend: nothing spreads, no sign is lost
    view = R.slice_view(src, conv_axis, True)
    table = [4, 0, 2] if conv_axis == 0 else [3, 1]
    got = _gather(src, conv_axis, list(view.shape[:3]), table)
    assert np.array_equal(_bits(got), _bits(view[table]))


@pytest.mark.parametrize("widths", [(1, 3), (4, 4), (1, 1, 1)])
def test_factor_one_channel_windows(gpu_ops, widths):
    """several sources written side by side into one array (the files of a multi-file y entry), bit-equal to the
    concatenated, transposed source"""
    from mpgan_amd.fluiddataloader_device import slice_zoom_gather
    parts = [_source((6, 5, 4, w), 20 + i) for i, w in enumerate(widths)]
    want = R.slice_view(np.concatenate(parts, axis=3), 2, False)
    table = [3, 0]
    out = torch.full((len(table), 5, 6, sum(widths)), float("nan"), dtype=torch.float32, device=DEV)
    tbl = torch.as_tensor(np.asarray(table, dtype=np.int32)).to(DEV)
    off = 0
    for p in parts:
        slice_zoom_gather(torch.as_tensor(p).to(DEV), [2, 1, 0], [4, 5, 6], tbl, None, out, off, False)
        off += p.shape[3]
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want[table]))


def test_gather_indexes_past_2_to_31(gpu_ops):
    """a source of more than 2^31 elements (the three 512^3 frames of an 8x entry pass 2^31 bytes): the last slice along
    the slowest-varying view axis, factor 1, against the same elements taken by indexing"""
    from mpgan_amd.fluiddataloader_device import slice_zoom_gather
    d0, d1, d2, c = 1030, 1024, 512, 4
    assert d0 * d1 * d2 * c > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(5)
    src = torch.rand((d0, d1, d2, c), dtype=torch.float32, device=DEV, generator=gen)
    table = [d2 - 1, 0]
    tbl = torch.as_tensor(np.asarray(table, dtype=np.int32)).to(DEV)
    out = torch.full((2, d1, d0, c), float("nan"), dtype=torch.float32, device=DEV)
    slice_zoom_gather(src, [2, 1, 0], [d2, d1, d0], tbl, [0, 3, 2, 1], out, 0, False)
    want = src[:, :, table, :].permute(2, 1, 0, 3)[..., [0, 3, 2, 1]]
    assert torch.equal(out, want)


MEANS_CASES = [(s, f, a) for s, f, a, adj, w in GATHER_CASES if not adj and w is None] + [
    ((5, 20, 30, 2), (4, 4, 4), 0),       # 20 slices (two blocks of the ordered sum) of 9600 pixels (three pixel blocks)
    ((5, 20, 30, 2), (4, 4, 4), 2),
]


@pytest.mark.parametrize("shape,factors,conv_axis", MEANS_CASES)
def test_means_against_the_restatement(gpu_ops, shape, factors, conv_axis):
    from mpgan_amd.fluiddataloader_device import slice_view_plan, slice_zoom_means
    src = _source(shape, 31)
    view = R.slice_view(src, conv_axis, True)
    out3 = [R.out_size(n, f) for n, f in zip(view.shape[:3], factors)]
    perm, cmap = slice_view_plan(conv_axis, True, shape[3])
    assert cmap[0] == 0                                     # the density channel is never exchanged
    want = np.array([np.average(R.zoom_ref(view[..., 0:1], out3)[s]) for s in range(out3[0])])
    scale = np.array([R.corner_max(view[..., 0:1], out3)[s].max() for s in range(out3[0])])
    d_src = torch.as_tensor(src).to(DEV)
    got = slice_zoom_means(d_src, perm, out3, 0).cpu().numpy()
    again = slice_zoom_means(d_src, perm, out3, 0).cpu().numpy()
    assert got.shape == (out3[0],) and np.array_equal(_bits(got), _bits(again))
    err = np.abs(got.astype(np.float64) - want)
    print("max err %.3e, max err / bound %.3f" % (err.max(), np.max(err / (R.BOUND * scale))))
    assert np.all(err <= R.BOUND * scale)


# ------------------------------------------------------------------------------------------------ loader level
@pytest.fixture(scope="module")
def sim_dir(tmp_path_factory):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import uniio
    return R.write_sim_dir(tmp_path_factory.mktemp("loader_sims"), uniio)


def _host_bounds(host, kw):
    """2^-19 * max |8 corners| for every element of the host loader's x and y, and the check that no filter decision of
    the host run hangs on rounding"""
    import scipy.ndimage
    rows_x, rows_y = [], []
    for e in host._entries:
        ax = host._assemble(e.x, kw["multi_file_list"], kw["multi_file_idxOff"], "arr_0")
        ay = host._assemble(e.y, kw["multi_file_list_y"], kw["multi_file_idxOff_y"], "arr_0")
        vx, vy = R.slice_view(ax, kw["conv_axis"], True), R.slice_view(ay, kw["conv_axis"], False)
        ox = [R.out_size(n, f) for n, f in zip(vx.shape[:3], kw["axis_scaling"][:3])]
        oy = [R.out_size(n, f) for n, f in zip(vy.shape[:3], kw["axis_scaling_y"][:3])]
        fx = scipy.ndimage.zoom(vx, kw["axis_scaling"], order=1)
        thr = kw["density_threshold"]
        means = [float(np.average(fx[s, :, :, 0:1])) for s in range(fx.shape[0])]
        assert all(abs(m - thr) > 1e-4 * thr for m in means)
        keep = [s for s, m in enumerate(means) if m >= thr]
        keep = keep[:int(len(keep) * kw["select_random"])]
        scale = R.corner_max(vx, ox)
        rows_x.append((R.add_adj_ref(scale) if kw.get("add_adj_idcs") else scale)[keep])
        rows_y.append(R.corner_max(vy, oy)[keep])
    return R.BOUND * np.concatenate(rows_x), R.BOUND * np.concatenate(rows_y)


@pytest.mark.parametrize("name", ["4x_first", "4x_second", "4x_second_prev", "8x_later_adj"])
def test_device_loader_matches_host_loader(gpu_ops, sim_dir, name):
    from mpgan_amd import fluiddataloader as FDL
    from mpgan_amd.fluiddataloader_device import DeviceFluidDataLoader
    kw = R.driver_argument_sets(sim_dir)[name]
    host = FDL.FluidDataLoader(**kw)
    state = np.random.get_state()
    hx, hy, hfn = host.get()
    bound, bound_y = _host_bounds(host, kw)
    dev = DeviceFluidDataLoader(device=DEV, **kw)
    after = np.random.get_state()
    assert dev.used_device_path
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    dx, dy, dfn = dev.get()
    assert dx.shape == hx.shape and dy.shape == hy.shape and dx.dtype == hx.dtype and dy.dtype == hy.dtype
    assert hx.shape[0] > 0 and dfn == hfn
    assert bound.shape == hx.shape
    err = np.abs(dx.astype(np.float64) - hx)
    print("x: max err %.3e, max err / bound %.3f" % (err.max(), np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)
    if all(float(f) == 1.0 for f in kw["axis_scaling"]):
        assert np.array_equal(_bits(dx), _bits(hx))
    if all(float(f) == 1.0 for f in kw["axis_scaling_y"]):
        assert np.array_equal(_bits(dy), _bits(hy))
    else:       # y brought down along the slice axis (the first 4x network): blends, the same bound
        assert bound_y.shape == hy.shape and np.all(np.abs(dy.astype(np.float64) - hy) <= bound_y)
    tx, ty, _ = dev.get_device()
    assert tx.is_cuda and ty.is_cuda
    assert np.array_equal(_bits(tx.cpu().numpy()), _bits(dx)) and np.array_equal(_bits(ty.cpu().numpy()), _bits(dy))


# ------------------------------------------------------------------------------------------------ drivers
def _write_driver_sims(tmp_path, sim_no, sim, up, frames, prev_name):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import uniio
    from mpgan_amd.synthetic import synthetic_volume
    d = tmp_path / "data" / ("sim_%04d" % sim_no)
    d.mkdir(parents=True)
    (tmp_path / "models").mkdir()
    hs = sim * up
    for f in range(frames):
        v = synthetic_volume(sim, 4, f)
        uniio.writeUni(str(d / ("density_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim), v[..., 0:1] + 0.05)
        uniio.writeUni(str(d / ("velocity_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
        for seed, nm in ((100, "density_high_%04d.uni"), (200, prev_name)):
            uniio.writeUni(str(d / (nm % f)), uniio.make_header(hs, hs, hs), synthetic_volume(hs, 1, seed + f) + 0.05)


def _run(script, args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("device_loader", [1, 0])
def test_4x_training_driver_device_loader(tmp_path, device_loader):
    """the second 4x network for two iterations at tile 4 / sim 8, with the device loader and, the same command, without"""
    from mpgan_amd import checkpoint
    sim, up = 8, 4
    _write_driver_sims(tmp_path, 1005, sim, up, 9, "density_low_2x2_%04d.uni")
    args = ["upRes", up, "out", 0, "tileSize", 4, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
            "useVelocities", 1, "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/",
            "frame_min", 0, "frame_max", 6, "genModel", "gen_resnet", "discModel", "disc_binclass", "randSeed", 43,
            "batchSize", 3, "trainingEpochs", 2, "outputInterval", 1, "saveInterval", 10, "lambda", 5.0, "lambda_t", 1.0,
            "data_fraction", 1.0, "dataAugmentation", 0, "upsamplingMode", 1, "upsampledData", 1, "batchNorm", 1,
            "deviceLoader", device_loader]
    out = _run("multipassGAN-4x.py", args, str(tmp_path))
    assert "TRAINING FINISHED" in out and "Epoch 00002/2" in out
    p = checkpoint.load(str(tmp_path / "models" / "test_0000" / "model_0000.ckpt"))
    assert all(np.isfinite(v).all() for v in p.values())


def test_8x_training_driver_device_loader(tmp_path):
    """the second 8x network (slices along x, add_adj_idcs off as in example_run_training.py) with deviceLoader 1"""
    from mpgan_amd import checkpoint
    sim, up = 8, 8
    _write_driver_sims(tmp_path, 1007, sim, up, 5, "density_low_t0000_2x2_%04d.uni")
    args = ["randSeed", 9631119, "upRes", 8, "use_res_net", 1, "batchNorm", 0, "pixelNorm", 1, "out", 0, "pretrain", 0,
            "pretrainDisc", 0, "tileSize", 4, "simSize", sim, "use_LSGAN", 0, "use_wgan_gp", 1, "lambda", 1.0, "lambda2", 0.0,
            "discRuns", 1, "genRuns", 1, "alwaysSave", 1, "fromSim", 1007, "toSim", 1007, "outputInterval", 3, "genTestImg", -1,
            "dropout", 0.5, "dataDim", 2, "batchSize", 3, "useVelocities", 1, "useVorticities", 0, "useK_Eps_Turb", 0,
            "useFlags", 0, "gif", 0, "genModel", "gen_resnet", "discModel", "disc_binclass",
            "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/", "lambda_t", 1.0,
            "lambda_t_l2", 0.0, "frame_max", 2, "frame_min", 0, "data_fraction", 1.0, "adv_flag", 1, "adv_mode", 0,
            "dataAugmentation", 0, "premadeTiles", 0, "decayLR", 1, "adam_beta1", 0.0, "adam_beta2", 0.99,
            "learningRate", 0.0001, "lossScaling", 1, "stageIter", 1, "decayIter", 1, "maxFms", 32, "startFms", 32,
            "filterSize", 5, "outNNTestNo", 0, "upsamplingMode", 1, "upsampledData", 1, "upsampleMode", 1,
            "usePixelShuffle", 0, "addBicubicUpsample", 1, "startingIter", 0, "useVelInTDisc", 0, "gpu", 0,
            "load_model_test", -1, "load_model_no", -1, "saveInterval", 100, "deviceLoader", 1]
    out = _run("multipassGAN-8x.py", args, str(tmp_path))
    assert "TRAINING FINISHED" in out
    last = checkpoint.load(str(tmp_path / "models" / "test_0000" / "model_0000.ckpt"))
    assert all(np.isfinite(v).all() for v in last.values())
