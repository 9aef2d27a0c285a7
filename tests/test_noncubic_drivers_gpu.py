"""The three drivers on a simulation directory of two (Z, Y, X) = (3, 5, 7) frames: the shape comes from the files, the
written headers carry it times upRes, the payloads are the library's bits, and what is out of scope on a non-cubic
volume exits with ``ERROR:`` and status 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _rank_noncubic as RN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPE = RN.SHAPE
Z, Y, X = SHAPE
FRAMES = 2
CODEC = ["uniCodec", 2, "uniIndex", 1, "deviceRead", 1]


def _run(script, args, cwd, ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _refused(script, args, cwd, *words):
    r = _run(script, args, cwd, ok=False)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ERROR: ")]
    assert len(line) == 1 and all(w in line[0] for w in words), r.stdout[-2000:]
    assert "Model restored" not in r.stdout and "synthetic weights" not in r.stdout and "OUTPUT ONLY" not in r.stdout


def _write(d, name, vol):
    from mpgan_amd import uniio
    z, y, x, c = vol.shape
    uniio.writeUni(str(d / name), uniio.make_header(x, y, z, vec3=(c == 3)), vol)


def _make_sim(tmp, shape=SHAPE, frames=FRAMES):
    import mpgan_amd  # noqa: F401
    d = tmp / "data" / "sim_1005"
    d.mkdir(parents=True)
    vols = []
    for f in range(frames):
        v = RN.volume(shape, 4, 40 + f)
        vols.append(v)
        _write(d, "density_low_%04d.uni" % f, v[..., 0:1])
        _write(d, "velocity_low_%04d.uni" % f, v[..., 1:4])
    for t in (0, 4, 9, 48):
        (tmp / "models" / ("test_%04d" % t)).mkdir(parents=True, exist_ok=True)
    return d, vols


def _paths(tmp):
    return ["basePath", str(tmp / "models") + "/", "packedSimPath", str(tmp / "data") + "/", "fromSim", 1005]


def _read(d, name, hi):
    """the payload [uZ, uY, uX] of a written volume, after the header check"""
    from mpgan_amd import uniio
    h, v = uniio.readUni(str(d / name))
    assert (h["dimZ"], h["dimY"], h["dimX"]) == hi, (name, h)
    assert v.shape == hi + (1,)
    return v[..., 0]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---------------------------------------------------------------------------- 4x: modes 2 -> 1 -> 3
def _args_4x(tmp, sim):
    return ["upRes", 4, "out", 1, "tileSize", sim, "simSize", sim, "toSim", 1005, "dataDim", 2, "useVelocities", 1,
            "frame_min", 0, "frame_max", FRAMES, "genUni", 1, "velScale", 1.0, "synthWeights", 1, "genModel", "gen_resnet"] \
        + _paths(tmp)


STEPS_4X = ((2, ["randSeed", 101, "load_model_test", 4, "load_model_no", 1199, "upsamplingMode", 2, "upsampledData", 0]),
            (1, ["randSeed", 102, "load_model_test", 48, "load_model_no", 799, "upsamplingMode", 1, "upsampledData", 1]),
            (3, ["randSeed", 103, "load_model_test", 48, "load_model_no", 800, "upsamplingMode", 3, "upsampledData", 1]))


@pytest.mark.parametrize("extra", [[], CODEC], ids=["host-files", "device-files"])
def test_4x_chain(tmp_path, mpg, extra):
    from mpgan_amd import multipass as MP
    d, vols = _make_sim(tmp_path)
    common = _args_4x(tmp_path, 5)                 # simSize is not the shape: one line says which shape is taken
    for _, step in STEPS_4X:
        out = _run("multipassGAN-4x.py", common + step + extra, str(tmp_path)).stdout
        assert out.count("simSize 5: the files hold 3 x 5 x 7 (z, y, x) volumes, which is the shape taken") == 1
    planes = MP.pass_planes_4x(SHAPE)
    g = [MP.Generator("gen_resnet", dict(tile_low=planes[i], up_res=4, channels=4, upsampling_mode=m), None, seed=101 + i)
         for i, m in enumerate((2, 1, 3))]
    hi = (4 * Z, 4 * Y, 4 * X)
    for f in range(FRAMES):
        low = _t(vols[f])
        w2, w1 = MP.two_pass_4x(g[0], g[1], low, 4)
        w3 = MP.refine_pass_4x(g[2], low, w2, 4, mode=3)
        for name, want in (("density_low_2x2_%04d.uni", w1), ("density_low_1x1_%04d.uni", w2), ("density_low_0x0_%04d.uni", w3)):
            assert _same_bits(_read(d, name % f, hi), want.cpu().numpy()), name % f


def test_4x_refusals(tmp_path, mpg):
    _make_sim(tmp_path)
    common = _args_4x(tmp_path, 7)
    cwd = str(tmp_path)
    _refused("multipassGAN-4x.py", common + STEPS_4X[0][1] + ["previews", 1], cwd, "previews 1", "cubic volumes, not 3 x 5 x 7")
    _refused("multipassGAN-4x.py", common + STEPS_4X[0][1] + ["upsampleFirst", 0], cwd, "upsampleFirst 0", "not 3 x 5 x 7")
    _refused("multipassGAN-4x.py", common + ["randSeed", 1, "load_model_test", 48, "load_model_no", 1, "upsamplingMode", 0,
                                             "upsampledData", 1], cwd, "upsamplingMode 0", "not 3 x 5 x 7")


# ---------------------------------------------------------------------------- multi-network 8x
NETS_OUT = ["firstNNArch", 1, "load_model_test_1", 0, "load_model_no_1", 299, "use_res_net1", 1, "add_adj_idcs1", 1,
            "startFms1", 32, "maxFms1", 32, "filterSize1", 3, "load_model_test_2", 4, "load_model_no_2", 585,
            "use_res_net2", 1, "add_adj_idcs2", 0, "startFms2", 32, "maxFms2", 16, "filterSize2", 5,
            "load_model_test_3", -1, "load_model_no_3", -1]
CFG_OUT = [dict(first_gen=True, filter_size=3, start_fms=32, max_fms=32, add_adj=True, first_nn_arch=True, use_res_net=True),
           dict(first_gen=False, filter_size=5, start_fms=32, max_fms=16, add_adj=False, first_nn_arch=False, use_res_net=True)]


def _args_out(tmp):
    return ["randSeed", 200, "upRes", 8, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", 4, "simSize", 4,
            "useVelocities", 1, "frame_max", FRAMES, "frame_min", 0, "velScale", 1.0, "genUni", 1, "upsampleMode", 1,
            "addBicubicUpsample", 1, "gpu", 0, "synthWeights", 1] + _paths(tmp) + NETS_OUT


@pytest.mark.parametrize("extra", [[], ["uniCodec", 2]], ids=["host-files", "device-files"])
def test_8x_out_driver_two_networks(tmp_path, mpg, extra):
    from mpgan_amd import multipass as MP
    d, vols = _make_sim(tmp_path)
    out = _run("multipassGAN-out.py", _args_out(tmp_path) + ["transposeAxis", 0] + extra, str(tmp_path)).stdout
    assert out.count("simSize 4: the files hold 3 x 5 x 7 (z, y, x) volumes, which is the shape taken") == 1
    gens = [MP.Generator("growing_gen", dict(tile_low=pl, up_res=8, channels=4, pixel_norm=True, batch_norm=False,
                                             upsample_mode=1, add_bicubic=True, **c), None, seed=200 + k)
            for k, (pl, c) in enumerate(zip(MP.pass_planes_8x(SHAPE), CFG_OUT))]
    for f in range(FRAMES):
        want = MP.multipass_8x(gens, _t(vols[f]), 8)
        assert _same_bits(_read(d, "source_%04d.uni" % f, (8 * Z, 8 * Y, 8 * X)), want.cpu().numpy()), f


def test_8x_out_driver_refusals(tmp_path, mpg):
    _make_sim(tmp_path)
    cwd = str(tmp_path)
    _refused("multipassGAN-out.py", _args_out(tmp_path) + ["transposeAxis", 0, "previews", 1], cwd, "previews 1", "not 3 x 5 x 7")
    _refused("multipassGAN-out.py", _args_out(tmp_path) + ["transposeAxis", 2], cwd, "transposeAxis 2", "not 3 x 5 x 7")


# ---------------------------------------------------------------------------- one 8x network per invocation
def _args_8x(tmp):
    return ["upRes", 8, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", 4, "simSize", 4, "toSim", 1005, "dataDim", 2,
            "useVelocities", 1, "frame_max", FRAMES, "frame_min", 0, "velScale", 1.0, "genUni", 1, "upsampleMode", 1,
            "addBicubicUpsample", 1, "synthWeights", 1, "genModel", "gen_resnet"] + _paths(tmp)


FIRST_8X = ["randSeed", 400, "use_res_net", 1, "firstNNArch", 1, "add_adj_idcs", 1, "load_model_test", 0, "load_model_no", 299,
            "upsampledData", 0, "upsamplingMode", 2, "maxFms", 32, "startFms", 32, "filterSize", 3]
SECOND_8X = ["randSeed", 401, "use_res_net", 1, "outNNTestNo", 0, "load_model_test", 9, "load_model_no", 499, "upsampledData", 1,
             "upsamplingMode", 1, "maxFms", 16, "startFms", 32, "filterSize", 5]


@pytest.mark.parametrize("extra", [[], CODEC], ids=["host-files", "device-files"])
def test_8x_chain(tmp_path, mpg, extra):
    from mpgan_amd import multipass as MP
    d, vols = _make_sim(tmp_path)
    _run("multipassGAN-8x.py", _args_8x(tmp_path) + FIRST_8X + ["transposeAxis", 0] + extra, str(tmp_path))
    _run("multipassGAN-8x.py", _args_8x(tmp_path) + SECOND_8X + ["transposeAxis", 2] + extra, str(tmp_path))
    gens = [MP.Generator("growing_gen", dict(tile_low=MP.single_pass_plane_8x(SHAPE, ta)[0], up_res=8, channels=4, upsampling_mode=m,
                                             pixel_norm=True, batch_norm=False, upsample_mode=1, add_bicubic=True,
                                             pixel_shuffle=False, vorticity=False, **c), None, seed=400 + k)
            for k, (ta, m, c) in enumerate(zip((0, 2), (2, 1), CFG_OUT))]
    hi = (8 * Z, 8 * Y, 8 * X)
    for f in range(FRAMES):
        w1 = MP.single_pass_8x(gens[0], _t(vols[f]), None, 8, 0)
        w2 = MP.single_pass_8x(gens[1], _t(vols[f]), w1, 8, 2)
        assert _same_bits(_read(d, "density_low_t0000_2x2_%04d.uni" % f, hi), w1.cpu().numpy()), f
        assert _same_bits(_read(d, "density_low_t0009_1x1_%04d.uni" % f, hi), w2.cpu().numpy()), f


def test_8x_refusals(tmp_path, mpg):
    _make_sim(tmp_path)
    cwd = str(tmp_path)
    first = _args_8x(tmp_path) + FIRST_8X + ["transposeAxis", 0]
    _refused("multipassGAN-8x.py", first + ["previews", 1], cwd, "previews 1", "not 3 x 5 x 7")
    _refused("multipassGAN-8x.py", first + ["upsampleFirst", 0], cwd, "upsampleFirst 0", "not 3 x 5 x 7")
    mode0 = [0 if k > 0 and SECOND_8X[k - 1] == "upsamplingMode" else a for k, a in enumerate(SECOND_8X)]
    _refused("multipassGAN-8x.py", _args_8x(tmp_path) + mode0 + ["transposeAxis", 0], cwd, "upsamplingMode 0", "not 3 x 5 x 7")


# ---------------------------------------------------------------------------- training takes cubes
def _training_sim(tmp, ups):
    """10 x 6 x 8 frames with their high-res targets (the slice loader keeps a tenth of the z slices)"""
    import mpgan_amd  # noqa: F401
    shape, frames = (10, 6, 8), 11
    d = tmp / "data" / "sim_1005"
    d.mkdir(parents=True)
    (tmp / "models").mkdir()
    for f in range(frames):
        v = RN.volume(shape, 4, 60 + f)
        _write(d, "density_low_%04d.uni" % f, v[..., 0:1] + np.float32(0.05))
        _write(d, "velocity_low_%04d.uni" % f, v[..., 1:4])
        for up, name in ups:
            _write(d, name % f, RN.volume(tuple(n * up for n in shape), 1, 100 * up + f) + np.float32(0.05))


def test_4x_training_takes_cubes(tmp_path, mpg):
    _training_sim(tmp_path, [(4, "density_high_%04d.uni")])
    args = ["upRes", 4, "out", 0, "tileSize", 4, "simSize", 6, "toSim", 1005, "dataDim", 2, "useVelocities", 1, "frame_min", 0,
            "frame_max", 6, "randSeed", 42, "batchSize", 4, "trainingEpochs", 1, "data_fraction", 1.0, "dataAugmentation", 0,
            "upsamplingMode", 2, "upsampledData", 0, "lambda_t", 0.0] + _paths(tmp_path)
    r = _run("multipassGAN-4x.py", args, str(tmp_path), ok=False)
    assert r.returncode == 1 and "ERROR: training takes simSize cubes" in r.stdout and "(6, 8)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "TRAINING STARTED" not in r.stdout


def test_8x_training_takes_cubes(tmp_path, mpg):
    _training_sim(tmp_path, [(2, "density_low_2_%04d.uni"), (4, "density_low_4_%04d.uni"), (8, "density_high_%04d.uni")])
    args = ["randSeed", 1, "upRes", 8, "use_res_net", 1, "batchNorm", 0, "pixelNorm", 1, "out", 0, "tileSize", 4, "simSize", 6,
            "use_wgan_gp", 1, "toSim", 1005, "dataDim", 2, "batchSize", 3, "useVelocities", 1, "lambda_t", 1.0, "frame_max", 2,
            "frame_min", 0, "data_fraction", 1.0, "dataAugmentation", 0, "stageIter", 2, "decayIter", 2, "maxFms", 32,
            "startFms", 32, "filterSize", 3, "upsamplingMode", 2, "upsampledData", 0, "firstNNArch", 1, "addBicubicUpsample", 1] \
        + _paths(tmp_path)
    r = _run("multipassGAN-8x.py", args, str(tmp_path), ok=False)
    assert r.returncode == 1 and "ERROR: training takes simSize cubes" in r.stdout and "(6, 8)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "TRAINING STARTED" not in r.stdout
