"""The three driver scripts with ``useVorticities 1``: the output modes against oracle networks fed slice batches assembled
by hand (vorticity_ref.py: scipy zoom, adjacent slices, the numpy restatement of the stencil) within the 1e-4 that
test_drivers_gpu.py holds ``prec 3`` to; both training drivers for a few iterations on device tiles and on host tiles
with the test image on; and the refusal without velocities."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vorticity_ref as VR
from conftest import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _proc(script, args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


def _run(script, args, cwd):
    r = _proc(script, args, cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _make_sim(tmp, sim, frames, tests=()):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import uniio
    from mpgan_amd.synthetic import synthetic_volume
    d = tmp / "data" / "sim_1005"
    d.mkdir(parents=True)
    vols = []
    for f in range(frames):
        v = synthetic_volume(sim, 4, f)
        vols.append(v)
        uniio.writeUni(str(d / ("density_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim), v[..., 0:1])
        uniio.writeUni(str(d / ("velocity_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
    for t in tests:
        (tmp / "models" / ("test_%04d" % t)).mkdir(parents=True)
    return vols


def test_4x_chain_of_three_networks(tmp_path):
    from mpgan_amd import uniio
    sim, up, vs = 8, 4, 0.5
    vols = _make_sim(tmp_path, sim, 1, (4, 48))
    common = ["upRes", up, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
              "useVelocities", 1, "useVorticities", 1, "basePath", str(tmp_path / "models") + "/",
              "packedSimPath", str(tmp_path / "data") + "/", "frame_min", 0, "frame_max", 1, "genUni", 1, "velScale", vs,
              "synthWeights", 1, "genModel", "gen_resnet", "prec", 3]
    for seed, test, no, mode, upsampled in ((101, 4, 1199, 2, 0), (102, 48, 799, 1, 1), (103, 48, 800, 3, 1)):
        _run("multipassGAN-4x.py", common + ["randSeed", seed, "load_model_test", test, "load_model_no", no,
                                             "upsamplingMode", mode, "upsampledData", upsampled], str(tmp_path))
    d = tmp_path / "data" / "sim_1005"
    got = [uniio.readUni(str(d / (n % 0)))[1][..., 0] for n in ("density_low_2x2_%04d.uni", "density_low_1x1_%04d.uni",
                                                                 "density_low_0x0_%04d.uni")]
    # against the oracle chained through its own volumes, and every network on the input the run itself read (the stored
    # volume of the run before it)
    s = sim * up
    want1, chained2, chained3 = VR.chain_4x((101, 102, 103), vols[0], up, vs)
    e1 = rel_l2(got[0], want1)
    c2, c3 = rel_l2(got[1], chained2), rel_l2(got[2], chained3)
    print("4x chain with vorticity, against the oracle chained through its own volumes:", c2, c3)
    assert c2 < 1e-4 and c3 < 1e-4
    from oracle import multipass as OM
    from oracle import nets as ON
    x2 = VR.refine_pass_4x_input(vols[0], got[0], up, 1, vs)
    want2 = OM.cutoff(ON.gen_resnet(ON.ParamSource(seed=102), x2, up, 1, True).reshape(s, s, s).transpose(1, 2, 0))
    x3 = VR.refine_pass_4x_input(vols[0], got[1], up, 3, vs)
    want3 = OM.cutoff(ON.gen_resnet(ON.ParamSource(seed=103), x3, up, 3, True).reshape(s, s, s).transpose(1, 0, 2))
    e2, e3 = rel_l2(got[1], want2), rel_l2(got[2], want3)
    print("4x chain with vorticity, rel L2 of the three stored volumes:", e1, e2, e3)
    assert got[0].shape == (s, s, s) and e1 < 1e-4 and e2 < 1e-4 and e3 < 1e-4
    # and the channels matter: the same networks without them give another volume
    plain = OM.cutoff(ON.gen_resnet(ON.ParamSource(seed=101), VR.first_pass_4x_input(vols[0], up, vs)[..., :4], up, 2,
                                    True).reshape(s, s, s))
    assert rel_l2(got[0], plain) > 1e-2


def test_4x_plane_pass_and_no_mode_0(tmp_path):
    """upsampleFirst 0: the z_low slices as they are get the channels; upsamplingMode 0 has none"""
    from mpgan_amd import uniio
    from oracle import multipass as OM
    from oracle import nets as ON
    sim, up, vs = 8, 4, 0.5
    s = sim * up
    vols = _make_sim(tmp_path, sim, 1, (4, 48))
    d = tmp_path / "data" / "sim_1005"
    common = ["upRes", up, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
              "useVelocities", 1, "useVorticities", 1, "basePath", str(tmp_path / "models") + "/",
              "packedSimPath", str(tmp_path / "data") + "/", "frame_min", 0, "frame_max", 1, "genUni", 1, "velScale", vs,
              "synthWeights", 1, "genModel", "gen_resnet", "prec", 3]
    _run("multipassGAN-4x.py", common + ["randSeed", 101, "load_model_test", 4, "load_model_no", 1199, "upsamplingMode", 2,
                                         "upsampledData", 0, "upsampleFirst", 0], str(tmp_path))
    v = uniio.readUni(str(d / "density_low_2x2x1_0000.uni"))[1][..., 0]
    wantp = OM.cutoff(ON.gen_resnet(ON.ParamSource(seed=101), VR.plane_pass_4x_input(vols[0], vs), up, 2, True).reshape(sim, s, s))
    assert rel_l2(v, wantp) < 1e-4
    r = _proc("multipassGAN-4x.py", common + ["randSeed", 104, "load_model_test", 48, "load_model_no", 801, "upsamplingMode", 0,
                                              "upsampledData", 1], str(tmp_path))
    assert r.returncode == 1 and "vorticity" in r.stdout


CFGS_8X = [dict(filter_size=3, start_fms=32, max_fms=32, add_adj=True, first_nn_arch=True, use_res_net=True),
           dict(filter_size=5, start_fms=32, max_fms=32, use_res_net=True)]


def test_out_driver_with_two_networks(tmp_path):
    from mpgan_amd import uniio
    sim, up = 4, 8
    vols = _make_sim(tmp_path, sim, 1, (0, 4))
    args = ["randSeed", 300, "upRes", up, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", sim, "simSize", sim,
            "fromSim", 1005, "useVelocities", 1, "useVorticities", 1, "basePath", str(tmp_path / "models") + "/",
            "packedSimPath", str(tmp_path / "data") + "/", "frame_max", 1, "frame_min", 0, "velScale", 1.0, "genUni", 1,
            "upsampleMode", 1, "addBicubicUpsample", 1, "transposeAxis", 0, "firstNNArch", 1, "synthWeights", 1, "prec", 3,
            "load_model_test_1", 0, "load_model_no_1", 1, "load_model_test_2", 4, "load_model_no_2", 2,
            "use_res_net1", 1, "add_adj_idcs1", 1, "startFms1", 32, "maxFms1", 32, "filterSize1", 3,
            "use_res_net2", 1, "add_adj_idcs2", 0, "startFms2", 32, "maxFms2", 32, "filterSize2", 5]
    _run("multipassGAN-out.py", args, str(tmp_path))
    v = uniio.readUni(str(tmp_path / "data" / "sim_1005" / "source_0000.uni"))[1][..., 0]
    want = VR.two_networks_8x((300, 301), CFGS_8X, vols[0], up)
    e = rel_l2(v, want)
    print("out driver, two networks with vorticity, rel L2:", e)
    assert v.shape == (32, 32, 32) and e < 1e-4


def test_8x_driver_output_mode(tmp_path):
    from mpgan_amd import uniio
    sim, up = 4, 8
    vols = _make_sim(tmp_path, sim, 1, (0,))
    args = ["upRes", up, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005,
            "toSim", 1005, "dataDim", 2, "useVelocities", 1, "useVorticities", 1, "basePath", str(tmp_path / "models") + "/",
            "packedSimPath", str(tmp_path / "data") + "/", "frame_max", 1, "frame_min", 0, "velScale", 1.0, "genUni", 1,
            "upsampleMode", 1, "addBicubicUpsample", 1, "synthWeights", 1, "prec", 3, "genModel", "gen_resnet",
            "randSeed", 400, "use_res_net", 1, "firstNNArch", 1, "add_adj_idcs", 1, "load_model_test", 0, "load_model_no", 299,
            "upsampledData", 0, "upsamplingMode", 2, "maxFms", 32, "startFms", 32, "filterSize", 3, "transposeAxis", 0]
    _run("multipassGAN-8x.py", args, str(tmp_path))
    v = uniio.readUni(str(tmp_path / "data" / "sim_1005" / "density_low_t0000_2x2_0000.uni"))[1][..., 0]
    e = rel_l2(v, VR.first_network_8x(400, CFGS_8X[0], vols[0], up))
    print("8x driver out 1 with vorticity, rel L2:", e)
    assert v.shape == (32, 32, 32) and e < 1e-4


@pytest.mark.parametrize("device_tiles", [1, 0])
def test_4x_training_driver(tmp_path, device_tiles):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import checkpoint, uniio
    from mpgan_amd.synthetic import synthetic_volume
    sim, up, frames = 16, 4, 9
    d = tmp_path / "data" / "sim_1005"
    d.mkdir(parents=True)
    (tmp_path / "models").mkdir()
    for f in range(frames):
        v = synthetic_volume(sim, 4, f)
        hi = synthetic_volume(sim * up, 1, 100 + f)
        uniio.writeUni(str(d / ("density_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim), v[..., 0:1] + 0.05)
        uniio.writeUni(str(d / ("velocity_low_%04d.uni" % f)), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
        uniio.writeUni(str(d / ("density_high_%04d.uni" % f)), uniio.make_header(sim * up, sim * up, sim * up), hi + 0.05)
    args = ["upRes", up, "out", 0, "tileSize", 8, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
            "useVelocities", 1, "useVorticities", 1, "basePath", str(tmp_path / "models") + "/",
            "packedSimPath", str(tmp_path / "data") + "/", "frame_min", 0, "frame_max", 6, "genModel", "gen_resnet",
            "discModel", "disc_binclass", "randSeed", 42, "batchSize", 4, "trainingEpochs", 2, "outputInterval", 1,
            "saveInterval", 10, "lambda", 5.0, "lambda_t", 1.0, "data_fraction", 1.0, "dataAugmentation", 0,
            "upsamplingMode", 2, "upsampledData", 0, "batchNorm", 1, "genTestImg", 1, "testInterval", 1, "numTests", 2,
            "deviceTiles", device_tiles]
    out = _run("multipassGAN-4x.py", args, str(tmp_path))
    assert "TRAINING FINISHED" in out and "Epoch 00002/2" in out
    import re
    losses = [float(x) for x in re.findall(r"train_loss=([0-9.eE+-]+|nan|inf)", out)]
    assert losses and np.isfinite(losses).all(), out[-1500:]
    test_dir = tmp_path / "models" / "test_0000"
    p = checkpoint.load(str(test_dir / "model_0000.ckpt"))
    assert p["generator/g_cA0/weight"].shape[2] == 7 and p["generator/g_s0/weight"].shape[2] == 7
    assert all(np.isfinite(v).all() for v in p.values())
    assert (test_dir / "test_img" / "img_0000.png").exists()


@pytest.mark.parametrize("device_tiles,adv_mode,add_adj,channels", [(1, 0, 1, 9), (0, 1, 0, 7)])
def test_8x_training_driver(tmp_path, device_tiles, adv_mode, add_adj, channels):
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
            "simSize", sim, "use_LSGAN", 0, "use_wgan_gp", 1, "lambda", 1.0, "lambda2", 0.0, "discRuns", 1, "genRuns", 1,
            "fromSim", 1005, "toSim", 1005, "outputInterval", 1, "genTestImg", 1, "testInterval", 1, "numTests", 3,
            "dataDim", 2, "batchSize", 3, "useVelocities", 1, "useVorticities", 1, "genModel", "gen_resnet",
            "discModel", "disc_binclass", "basePath", str(tmp_path / "models") + "/",
            "packedSimPath", str(tmp_path / "data") + "/", "lambda_t", 1.0, "lambda_t_l2", 0.0, "frame_max", 2, "frame_min", 0,
            "data_fraction", 1.0, "adv_flag", 1, "adv_mode", adv_mode, "dataAugmentation", 0, "decayLR", 1, "adam_beta1", 0.0,
            "adam_beta2", 0.99, "learningRate", 0.0001, "lossScaling", 1, "stageIter", 1, "decayIter", 1, "maxFms", 32,
            "startFms", 32, "filterSize", 3, "upsamplingMode", 2, "upsampledData", 0, "firstNNArch", 1, "add_adj_idcs", add_adj,
            "addBicubicUpsample", 1, "upsampleMode", 1, "saveInterval", 100, "deviceTiles", device_tiles]
    out = _run("multipassGAN-8x.py", args, str(tmp_path))
    assert "TRAINING FINISHED" in out and "NEW UPRES: 8" in out
    import re
    losses = [float(x) for x in re.findall(r"train_loss=([0-9.eE+-]+|nan|inf)", out)]
    assert losses and np.isfinite(losses).all(), out[-1500:]
    test_dir = tmp_path / "models" / "test_0000"
    last = checkpoint.load(str(test_dir / "model_0002.ckpt"))
    assert all(np.isfinite(v).all() for v in last.values())
    # the first generator layers (firstNNArch): the convolution and the shortcut that read the tile
    assert last["generator/genBlock2/g_cA_first/weight"].shape[2] == channels
    assert last["generator/genBlock2/g_s_first/weight"].shape[2] == channels
    assert (test_dir / "test_img" / "img_0000.png").exists()


@pytest.mark.parametrize("script,extra", [("multipassGAN-4x.py", ["out", 0]), ("multipassGAN-4x.py", ["out", 1]),
                                          ("multipassGAN-8x.py", ["out", 0]), ("multipassGAN-8x.py", ["out", 1]),
                                          ("multipassGAN-out.py", [])])
def test_vorticity_without_velocities_is_refused(tmp_path, script, extra):
    r = _proc(script, ["useVorticities", 1, "useVelocities", 0, "basePath", str(tmp_path) + "/",
                       "packedSimPath", str(tmp_path) + "/"] + extra, str(tmp_path))
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "useVorticities 1" in r.stdout and "useVelocities 1" in r.stdout
