"""`previews 1` of the three inference drivers: the PNG files appear under the reference's names in
basePath/test_%04d/out_%04d-%04d_%04d/, decode, and agree with preview.projection_image / the restatement of the volume
computed in this process from the same input files and seeds; without the parameter no PNG is written."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import preview_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _run(script, args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _make_sim(tmp, sim, vel):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import uniio
    from mpgan_amd.synthetic import synthetic_volume
    d = tmp / "data" / "sim_1005"
    d.mkdir(parents=True)
    v = synthetic_volume(sim, 4, 0)
    uniio.writeUni(str(d / "density_low_0000.uni"), uniio.make_header(sim, sim, sim), v[..., 0:1])
    if vel:
        uniio.writeUni(str(d / "velocity_low_0000.uni"), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
    (tmp / "models").mkdir()                               # no test_%04d directory: synthWeights 1 and previews 1 create it


def _load_low(tmp, seed, vel):
    """the frame as the drivers load it"""
    from mpgan_amd import fluiddataloader as FDL
    sims = str(tmp / "data") + "/"
    fl = FDL.FluidDataLoader(print_info=0, base_path=sims, base_path_y=sims, numpy_seed=seed, filename="density_low_%04d.uni",
                             filename_index_min=0, oldNamingScheme=False, filename_y=None, filename_index_max=1, indices=[1005],
                             data_fraction=1.0, multi_file_list=["density"] + (["velocity"] if vel else []),
                             multi_file_list_y=["density"])
    x, _, _ = fl.get()
    return torch.as_tensor(np.ascontiguousarray(x[0])).to(DEV)


def _pngs(tmp):
    from mpgan_amd import heldout
    files = glob.glob(str(tmp / "models" / "**" / "*.png"), recursive=True)
    return {os.path.relpath(f, str(tmp / "models")): heldout.decode_gray_png(open(f, "rb").read()) for f in files}


def _close(img, want):
    """the same picture up to the one grey level a sum taken in another order can move a pixel next to a level's edge"""
    return img.shape == want.shape and int(np.abs(img.astype(np.int32) - want.astype(np.int32)).max()) <= 1


OUT_ARGS = ["randSeed", 200, "upRes", 8, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", 4, "simSize", 4,
            "fromSim", 1005, "useVelocities", 1, "genModel", "gen_resnet", "discModel", "disc_binclass", "frame_max", 1,
            "frame_min", 0, "velScale", 1.0, "genUni", 1, "upsampleMode", 1, "addBicubicUpsample", 1, "transposeAxis", 0,
            "firstNNArch", 1, "load_model_test_1", 0, "load_model_no_1", 299, "use_res_net1", 1, "add_adj_idcs1", 1,
            "startFms1", 256, "maxFms1", 256, "filterSize1", 3, "load_model_test_2", 4, "load_model_no_2", 585,
            "use_res_net2", 1, "add_adj_idcs2", 0, "startFms2", 192, "maxFms2", 192, "filterSize2", 5,
            "load_model_test_3", -1, "load_model_no_3", -1, "synthWeights", 1]
CFGS_OUT = [dict(first_gen=True, filter_size=3, start_fms=256, max_fms=256, add_adj=True, first_nn_arch=True, use_res_net=True),
            dict(first_gen=False, filter_size=5, start_fms=192, max_fms=192, add_adj=False, first_nn_arch=False,
                 use_res_net=True)]


def test_out_driver_previews(tmp_path):
    from mpgan_amd import multipass as MP, preview
    sim, up = 4, 8
    s = sim * up
    _make_sim(tmp_path, sim, 1)
    paths = ["basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/"]
    out = _run("multipassGAN-out.py", OUT_ARGS + paths, str(tmp_path))
    assert "pngs written" not in out and _pngs(tmp_path) == {}
    out = _run("multipassGAN-out.py", OUT_ARGS + paths + ["previews", 1], str(tmp_path))
    got = _pngs(tmp_path)
    where = "test_0004/out_0004-0585_0000/"                # the last loaded network names test_path, as in the reference
    assert all(n.startswith(where) for n in got), sorted(got)
    got = {n[len(where):]: img for n, img in got.items()}
    assert "%d pngs written to %s" % (len(got), str(tmp_path / "models") + "/" + where) in out
    low = _load_low(tmp_path, 200, 1)
    gens = [MP.Generator("growing_gen", dict(tile_low=sim, up_res=up, channels=4, pixel_norm=True, batch_norm=False,
                                             upsample_mode=1, add_bicubic=True, pixel_shuffle=False, **c), None, device=DEV,
                         seed=200 + k) for k, c in enumerate(CFGS_OUT)]
    r1 = MP.multipass_8x(gens[:1], low, up, apply_cutoff=False)           # the slice stack of pass 1
    r2 = MP.multipass_8x(gens, low, up, apply_cutoff=False)               # stack of pass 2 .permute(2,1,0) = the final dim_output
    want = R.slice_files(r2.cpu().numpy(), 0, s)
    assert sorted(got) == sorted(["source_1st_0000.png", "source_2nd_0000.png"] + list(want))
    assert got["source_1st_0000.png"].shape == (3 * s, s)
    assert _close(got["source_1st_0000.png"], preview.projection_image(r1, (2, 1, 0)).cpu().numpy())      # out.py:459
    # :521 applies (1,2,0) to the stack, which is r2.permute(2,1,0): together r2.permute(1,0,2)
    assert _close(got["source_2nd_0000.png"], preview.projection_image(r2, (1, 0, 2)).cpu().numpy())
    assert got["source_2nd_0000.png"].max() > 0
    for name, img in want.items():
        assert img.shape == (s, s) and np.array_equal(got[name], img), name


def test_4x_driver_previews(tmp_path):
    from mpgan_amd import multipass as MP, ops, preview
    sim, up = 8, 4
    s = sim * up
    _make_sim(tmp_path, sim, 0)
    args = ["upRes", up, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
            "useVelocities", 0, "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/",
            "frame_min", 0, "frame_max", 1, "genUni", 1, "velScale", 1.0, "synthWeights", 1, "genModel", "gen_resnet",
            "randSeed", 101, "load_model_test", 4, "load_model_no", 1199, "upsamplingMode", 2, "upsampledData", 0]
    out = _run("multipassGAN-4x.py", args, str(tmp_path))
    assert "pngs written" not in out and _pngs(tmp_path) == {}
    out = _run("multipassGAN-4x.py", args + ["previews", 1], str(tmp_path))
    got = _pngs(tmp_path)
    assert sorted(got) == ["test_0004/out_0004-1199_0000/source_0000.png"] and "1 pngs written" in out
    img = got["test_0004/out_0004-1199_0000/source_0000.png"]
    low = _load_low(tmp_path, 101, 0)
    gen = MP.Generator("gen_resnet", dict(tile_low=sim, up_res=up, channels=1, upsampling_mode=2, batch_norm=True), None,
                       device=DEV, seed=101)
    vol = MP._run_pass(gen, ops.axis_zoom_linear(low, 0, up), None, 0, s, 8)                  # 4x.py:1103,1126-1133
    assert img.shape == (3 * s, s) and img.max() > 0
    assert np.array_equal(img, preview.projection_image(vol).cpu().numpy())


def test_8x_driver_previews(tmp_path):
    from mpgan_amd import multipass as MP, preview
    sim, up = 4, 8
    s = sim * up
    _make_sim(tmp_path, sim, 1)
    args = ["upRes", up, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005,
            "toSim", 1005, "dataDim", 2, "useVelocities", 1, "basePath", str(tmp_path / "models") + "/",
            "packedSimPath", str(tmp_path / "data") + "/", "frame_max", 1, "frame_min", 0, "velScale", 1.0, "genUni", 1,
            "upsampleMode", 1, "addBicubicUpsample", 1, "synthWeights", 1, "genModel", "gen_resnet", "randSeed", 400,
            "use_res_net", 1, "firstNNArch", 1, "add_adj_idcs", 1, "load_model_test", 0, "load_model_no", 299,
            "upsampledData", 0, "upsamplingMode", 2, "maxFms", 256, "startFms", 256, "filterSize", 3, "transposeAxis", 1]
    out = _run("multipassGAN-8x.py", args, str(tmp_path))
    assert "pngs written" not in out and _pngs(tmp_path) == {}
    out = _run("multipassGAN-8x.py", args + ["previews", 1], str(tmp_path))
    got = _pngs(tmp_path)
    assert sorted(got) == ["test_0000/out_0000-0299_0000/source_0000.png"] and "1 pngs written" in out
    img = got["test_0000/out_0000-0299_0000/source_0000.png"]
    low = _load_low(tmp_path, 400, 1)
    gen = MP.Generator("growing_gen", dict(tile_low=sim, up_res=up, channels=4, first_gen=True, filter_size=3, start_fms=256,
                                           max_fms=256, add_adj=True, first_nn_arch=True, use_res_net=True, pixel_norm=True,
                                           batch_norm=False, upsample_mode=1, add_bicubic=True, pixel_shuffle=False), None,
                       device=DEV, seed=400)
    vol = MP.single_pass_8x(gen, low, None, up, 1, batch=2, apply_cutoff=False)           # the stack .permute(1,0,2) (:1720-1721)
    assert img.shape == (3 * s, s) and img.max() > 0
    assert _close(img, preview.projection_image(vol, (1, 0, 2)).cpu().numpy())            # :1718 looks at the stack itself
