"""The 4x pipeline whose second network upsamples z itself (upsamplingMode 2 with upsampleFirst 0, then upsamplingMode 0),
without a GPU: the restatement (axis_upsample_ref.py) against hand-written expectations, the two oracles of the mode-0
generator against each other, the product's pass functions on the host backend against the restatement, and the launch
plan of the mode-0 generator."""
import numpy as np
import pytest
import torch

import axis_upsample_ref as AR
from conftest import rel_l2
from oracle import nets as ON
from oracle import torch_ref


class OracleGen(object):
    """callable with the Generator interface, evaluated by the numpy oracle"""

    def __init__(self, seed, up_res, mode):
        self.ps, self.up_res, self.mode = ON.ParamSource(seed=seed), up_res, mode

    def __call__(self, x, y=None):
        return torch.as_tensor(ON.gen_resnet(self.ps, x.numpy(), self.up_res, self.mode, True)[..., 0])


def test_pass2_input_by_hand():
    """one voxel of one plane: which source voxel and which factor each of the four channels carries"""
    zl, up, vs = 4, 4, 0.5
    s = zl * up
    rng = np.random.default_rng(0)
    low = rng.random((zl, zl, zl, 4)).astype(np.float32) + 1.0
    prev = rng.random((zl, s, s)).astype(np.float32)
    xs = AR.pass2_input(prev, low, up, vs)
    assert xs.shape == (s, s, zl, 4) and xs.dtype == np.float32
    # the zoom maps output index o to source o * (n - 1) / (big - 1): the corners o = 0 and o = big - 1 are source voxels
    for (xi, yi, zi), (xl, yl) in (((0, 0, 2), (0, 0)), ((s - 1, 0, 1), (zl - 1, 0)), ((s - 1, s - 1, 3), (zl - 1, zl - 1))):
        d, vx, vy, vz = prev[zi, yi, xi], low[zi, yl, xl, 1], low[zi, yl, xl, 2], low[zi, yl, xl, 3]
        got = xs[xi, yi, zi]
        assert got[0] == d                                                  # density of the previous pass, z not zoomed
        assert got[1] == np.float32(vz * np.float32(vs))                    # vz: velocity scale, no upres factor
        assert got[2] == np.float32(vy * np.float32(vs)) * np.float32(up)   # vy: velocity scale and upres factor
        assert got[3] == vx * np.float32(up)                                # vx: upres factor, no velocity scale
    # an interior voxel is interpolated along y and x only: halfway between two source rows at the same z
    lin = np.zeros((zl, zl, zl, 4), np.float32)
    lin[..., 1] = np.arange(zl, dtype=np.float32)[None, None, :]            # vx = x index
    lin[..., 3] = np.arange(zl, dtype=np.float32)[:, None, None]            # vz = z index
    xs = AR.pass2_input(np.zeros((zl, s, s), np.float32), lin, up, 1.0)
    assert np.allclose(xs[5, 7, :, 3], 5 * (zl - 1) / (s - 1) * up)         # linear in x, the same for every z
    assert np.array_equal(xs[5, 7, :, 1], np.arange(zl, dtype=np.float32))  # z stays the low-res index
    # density only: planes of the previous pass alone
    xs1 = AR.pass2_input(prev, low[..., :1], up)
    assert xs1.shape == (s, s, zl, 1) and xs1[3, 9, 2, 0] == prev[2, 9, 3]


def test_gen_resnet_mode0_numpy_vs_torch_twin():
    for nch, rows, cols in ((1, 12, 3), (4, 8, 2)):
        ps = ON.ParamSource(seed=3)
        x = np.random.default_rng(nch).random((2, rows, cols, nch)).astype(np.float32)
        a = ON.gen_resnet(ps, x, 4, 0, True)
        b = torch_ref.gen_resnet(ps.params, x, 4, 0, True)
        assert a.shape == (2, rows, cols * 4, 1)
        assert rel_l2(b, a) < 2e-5                                          # tests/test_oracle.py, the other modes


@pytest.mark.parametrize("nch", [1, 4])
def test_pass_functions_on_the_host_backend(mpg, nch):
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    import cpu_backend
    sim, up = 4, 4
    vs = 0.5 if nch > 1 else 1.0
    low = synthetic_volume(sim, nch, 3)
    g1, g0 = OracleGen(5, up, 2), OracleGen(6, up, 0)
    want, want1 = AR.two_pass(ON.ParamSource(seed=5), ON.ParamSource(seed=6), low, up, vs)
    lt = torch.as_tensor(low)
    v1 = MP.plane_pass_4x(g1, lt, up, batch=3, backend=cpu_backend, vel_scale=vs)
    assert v1.shape == (sim, sim * up, sim * up) and np.array_equal(v1.numpy(), want1)
    out = MP.upsample_pass_4x(g0, lt, v1, up, batch=5, backend=cpu_backend, vel_scale=vs)
    assert out.shape == (sim * up,) * 3 and np.array_equal(out.numpy(), want)
    both = MP.two_pass_4x_axis(g1, g0, lt, up, batch=8, backend=cpu_backend, vel_scale=vs)
    assert np.array_equal(both[0].numpy(), want) and np.array_equal(both[1].numpy(), want1)
    # without the storage cutoff
    raw1 = MP.plane_pass_4x(g1, lt, up, backend=cpu_backend, vel_scale=vs, apply_cutoff=False)
    assert np.array_equal(raw1.numpy(), AR.pass1(ON.ParamSource(seed=5), low, up, vs, apply_cutoff=False))
    raw = MP.upsample_pass_4x(g0, lt, v1, up, backend=cpu_backend, vel_scale=vs, apply_cutoff=False)
    assert np.array_equal(raw.numpy(), AR.pass2(ON.ParamSource(seed=6), want1, low, up, vs, apply_cutoff=False))


def test_more_than_one_rank_is_refused(mpg):
    from mpgan_amd import multipass as MP
    import cpu_backend

    class TwoRanks(object):
        rank, world = 0, 2

    low = torch.zeros((4, 4, 4, 1))
    g = OracleGen(5, 4, 2)
    with pytest.raises(ValueError):
        MP.plane_pass_4x(g, low, 4, comm=TwoRanks(), backend=cpu_backend)
    with pytest.raises(ValueError):
        MP.upsample_pass_4x(g, low, torch.zeros((4, 16, 16)), 4, comm=TwoRanks(), backend=cpu_backend)
    with pytest.raises(ValueError):
        MP.two_pass_4x_axis(g, g, low, 4, comm=TwoRanks(), backend=cpu_backend)


@pytest.mark.parametrize("nch", [1, 4])
@pytest.mark.parametrize("prec", [2, 3])
def test_mode0_plan_fuses_the_column_upsample(mpg, nch, prec):
    """no standalone resize: the first residual block reads the [high, low] planes through up_log2 = 2, up_x_only = 1"""
    from mpgan_amd import multipass as MP
    g = MP.Generator("gen_resnet", dict(tile_low=8, up_res=4, channels=nch, upsampling_mode=0), None, prec)
    assert g.x.shape[1] == 32 * 8 * nch
    plan = g.sess.plan_summary(g.sampler)
    assert "resize" not in [e["kind"] for e in plan]
    fused = [e for e in plan if e["kind"] in ("conv2d_fused", "conv2d_small_pair")]
    # nothing but fused launches (and reshapes of the flat input / output): every layer is on the HIP convolutions
    assert set(e["kind"] for e in plan) <= {"conv2d_fused", "conv2d_small_pair", "reshape"}
    up = [(s["weight"], s["up_log2"], s.get("up_x_only", 0)) for e in fused for s in e["segments"] if s["up_log2"]]
    assert sorted(up) == [("generator/g_cA0/weight", 2, 1), ("generator/g_s0/weight", 2, 1)]
    # the square mode keeps its plan: both axes
    g2 = MP.Generator("gen_resnet", dict(tile_low=8, up_res=4, channels=nch, upsampling_mode=2), None, prec)
    up2 = [(s["up_log2"], s.get("up_x_only", 0)) for e in g2.sess.plan_summary(g2.sampler) if "segments" in e for s in e["segments"]
           if s["up_log2"]]
    assert up2 == [(2, 0), (2, 0)]
