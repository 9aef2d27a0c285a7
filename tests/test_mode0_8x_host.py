"""The 8x pipeline whose second network upsamples z itself (upsamplingMode 2 with upsampleFirst 0, then upsamplingMode 0),
without a GPU: the network table and graph, the refusals, the restatement (upsample_mode0_8x_ref.py) against the oracle's
general bicubic resize and against hand-assembled volumes, the product's pass functions on the host backend against the
restatement, and the launch plan."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import upsample_mode0_8x_ref as MR
from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NARROW = dict(filter_size=3, start_fms=32, max_fms=16)


def _gen(MP, low=4, **kw):
    cfg = dict(tile_low=low, up_res=8, channels=4, upsampling_mode=0, use_res_net=True, **NARROW)
    cfg.update(kw)
    return MP.Generator("growing_gen", cfg, None, prec=2)


def _nodes(fetch):
    seen, stack, out = set(), [fetch], []
    while stack:
        n = stack.pop()
        if n.id not in seen:
            seen.add(n.id)
            out.append(n)
            stack.extend(n.inputs)
    return out


# ---- network ---------------------------------------------------------------------------------------------------------
def test_cfg8x_mode0_constructs(mpg):
    from mpgan_amd.arch import Cfg8x
    c = Cfg8x(tileSizeLow=4, upRes=8, n_inputChannels=4, upsampling_mode=0)
    assert c.tileSizeHigh == 32 and c.n_input == 32 * 4 * 5 and c.n_output == 32 * 32
    assert c.axis_gen and not c.first_gen
    # the other modes keep their input size
    assert Cfg8x(tileSizeLow=4, upRes=8, n_inputChannels=4, upsampling_mode=1).n_input == 4 * 4 * 4


def test_fewer_than_five_channels_are_refused(mpg):
    from mpgan_amd.arch import Cfg8x
    for nch in (1, 3):
        with pytest.raises(ValueError, match="channel 4"):
            Cfg8x(tileSizeLow=4, upRes=8, n_inputChannels=nch, upsampling_mode=0, addBicubicUpsample=True)
    # without the residual nothing reads channel 4
    assert Cfg8x(tileSizeLow=4, upRes=8, n_inputChannels=1, upsampling_mode=0, addBicubicUpsample=False).n_input == 32 * 4 * 2


def test_training_form_is_refused(mpg):
    from mpgan_amd import arch, graph as G
    from mpgan_amd.train import Trainer8x
    cfg = arch.Cfg8x(tileSizeLow=4, upRes=8, n_inputChannels=4, upsampling_mode=0, first_nn_arch=False, start_fms=32, max_fms=16)
    prev = G.get_default_graph()
    G.reset_default_graph()
    try:
        x = G.placeholder([None, cfg.n_input])
        with pytest.raises(NotImplementedError, match="training upsampling_mode 0"):
            arch.growing_gen(x, cfg, G.scalar_placeholder("percentage"), train=True)
    finally:
        G._default_graph[0] = prev
    with pytest.raises(NotImplementedError, match="training upsampling_mode 0"):
        Trainer8x(cfg, device="cpu")


@pytest.mark.parametrize("use_res_net", [True, False])
def test_graph_one_column_depool_per_block_and_residual_from_channel_4(mpg, use_res_net):
    from mpgan_amd import multipass as MP
    low, high = 4, 32
    g = _gen(MP, low, use_res_net=use_res_net)
    assert g.x.shape[1] == high * low * 5 and g.y is None
    nodes = _nodes(g.sampler)
    depools = sorted((n for n in nodes if n.op == "resize" and n.attrs["method"] == 1), key=lambda n: n.id)
    assert [(n.inputs[0].shape[1:3], n.shape[1:3]) for n in depools] == [
        ((high, low), (high, 2 * low)), ((high, 2 * low), (high, 4 * low)), ((high, 4 * low), (high, 8 * low))]
    # each one feeds the first unit of its block: convA and, in a residual unit, the 1x1 shortcut
    from mpgan_amd import graph as G
    cons = G.consumers([g.sampler])
    for n, up in zip(depools, (2, 4, 8)):
        readers = cons[n.id]
        assert all(r.op == "conv2d" for r in readers) and len(readers) == (2 if use_res_net else 1)
        names = sorted(r.inputs[1].attrs["var"] for r in readers)
        tag = ("g_cA_first", "g_s_first") if use_res_net else ("g_cA%d" % up,)
        assert names == ["generator/genBlock%d/%s/weight" % (up, t) for t in tag]
    bic = [n for n in nodes if n.op == "resize" and n.attrs["method"] == 2]
    assert len(bic) == 1 and bic[0].shape[1:] == (high, high, 1)
    sl = bic[0].inputs[0]
    assert sl.op == "slice" and (sl.attrs["begin"], sl.attrs["size"]) == (4, 1) and sl.inputs[0].shape[1:] == (high, low, 5)
    assert g.sampler.shape[1] == high * high


# ---- restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 4, 8])
@pytest.mark.parametrize("wl", [3, 8])
def test_column_bicubic_is_the_general_resize_at_row_scale_1(wl, f):
    rng = np.random.default_rng(wl * 10 + f)
    x = rng.standard_normal((2, 5, wl, 1)).astype(F32)
    want = O.resize_bicubic_tf1(x, 5, wl * f)
    got = MR.bicubic_cols(x[..., 0], f)
    assert got.dtype == np.float64 and np.array_equal(got.astype(F32), want[..., 0])
    src = rng.standard_normal((2, 5, wl, 5)).astype(F32)
    dens = rng.standard_normal((2, 5, wl * f, 1)).astype(F32)
    both = MR.bicubic_cols_add(src, 4, f, dens)
    assert np.array_equal(both, dens.astype(np.float64) + MR.bicubic_cols(src[..., 4], f)[..., None])
    # the row weights of the general resize at scale 1 are exactly (0, 1, 0, 0)
    _, wy = O.bicubic_taps_tf1(5, 5)
    assert np.array_equal(wy, np.tile(np.array([0, 1, 0, 0], F32), (5, 1)))


def _distinct_volume(n=4):
    """[n, n, n, 4] of distinct integers: 1000 z + 100 y + 10 x + channel"""
    z, y, x, c = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), np.arange(4), indexing="ij")
    return (1000 * z + 100 * y + 10 * x + c + 1).astype(F32)


def test_pass2_input_by_hand():
    zl, up = 4, 2
    s = zl * up
    low = _distinct_volume(zl)
    prev = (np.arange(zl * s * s, dtype=F32) + 0.5).reshape(zl, s, s)
    xs = MR.pass2_input(prev, low, up)
    assert xs.shape == (s, s, zl, 5) and xs.dtype == F32
    # the linear zoom maps output o to source o (n - 1) / (N - 1); written out voxel by voxel
    want = np.zeros((s, s, zl, 5))
    for xi in range(s):
        for yi in range(s):
            sx, sy = xi * (zl - 1) / (s - 1), yi * (zl - 1) / (s - 1)
            x0, y0 = min(int(sx), zl - 1), min(int(sy), zl - 1)
            x1, y1 = min(x0 + 1, zl - 1), min(y0 + 1, zl - 1)
            tx, ty = sx - x0, sy - y0
            for zi in range(zl):
                p = low[zi].astype(np.float64)
                v = ((1 - ty) * ((1 - tx) * p[y0, x0] + tx * p[y0, x1]) + ty * ((1 - tx) * p[y1, x0] + tx * p[y1, x1]))
                d, vx, vy, vz = v
                want[xi, yi, zi] = (prev[zi, yi, xi], vy, vx * up, d * up, vz)
    assert np.allclose(xs, want, rtol=1e-6, atol=0)
    # the corners are source voxels, exactly: plane index = x, row = y, column = z_low; (prev, vy, vx * up, d * up, vz)
    for (xi, yi, zi), (xl, yl) in (((0, 0, 2), (0, 0)), ((s - 1, 0, 1), (zl - 1, 0)), ((s - 1, s - 1, 3), (zl - 1, zl - 1))):
        d, vx, vy, vz = low[zi, yl, xl]
        assert tuple(xs[xi, yi, zi]) == (prev[zi, yi, xi], vy, vx * up, d * up, vz)
    assert xs[s - 1, 0, 1, 4] == 1000 * 1 + 10 * (zl - 1) + 4        # channel 4, which the residual reads, is vz


def test_pass_axis_order_by_hand(monkeypatch):
    """both passes with stand-in networks that repeat channel 0: which voxel ends up where"""
    zl, up = 4, 2
    s = zl * up
    low = _distinct_volume(zl)
    cfg = dict(NARROW)

    def first(ps, x, up_res, first_gen, *a, **k):
        assert first_gen and x.shape == (zl, zl, zl, 4)
        return x[..., 0:1].repeat(up_res, axis=1).repeat(up_res, axis=2)

    def second(ps, x, up_res, *a, **k):
        assert x.shape == (s, s, zl, 5)
        return x[..., 0:1].repeat(up_res, axis=2)

    monkeypatch.setattr(MR.ON, "growing_gen", first)
    monkeypatch.setattr(MR, "growing_gen_mode0", second)
    v1 = MR.pass1(None, cfg, low, up)
    assert v1.shape == (zl, s, s)
    for z, y, x in ((0, 0, 0), (1, 5, 2), (3, 7, 6)):
        assert v1[z, y, x] == low[z, y // up, x // up, 0]            # slices along z, nothing zoomed along z
    out0 = MR.pass2(None, cfg, v1, low, up, transpose_axis=0)
    out2 = MR.pass2(None, cfg, v1, low, up, transpose_axis=2)
    assert out0.shape == out2.shape == (s, s, s)
    for z, y, x in ((0, 0, 0), (3, 5, 2), (6, 7, 1)):
        assert out0[x, y, z] == v1[z // up, y, x]                    # the stack [x][y][z] as the reference stores it
        assert out2[z, y, x] == v1[z // up, y, x]                    # transposeAxis 2 restores [z, y, x]


# ---- the product's pass functions on the host backend ------------------------------------------------------------
class OracleGen(object):
    """callable with the Generator interface, evaluated by the restatement"""

    def __init__(self, seed, mode):
        from oracle import nets as ON
        self.ps, self.mode, self.cfg = ON.ParamSource(seed=seed), mode, dict(NARROW, upsampling_mode=mode)

    def __call__(self, x, y=None):
        from oracle import nets as ON
        if self.mode == 0:
            out = MR.growing_gen_mode0(self.ps, x.numpy(), 8, **NARROW)
        else:
            out = ON.growing_gen(self.ps, x.numpy(), 8, True, NARROW["filter_size"], NARROW["start_fms"], NARROW["max_fms"])
        return torch.as_tensor(out[..., 0])


@pytest.mark.parametrize("ta", [0, 2])
def test_pass_functions_on_the_host_backend(mpg, ta):
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    from oracle import nets as ON
    import cpu_backend
    sim, up = 2, 8
    low = synthetic_volume(sim, 4, 3)
    g1, g0 = OracleGen(5, 2), OracleGen(6, 0)
    want, want1 = MR.two_pass(ON.ParamSource(seed=5), ON.ParamSource(seed=6), NARROW, NARROW, low, up, ta)
    lt = torch.as_tensor(low)
    v1 = MP.plane_pass_8x(g1, lt, up, batch=1, backend=cpu_backend)
    assert v1.shape == (sim, sim * up, sim * up) and np.array_equal(v1.numpy(), want1)
    out = MP.upsample_pass_8x(g0, lt, v1, up, ta, batch=5, backend=cpu_backend)
    assert out.shape == (sim * up,) * 3 and np.array_equal(out.numpy(), want)
    both = MP.two_pass_8x_axis(g1, g0, lt, up, (2, 3), ta, backend=cpu_backend)
    assert np.array_equal(both[0].numpy(), want) and np.array_equal(both[1].numpy(), want1)
    # single_pass_8x dispatches on upsample_first and on the generator's mode
    a = MP.single_pass_8x(g1, lt, None, up, 0, batch=2, backend=cpu_backend, upsample_first=False)
    b = MP.single_pass_8x(g0, lt, a, up, ta, batch=2, backend=cpu_backend)
    assert np.array_equal(a.numpy(), want1) and np.array_equal(b.numpy(), want)


def test_pass_refusals(mpg):
    from mpgan_amd import multipass as MP
    import cpu_backend

    class TwoRanks(object):
        rank, world = 0, 2

    g1, g0 = OracleGen(5, 2), OracleGen(6, 0)
    low = torch.zeros((2, 2, 2, 4))
    prev = torch.zeros((2, 16, 16))
    with pytest.raises(ValueError, match="one process"):
        MP.plane_pass_8x(g1, low, 8, comm=TwoRanks(), backend=cpu_backend)
    with pytest.raises(ValueError, match="one process"):
        MP.upsample_pass_8x(g0, low, prev, 8, comm=TwoRanks(), backend=cpu_backend)
    with pytest.raises(ValueError, match="low-res channels"):
        MP.upsample_pass_8x(g0, low[..., :1], prev, 8, backend=cpu_backend)
    with pytest.raises(ValueError, match="previous volume"):
        MP.upsample_pass_8x(g0, low, torch.zeros((16, 16, 16)), 8, backend=cpu_backend)
    with pytest.raises(ValueError, match="upsampleFirst 0"):
        MP.single_pass_8x(g1, low, None, 8, 1, backend=cpu_backend, upsample_first=False)
    with pytest.raises(ValueError, match="upsamplingMode 0"):
        MP.single_pass_8x(g0, low, None, 8, 0, backend=cpu_backend)
    with pytest.raises(ValueError, match="vorticity"):
        MP.Generator("growing_gen", dict(tile_low=4, up_res=8, channels=4, upsampling_mode=0, vorticity=True, **NARROW), None)


# ---- planner ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(32, 16), (512, 256)])
def test_plan_fuses_the_column_depools_and_emits_the_residual_kernel(mpg, widths):
    from mpgan_amd import multipass as MP
    g = _gen(MP, 4, start_fms=widths[0], max_fms=widths[1])
    plan = g.sess.plan_summary(g.sampler)
    kinds = [e["kind"] for e in plan]
    assert "resize" not in kinds and "slice" not in kinds and "add" not in kinds
    assert set(kinds) <= {"conv2d_fused", "conv2d_small_pair", "bicubic_cols_add", "reshape"}
    up = sorted((s["weight"], s["up_log2"], s.get("up_x_only", 0), e.get("launches", 1))
                for e in plan if "segments" in e for s in e["segments"] if s["up_log2"])
    wide = 2 if widths[0] == 512 else 1          # the 256-wide first level runs as two channel windows
    assert up == sorted([("generator/genBlock%d/g_%s_first/weight" % (b, t), 1, 1, wide if b == 2 else 1)
                         for b in (2, 4, 8) for t in ("cA", "s")])
    res = [e for e in plan if e["kind"] == "bicubic_cols_add"]
    assert len(res) == 1 and (res[0]["c_src"], res[0]["factor"]) == (4, 8)
    assert kinds.index("bicubic_cols_add") == len(kinds) - 2 and kinds[-1] == "reshape"
    # the density head in front of it keeps no post-add
    head = [e for e in plan if e.get("cout") == 1 and "segments" in e]
    assert len(head) == 1 and head[0]["post_add"] is None


def test_other_residuals_keep_their_plan(mpg):
    """a resize that changes the rows, or a wider slice, stays the unfused composition"""
    from mpgan_amd import graph as G
    from mpgan_amd.session import Session
    prev = G.get_default_graph()
    g = G.reset_default_graph()
    try:
        x = G.reshape(G.placeholder([None, 8 * 4 * 5]), [-1, 8, 4, 5])
        d = G.reshape(G.placeholder([None, 16 * 8]), [-1, 16, 8, 1])
        both = d + G.resize_images(G.slice_channels(x, 4, 1), [16, 8], 2)
        cols = G.reshape(G.placeholder([None, 8 * 8]), [-1, 8, 8, 1]) + G.resize_images(G.slice_channels(x, 4, 1), [8, 8], 2)
    finally:
        G._default_graph[0] = prev
    assert Session._cols_residual(both) is None
    got = Session._cols_residual(cols)
    assert got is not None and got[2:] == (4, 2)
    sess = Session(device="cpu", graph=g)
    assert [e["kind"] for e in sess.plan_summary(cols)][-1] == "bicubic_cols_add"
    assert "bicubic_cols_add" not in [e["kind"] for e in sess.plan_summary(both)]


# ---- driver ----------------------------------------------------------------------------------------------------------
def test_driver_says_that_training_mode0_is_not_built(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", "multipassGAN-8x.py"), "out", "0", "upsamplingMode", "0", "upsampledData", "1",
           "upRes", "8", "basePath", str(tmp_path) + "/", "packedSimPath", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert "training upsamplingMode 0 is not built" in r.stdout
