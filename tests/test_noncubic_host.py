"""Non-cubic volumes through the 4x and 8x inference pipelines, on the CPU: the marshalling of ``multipass`` (on
tests/cpu_backend.py) against the numpy restatements of tests/noncubic_ref.py, which are themselves anchored to
``oracle.multipass`` on a cube.  The main shape (Z, Y, X) = (3, 5, 7) has three different, odd sizes."""
import os

import numpy as np
import pytest
import torch

import noncubic_ref as NR
import _rank_noncubic as RN
from oracle import multipass as OM
from oracle import nets as ON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = RN.SHAPE
CFG8 = [dict(filter_size=3, start_fms=32, max_fms=32, first_nn_arch=True, add_adj=True),
        dict(filter_size=3, start_fms=32, max_fms=16),
        dict(filter_size=3, start_fms=16, max_fms=16, use_res_net=False)]


@pytest.fixture(scope="module")
def MP(mpg):
    from mpgan_amd import multipass
    return multipass


# ---------------------------------------------------------------------------- the restatements on a cube
@pytest.mark.parametrize("nch", [1, 4])
def test_restated_4x_equals_the_oracle_on_a_cube(mpg, nch):
    from mpgan_amd.synthetic import synthetic_volume
    low = synthetic_volume(4, nch, 3)
    ps = [ON.ParamSource(seed=5 + i) for i in range(3)]
    want2, want1 = OM.two_pass_4x(ps[0], ps[1], low, 4, True, 0.7)
    want3 = OM.pass3_4x(ps[2], want2, low, 4, True, 0.7)
    gens = [NR.oracle_gen_resnet(p, 4, m) for p, m in zip(ps, (2, 1, 3))]
    got2, got1 = NR.two_pass_4x(gens[0], gens[1], low, 4, 0.7)
    assert np.array_equal(got1, want1) and np.array_equal(got2, want2)
    assert np.array_equal(NR.refine_mode3_4x(gens[2], got2, low, 4, 0.7), want3)
    assert np.array_equal(NR.refine_mode1_4x(gens[1], got1, low, 4, 0.7), want2)


def test_restated_8x_equals_the_oracle_on_a_cube(mpg):
    from mpgan_amd.synthetic import synthetic_volume
    low = synthetic_volume(4, 4, 2)
    pss = [ON.ParamSource(seed=41 + i) for i in range(3)]
    gens = [NR.oracle_growing_gen(p, c, 8, i == 0) for i, (p, c) in enumerate(zip(pss, CFG8))]
    for n in (1, 2, 3):
        assert np.array_equal(NR.multipass_8x(gens[:n], True, low, 8), OM.multipass_8x(pss[:n], CFG8[:n], low, 8)), n
    for ta in range(4):
        w1 = OM.single_pass_8x(pss[0], CFG8[0], low, None, 8, ta)
        assert np.array_equal(NR.single_pass_8x(gens[0], True, low, None, 8, ta), w1), ta
        w2 = OM.single_pass_8x(pss[1], CFG8[1], low, w1, 8, ta)
        assert np.array_equal(NR.single_pass_8x(gens[1], False, low, w1, 8, ta), w2), ta
    y = np.random.default_rng(0).random((2, 8, 8, 1)).astype(np.float32)
    x = np.random.default_rng(1).random((2, 2, 2, 3)).astype(np.float32)
    assert np.array_equal(NR.gen2_input(y, x, (8, 8)), ON.gen2_input(y, x, 8))


@pytest.mark.parametrize("net,seed,nch,adj", [(0, 11, 4, True), (0, 41, 4, True), (0, 41, 4, False), (0, 41, 1, True),
                                              (1, 11, 4, False), (1, 42, 4, False), (2, 11, 4, False), (2, 43, 4, False)])
def test_reduced_8x_networks_are_well_conditioned(net, seed, nch, adj):
    """the networks the GPU tests hold to the 1e-4 / 5e-4 table (noncubic_ref.CFG8X), with the seeds used there, the
    first one on the slices the pipelines feed it: the oracle's output moves by less than 2e-4 under relative weight
    noise of 2e-5 (the full-size networks: 7e-5)"""
    from conftest import rel_l2
    from oracle import ops as O
    cfg, tile = dict(NR.CFG8X[net], add_adj=adj), ((5, 7), (5, 3), (3, 7))[net]
    rng = np.random.default_rng(4)
    if net == 0:
        x, y = O.zoom_axis_linear(RN.volume(SHAPE, nch, RN.PARITY_SEEDS_8X[nch]), 0, 8)[8:12], None
        x = OM.add_adjacent(x, nch) if adj else x
    else:
        x = rng.standard_normal((2,) + tile + (nch,)).astype(np.float32)
        y = rng.random((2, tile[0] * 8, tile[1] * 8)).astype(np.float32)
    ps = ON.ParamSource(seed=seed)
    ref = NR.oracle_growing_gen(ps, cfg, 8, net == 0)(x, y)
    for draw in range(3):
        noise = np.random.default_rng(100 + draw)
        moved = ON.ParamSource(params={k: (v * (1 + 2e-5 * noise.standard_normal(v.shape))).astype(np.float32)
                                       for k, v in ps.params.items()})
        assert rel_l2(NR.oracle_growing_gen(moved, cfg, 8, net == 0)(x, y), ref) < 2e-4


@pytest.mark.parametrize("nch,ta", [(4, 0), (4, 1), (4, 2), (4, 3), (1, 0), (1, 3)])
def test_8x_parity_volumes_are_well_conditioned(nch, ta):
    """the same for the first network over the whole volume, in every slicing the GPU tests run (the planes of
    transposeAxis 0 are those of multipass_8x): RN.PARITY_SEEDS_8X names volumes without a pixel-norm singularity"""
    from conftest import rel_l2
    low, cfg = RN.volume(SHAPE, nch, RN.PARITY_SEEDS_8X[nch]), NR.CFG8X[0]
    ps = ON.ParamSource(seed=41)
    ref = NR.single_pass_8x(NR.oracle_growing_gen(ps, cfg, 8, True), True, low, None, 8, ta, apply_cutoff=False)
    for draw in range(2):
        noise = np.random.default_rng(100 + draw)
        moved = ON.ParamSource(params={k: (v * (1 + 2e-5 * noise.standard_normal(v.shape))).astype(np.float32)
                                       for k, v in ps.params.items()})
        got = NR.single_pass_8x(NR.oracle_growing_gen(moved, cfg, 8, True), True, low, None, 8, ta, apply_cutoff=False)
        assert rel_l2(got, ref) < 2e-4


# ---------------------------------------------------------------------------- (3, 5, 7) on the CPU backend
def _restated(shape=SHAPE):
    """what RN.pipelines computes, by the restatements"""
    outs = {}
    for nch in (1, 4):
        vs = 0.7 if nch > 1 else 1.0
        low = RN.volume(shape, nch, 10 + nch)
        g = RN.stand_ins(4)
        final, v1 = NR.two_pass_4x(g[0], g[1], low, 4, vs)
        outs["4x_c%d" % nch], outs["4x_c%d_v1" % nch] = final, v1
        outs["4x_c%d_batch1" % nch] = NR.two_pass_4x(g[0], g[1], RN.volume(shape, nch, 20 + nch), 4, vs)[0]
        r1 = NR.refine_mode1_4x(g[1], final, low, 4, vs)
        outs["4x_c%d_mode1" % nch] = r1
        outs["4x_c%d_mode3" % nch] = NR.refine_mode3_4x(g[2], r1, low, 4, vs)
        for adj in (False, True):
            g = RN.stand_ins(8, adj)
            for n in (1, 2, 3):
                outs["8x_c%d_adj%d_%dnets" % (nch, adj, n)] = NR.multipass_8x(g[:n], adj, low, 8)
            for ta in range(4):
                v = NR.single_pass_8x(g[0], adj, low, None, 8, ta)
                outs["8x_c%d_adj%d_single_ta%d" % (nch, adj, ta)] = v
                outs["8x_c%d_adj%d_single2_ta%d" % (nch, adj, ta)] = NR.single_pass_8x(g[1], False, low, v, 8, ta)
    return outs


@pytest.fixture(scope="module")
def restated():
    return _restated()


def _same(got, want, skip=()):
    assert set(want) - set(skip) <= set(got)
    hi = tuple(4 * n for n in SHAPE), tuple(8 * n for n in SHAPE)
    for k, v in want.items():
        if k in skip:
            continue
        assert got[k].shape == v.shape == hi[k.startswith("8x")], (k, got[k].shape, v.shape)
        assert np.array_equal(got[k], v), k
        assert np.abs(v).max() > 0


def test_pipelines_equal_the_restatements(MP, restated):
    _same(RN.pipelines(batch=1), restated)


def test_ragged_batches(MP, restated):
    _same(RN.pipelines(batch=5), restated)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("exchange", ["all_gather", "all_to_all"])
def test_two_gloo_ranks_equal_one(MP, restated, tmp_path, exchange):
    from mpgan_amd import launch
    path = str(tmp_path / "rank%d.npz")
    rc, out = launch.spawn_ranks(os.path.join(ROOT, "tests", "_rank_noncubic.py"), [exchange, path], 2, timeout=500)
    assert rc == 0, out
    for r in range(2):
        got = dict(np.load(path % r))
        # the block exchange never assembles the pass-1 volume on several ranks
        _same(got, restated, skip=[k for k in restated if k.endswith("_v1")] if exchange == "all_to_all" else ())


def test_pass_planes(MP):
    z, y, x = SHAPE
    assert MP.pass_planes_4x(SHAPE) == ((y, x), (z, y), (z, x))
    assert MP.pass_planes_8x(SHAPE) == ((y, x), (y, z), (z, x))
    assert MP.pass_counts_4x(SHAPE, 4) == (12, 28, 20) and MP.pass_counts_8x(SHAPE, 8) == (24, 56, 40)
    assert [MP.single_pass_plane_8x(SHAPE, ta) for ta in range(4)] == [((y, x), z), ((z, x), y), ((y, z), x), ((z, y), x)]
    assert MP.pass_planes_4x((4, 4, 4)) == ((4, 4),) * 3 and MP.pass_planes_8x((4, 4, 4)) == ((4, 4),) * 3


# ---------------------------------------------------------------------------- refusals
class _Backend(object):
    """a backend on which nothing may run"""

    def __getattr__(self, name):
        raise AssertionError("backend.%s was called" % name)


class _Sink(object):
    def check_comm(self, comm):
        pass


class _Ranks(object):
    def __init__(self, world):
        self.rank, self.world = 0, world


def _low(nch=4):
    return torch.as_tensor(RN.volume(SHAPE, nch, 1))


def _refused(match, fn, *args, **kw):
    gens = [g for a in args for g in (a if isinstance(a, list) else [a]) if isinstance(g, NR.StandIn)]
    with pytest.raises(ValueError, match=match):
        fn(*args, backend=_Backend(), **kw)
    assert all(g.calls == 0 for g in gens)


def test_multipass_8x_transpose_axis_needs_a_cube(MP):
    for ta in (1, 2, 3):
        _refused("multipass_8x with transposeAxis %d: the 3 x 5 x 7 volume is not a cube" % ta, MP.multipass_8x,
                 RN.stand_ins(8), _low(), 8, transpose_axis=ta)


def test_mode0_pipelines_need_a_cube(MP):
    g, prev = NR.StandIn("low", 4), torch.zeros(3, 20, 28)
    for name, args in (("plane_pass_4x", (g, _low())), ("upsample_pass_4x", (g, _low(), prev)),
                       ("two_pass_4x_axis", (g, g, _low())), ("plane_pass_8x", (g, _low())),
                       ("upsample_pass_8x", (g, _low(), prev)), ("two_pass_8x_axis", (g, g, _low()))):
        _refused(name + ": the 3 x 5 x 7 volume is not a cube; the upsamplingMode 0 pipelines", getattr(MP, name), *args)


def test_previews_need_a_cube(MP):
    g = RN.stand_ins(8)
    _refused("previews: the 3 x 5 x 7 volume is not a cube", MP.multipass_8x, g, _low(), 8, previews=_Sink())
    _refused("previews: the 3 x 5 x 7 volume is not a cube", MP.single_pass_8x, g[0], _low(), None, 8, previews=_Sink())
    _refused("previews: the 3 x 5 x 7 volume is not a cube", MP.refine_pass_4x, g[0], _low(), torch.zeros(12, 20, 28), 4,
             previews=_Sink())


def test_wrongly_shaped_generator(MP):
    ok4 = [NR.StandIn("low", 4, out_hw=(20, 28)), NR.StandIn("high", 4, out_hw=(12, 20)), NR.StandIn("high", 4, out_hw=(12, 28))]
    bad = NR.StandIn("high", 4, out_hw=(20, 12))
    _refused(r"two_pass_4x pass 2 runs planes of 12 x 20 \(low 3 x 5\): its generator was built for 20 x 12",
             MP.two_pass_4x, ok4[0], bad, _low(), 4)
    _refused(r"two_pass_4x pass 1 runs planes of 20 x 28 \(low 5 x 7\): its generator was built for 12 x 28",
             MP.two_pass_4x_batch, ok4[2], ok4[1], [_low()], 4)
    _refused(r"refine_pass_4x \(upsamplingMode 3\) runs planes of 12 x 28 .*built for 12 x 20",
             MP.refine_pass_4x, ok4[1], _low(), torch.zeros(12, 20, 28), 4, mode=3)
    ok8 = [NR.StandIn("low", 8, out_hw=(40, 56)), NR.StandIn("later", 8, out_hw=(40, 24)), NR.StandIn("later", 8, out_hw=(24, 56))]
    _refused(r"multipass_8x pass 3 runs planes of 24 x 56 \(low 3 x 7\): its generator was built for 40 x 24",
             MP.multipass_8x, [ok8[0], ok8[1], ok8[1]], _low(), 8)
    _refused(r"single_pass_8x \(transposeAxis 2\) runs planes of 40 x 24 .*built for 24 x 56",
             MP.single_pass_8x, ok8[2], _low(), None, 8, 2)
    # and rightly shaped ones run
    out, _ = MP.two_pass_4x(ok4[0], ok4[1], _low(), 4, backend=__import__("cpu_backend"))
    assert out.shape == (12, 20, 28)


def test_world_size_must_divide_every_pass(MP):
    g4, g8 = RN.stand_ins(4), RN.stand_ins(8)
    # 12, 28, 20 slices at 4x; 24, 56, 40 at 8x
    _refused("two_pass_4x pass 1: slice count 12 does not divide over 8 ranks", MP.two_pass_4x, g4[0], g4[1], _low(), 4,
             comm=_Ranks(8))
    _refused("two_pass_4x pass 2: slice count 28 does not divide over 3 ranks", MP.two_pass_4x, g4[0], g4[1], _low(), 4,
             comm=_Ranks(3))
    _refused(r"refine_pass_4x \(upsamplingMode 3\): slice count 20 does not divide over 3 ranks", MP.refine_pass_4x, g4[2],
             _low(), torch.zeros(12, 20, 28), 4, mode=3, comm=_Ranks(3))
    _refused("multipass_8x pass 2: slice count 56 does not divide over 3 ranks", MP.multipass_8x, g8, _low(), 8,
             comm=_Ranks(3))
    _refused("multipass_8x pass 1: slice count 24 does not divide over 5 ranks", MP.multipass_8x, g8[:2], _low(), 8,
             comm=_Ranks(5))
    _refused("multipass_8x pass 3: slice count 16 does not divide over 3 ranks", MP.multipass_8x, g8,
             torch.as_tensor(RN.volume((3, 2, 3), 4, 1)), 8, comm=_Ranks(3))
    _refused(r"single_pass_8x \(transposeAxis 1\): slice count 40 does not divide over 3 ranks", MP.single_pass_8x, g8[0],
             _low(), None, 8, 1, comm=_Ranks(3))
