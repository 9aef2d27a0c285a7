"""Non-cubic volumes on the GPU: rectangular generators against ``oracle.nets``, the 4x and 8x pipelines on the
(Z, Y, X) = (3, 5, 7) volume against tests/noncubic_ref.py with oracle networks, and the pipelines bit for bit against
the same Generator objects called on slice batches assembled here with the ``ops`` calls in the documented order.
Bounds: the TOL table of tests/test_nets_gpu.py (1e-4 for MPG_PREC_F16X3, 5e-4 for MPG_PREC_F16F6)."""
import numpy as np
import pytest
import torch

import noncubic_ref as NR
import _rank_noncubic as RN
from conftest import rel_l2
from oracle import nets as ON
from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {3: 1e-4, 2: 5e-4}
SHAPE = RN.SHAPE
Z, Y, X = SHAPE

CFG8 = [dict(c) for c in NR.CFG8X]            # the 8x networks at reduced widths


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _n(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def MP(mpg):
    from mpgan_amd import multipass
    return multipass


class _Memo(object):
    """an oracle generator that computes each distinct input once (the references of a module share their prefixes)"""

    def __init__(self, fn):
        self.fn, self.seen = fn, {}

    def __call__(self, x, y=None):
        key = (x.shape, x.tobytes(), None if y is None else y.tobytes())
        if key not in self.seen:
            self.seen[key] = self.fn(x, y)
        return self.seen[key]


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------- generators on rectangular planes
@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("nch", [1, 4])
@pytest.mark.parametrize("mode,tile", [(2, (5, 7)), (1, (3, 5)), (3, (3, 7))])
def test_gen_resnet_rectangular(MP, prec, nch, mode, tile):
    up = 4
    plane = tile if mode == 2 else (tile[0] * up, tile[1] * up)
    x = np.random.default_rng(nch * 10 + mode).random((3,) + plane + (nch,)).astype(np.float32)
    ps = ON.ParamSource(seed=5)
    ref = _cached(("gen4", nch, mode), lambda: ON.gen_resnet(ps, x, up, mode, True)[..., 0])
    ps.params.update(_cached(("gen4p", nch, mode), lambda: dict(ps.params)))
    gen = MP.Generator("gen_resnet", dict(tile_low=tile, up_res=up, channels=nch, upsampling_mode=mode, batch_norm=True),
                       params=ps.params, prec=prec)
    assert sorted(gen.graph.variables) == sorted(ps.params)          # the names of the square network
    assert gen.out_hw == (tile[0] * up, tile[1] * up) and gen.in_hw == plane
    y = gen(_t(x))
    assert tuple(y.shape) == (3,) + gen.out_hw
    assert rel_l2(_n(y), ref) < TOL[prec], rel_l2(_n(y), ref)
    # odd batch offsets: slice 1 of a C = 1 batch on (5, 7) starts 140 bytes into the buffer
    assert np.array_equal(_n(gen(_t(x)[1:])), _n(y)[1:])
    with pytest.raises(ValueError, match=r"built for input planes %d x %d .*batch \(3, %d, %d, %d\) has planes %d x %d"
                       % (plane + (plane[1], plane[0], nch, plane[1], plane[0]))):
        gen(_t(x.transpose(0, 2, 1, 3)))


@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("net,tile", [(0, (5, 7)), (1, (5, 3)), (2, (3, 7))])
def test_growing_gen_rectangular(MP, prec, net, tile):
    cfg, up, nch = CFG8[net], 8, 4
    high = (tile[0] * up, tile[1] * up)
    rng = np.random.default_rng(3 + net)
    ps = ON.ParamSource(seed=11)
    if net == 0:
        x, yp = rng.standard_normal((2,) + tile + (nch + 2,)).astype(np.float32), None
        ref = _cached(("gen8", net), lambda: NR.oracle_growing_gen(ps, cfg, up, True)(x))
    else:
        x = rng.standard_normal((2,) + tile + (nch,)).astype(np.float32)
        yp = rng.random((2,) + high).astype(np.float32)
        ref = _cached(("gen8", net), lambda: NR.oracle_growing_gen(ps, cfg, up, False)(x, yp))
    ps.params.update(_cached(("gen8p", net), lambda: dict(ps.params)))
    gen = MP.Generator("growing_gen", dict(tile_low=tile, up_res=up, channels=nch, **cfg), params=ps.params, prec=prec)
    assert sorted(gen.graph.variables) == sorted(ps.params)
    assert gen.out_hw == high
    y = gen(_t(x), None if yp is None else _t(yp))
    assert tuple(y.shape) == (2,) + high
    assert rel_l2(_n(y), ref) < TOL[prec], rel_l2(_n(y), ref)
    if yp is not None:
        with pytest.raises(ValueError, match="built for previous-pass planes %d x %d" % high):
            gen(_t(x), _t(yp.transpose(0, 2, 1)))


# ---------------------------------------------------------------------------- 4x pipelines on (3, 5, 7)
def _gens_4x(MP, shape, nch, prec, params):
    planes = MP.pass_planes_4x(shape)
    return [MP.Generator("gen_resnet", dict(tile_low=planes[i], up_res=4, channels=nch, upsampling_mode=m), p, prec, seed=50 + i)
            for i, (m, p) in enumerate(zip((2, 1, 3), params))]


def _ref_4x(nch):
    def make():
        vs = 0.7 if nch > 1 else 1.0
        low = RN.volume(SHAPE, nch, 10 + nch)
        ps = [ON.ParamSource(seed=71 + i) for i in range(3)]
        g = [NR.oracle_gen_resnet(p, 4, m) for p, m in zip(ps, (2, 1, 3))]
        final, v1 = NR.two_pass_4x(g[0], g[1], low, 4, vs)
        return low, vs, [p.params for p in ps], final, v1, NR.refine_mode3_4x(g[2], final, low, 4, vs)
    return _cached(("4x", nch), make)


@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("nch", [1, 4])
def test_two_pass_4x(MP, prec, nch):
    low, vs, params, ref, ref1, _ = _ref_4x(nch)
    g = _gens_4x(MP, SHAPE, nch, prec, params)
    out, v1 = MP.two_pass_4x(g[0], g[1], _t(low), 4, batch=8, vel_scale=vs)
    assert tuple(out.shape) == tuple(v1.shape) == (4 * Z, 4 * Y, 4 * X)
    e1, e2 = rel_l2(_n(v1), ref1), rel_l2(_n(out), ref)
    print("two_pass_4x %s C=%d prec %d: pass 1 %.3e, final %.3e" % (SHAPE, nch, prec, e1, e2))
    assert e1 < TOL[prec] and e2 < TOL[prec], (e1, e2)
    out5, _ = MP.two_pass_4x(g[0], g[1], _t(low), 4, batch=5, vel_scale=vs)        # ragged, and unaligned at C = 1
    assert np.array_equal(_n(out5), _n(out))


def test_three_pass_4x(MP):
    """modes 2 -> 1 -> 3, held to the bound of test_nets_gpu.test_three_pass_4x"""
    low, vs, params, ref, _, ref3 = _ref_4x(4)
    g = _gens_4x(MP, SHAPE, 4, 3, params)
    out2, _ = MP.two_pass_4x(g[0], g[1], _t(low), 4, vel_scale=vs)
    out3 = MP.refine_pass_4x(g[2], _t(low), out2, 4, mode=3, vel_scale=vs)
    assert tuple(out3.shape) == (4 * Z, 4 * Y, 4 * X)
    e = rel_l2(_n(out3), ref3)
    print("three-pass 4x %s: %.3e" % (SHAPE, e))
    assert e < 2e-4, e
    # the second network as its own invocation (mode 1) gives what the pair gives
    assert np.array_equal(_n(MP.refine_pass_4x(g[1], _t(low), MP.two_pass_4x(g[0], g[1], _t(low), 4, vel_scale=vs)[1], 4,
                                               mode=1, vel_scale=vs)), _n(out2))


def test_two_pass_4x_larger(MP):
    """8 x 12 x 16: planes of 48 x 64 and 32 x 48 pixels, more than one convolution tile each"""
    shape, prec = (8, 12, 16), 3
    low = RN.volume(shape, 4, 5)
    g = _gens_4x(MP, shape, 4, prec, [None, None, None])
    p = [x.params() for x in g[:2]]
    o = [lambda x, y=None, p=p[i], m=m: torch_ref.gen_resnet(p, x, 4, m, True)[..., 0] for i, m in enumerate((2, 1))]
    ref, ref1 = NR.two_pass_4x(o[0], o[1], low, 4, 0.7)
    out, v1 = MP.two_pass_4x(g[0], g[1], _t(low), 4, vel_scale=0.7)
    assert tuple(out.shape) == (32, 48, 64)
    e1, e2 = rel_l2(_n(v1), ref1), rel_l2(_n(out), ref)
    print("two_pass_4x %s prec %d: pass 1 %.3e, final %.3e" % (shape, prec, e1, e2))
    assert e1 < TOL[prec] and e2 < TOL[prec], (e1, e2)


# ---------------------------------------------------------------------------- 8x pipelines on (3, 5, 7)
def _cfgs8(adj):
    return [dict(CFG8[0], add_adj=adj), CFG8[1], CFG8[2]]


def _ref_8x(nch, adj):
    def make():
        low = RN.volume(SHAPE, nch, RN.PARITY_SEEDS_8X[nch])
        pss = [ON.ParamSource(seed=41 + i) for i in range(3)]
        og = [_Memo(NR.oracle_growing_gen(p, c, 8, i == 0)) for i, (p, c) in enumerate(zip(pss, _cfgs8(adj)))]
        refs = {n: NR.multipass_8x(og[:n], adj, low, 8) for n in (1, 2, 3)}
        return low, pss, og, refs
    return _cached(("8x", nch, adj), make)


def _gens_8x(MP, planes, nch, adj, prec, pss):
    return [MP.Generator("growing_gen", dict(tile_low=pl, up_res=8, channels=nch, **c), None if ps is None else ps.params, prec,
                         seed=60 + i) for i, (pl, c, ps) in enumerate(zip(planes, _cfgs8(adj), pss))]


@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("nch,adj", [(4, True), (4, False), (1, True)])
def test_multipass_8x(MP, prec, nch, adj):
    low, pss, _, refs = _ref_8x(nch, adj)
    gens = _gens_8x(MP, MP.pass_planes_8x(SHAPE), nch, adj, prec, pss)
    for n in (1, 2, 3):
        out = MP.multipass_8x(gens[:n], _t(low), 8)
        assert tuple(out.shape) == (8 * Z, 8 * Y, 8 * X)
        e = rel_l2(_n(out), refs[n])
        print("multipass_8x %s C=%d add_adj %d, %d nets, prec %d: %.3e" % (SHAPE, nch, adj, n, prec, e))
        assert e < TOL[prec], (n, e)


@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("nch,ta", [(4, 0), (4, 1), (4, 2), (4, 3), (1, 0), (1, 3)])
def test_single_pass_8x(MP, prec, nch, ta):
    low, pss, og, _ = _ref_8x(nch, True)
    w1 = _cached(("8x1", nch, ta), lambda: NR.single_pass_8x(og[0], True, low, None, 8, ta))
    w2 = _cached(("8x2", nch, ta), lambda: NR.single_pass_8x(og[1], False, low, w1, 8, ta))
    plane = MP.single_pass_plane_8x(SHAPE, ta)[0]
    gens = _gens_8x(MP, [plane, plane], nch, True, prec, pss[:2])
    v1 = MP.single_pass_8x(gens[0], _t(low), None, 8, ta)              # batch 2: odd byte offsets at C = 1
    v2 = MP.single_pass_8x(gens[1], _t(low), v1, 8, ta)
    assert tuple(v1.shape) == tuple(v2.shape) == (8 * Z, 8 * Y, 8 * X)
    e1, e2 = rel_l2(_n(v1), w1), rel_l2(_n(v2), w2)
    print("single_pass_8x %s C=%d transposeAxis %d prec %d: %.3e, %.3e" % (SHAPE, nch, ta, prec, e1, e2))
    assert e1 < TOL[prec] and e2 < TOL[prec], (e1, e2)


# ---------------------------------------------------------------------------- bit for bit
def _batches(gen, xs, ys=None, batch=8):
    return torch.cat([gen(xs[j:j + batch], None if ys is None else ys[j:j + batch]) for j in range(0, xs.shape[0], batch)], 0)


def test_4x_equals_hand_assembled_batches(MP, gpu_ops):
    ops, vs, up = gpu_ops, 0.7, 4
    low = _t(RN.volume(SHAPE, 4, 14))
    g = _gens_4x(MP, SHAPE, 4, 2, [None] * 3)
    out, v1 = MP.two_pass_4x(g[0], g[1], low, up, batch=8, vel_scale=vs)
    out3 = MP.refine_pass_4x(g[2], low, out, up, mode=3, batch=8, vel_scale=vs)
    # pass 1: all velocities times velScale, zoom z, slices along z, cutoff
    low1 = ops.channel_gather(low, None, [0, 1, 2, 3], [1.0, vs, vs, vs])
    w1 = ops.cutoff(_batches(g[0], ops.axis_zoom_linear(low1, 0, up)), MP.CUTOFF)
    assert torch.equal(w1, v1)
    # velocities times upRes, vy and vz times velScale, zoomed along z, y, x
    vel = ops.channel_gather(low, None, [1, 2, 3], [float(up)] * 3, [1.0, vs, vs])
    for ax in range(3):
        vel = ops.axis_zoom_linear(vel, ax, up)
    # pass 2: [x][z][y] planes of (pass 1, vy, vz, vx); result [x][z][y] -> [z][y][x], cutoff
    x2 = ops.channel_gather(ops.volume_transpose(w1, (2, 0, 1)).reshape(4 * X, 4 * Z, 4 * Y, 1),
                            ops.volume_transpose(vel, (2, 0, 1), chan_map=[1, 2, 0]), [0, 1, 2, 3])
    w2 = ops.volume_transpose(_batches(g[1], x2), (1, 2, 0), cutoff=MP.CUTOFF)
    assert torch.equal(w2, out)
    # mode 3: [y][z][x] planes of (pass 2, vx, vz, vy); result [y][z][x] -> [z][y][x], cutoff
    x3 = ops.volume_transpose(ops.channel_gather(w2.reshape(4 * Z, 4 * Y, 4 * X, 1), vel, [0, 1, 2, 3]), (1, 0, 2),
                              chan_map=[0, 1, 3, 2])
    assert tuple(x3.shape) == (4 * Y, 4 * Z, 4 * X, 4)
    w3 = ops.volume_transpose(_batches(g[2], x3), (1, 0, 2), cutoff=MP.CUTOFF)
    assert torch.equal(w3, out3)


def test_8x_equals_hand_assembled_batches(MP, gpu_ops):
    ops, up = gpu_ops, 8
    low = _t(RN.volume(SHAPE, 4, 15))
    gens = _gens_8x(MP, MP.pass_planes_8x(SHAPE), 4, True, 2, [None] * 3)
    # pass 1: zoom z, add_adj_idcs channels, slices along z -> [z][y][x]
    o1 = _batches(gens[0], ops.add_adjacent(ops.axis_zoom_linear(low, 0, up)), None, 8)
    # pass 2: zoom x, [x][y][z_low] planes with vx <-> vz, on the planes [x][y][z] of pass 1 -> [x][y][z]
    x2 = ops.volume_transpose(ops.axis_zoom_linear(low, 2, up), (2, 1, 0), chan_map=[0, 3, 2, 1])
    assert tuple(x2.shape) == (8 * X, Y, Z, 4)
    o2 = _batches(gens[1], x2, ops.volume_transpose(o1, (2, 1, 0)), 2)
    # pass 3: zoom y, [y][z_low][x_low] planes with vy <-> vz, on the planes [y][z][x] of pass 2 -> [y][z][x]
    x3 = ops.volume_transpose(ops.axis_zoom_linear(low, 1, up), (1, 0, 2), chan_map=[0, 1, 3, 2])
    assert tuple(x3.shape) == (8 * Y, Z, X, 4)
    o3 = _batches(gens[2], x3, ops.volume_transpose(o2, (1, 2, 0)), 2)
    want = {1: ops.cutoff(o1, MP.CUTOFF), 2: ops.volume_transpose(o2, (2, 1, 0), cutoff=MP.CUTOFF),
            3: ops.volume_transpose(o3, (1, 0, 2), cutoff=MP.CUTOFF)}
    for n in (1, 2, 3):
        assert torch.equal(MP.multipass_8x(gens[:n], low, up), want[n]), n
    # one network per invocation, transposeAxis 3: zoom x, [x][z_low][y_low] planes, channels (d, vy, vz, vx)
    plane = MP.single_pass_plane_8x(SHAPE, 3)[0]
    g = _gens_8x(MP, [plane, plane], 4, True, 2, [None] * 2)
    xs = ops.volume_transpose(ops.axis_zoom_linear(low, 2, up), (2, 0, 1), chan_map=[0, 2, 3, 1])
    assert tuple(xs.shape) == (8 * X, Z, Y, 4)
    s1 = ops.volume_transpose(_batches(g[0], ops.add_adjacent(xs), None, 2), (1, 2, 0), cutoff=MP.CUTOFF)
    v1 = MP.single_pass_8x(g[0], low, None, up, 3)
    assert torch.equal(v1, s1)
    s2 = ops.volume_transpose(_batches(g[1], xs, ops.volume_transpose(v1, (2, 0, 1)), 2), (1, 2, 0), cutoff=MP.CUTOFF)
    assert torch.equal(MP.single_pass_8x(g[1], low, v1, up, 3), s2)


def test_batches_lanes_and_reruns(MP):
    """batch 5 equals batch 8, one lane equals two, a second run gives the same bits"""
    low4, low8 = _t(RN.volume(SHAPE, 4, 16)), _t(RN.volume(SHAPE, 1, 17))
    g4 = _gens_4x(MP, SHAPE, 4, 2, [None] * 3)
    g8 = _gens_8x(MP, MP.pass_planes_8x(SHAPE), 1, True, 2, [None] * 3)
    keep = MP.PASS_LANES[0]
    res = {}
    try:
        for lanes, batch in ((1, 8), (2, 8), (2, 5), (2, 8)):
            MP.set_pass_lanes(lanes)
            a, _ = MP.two_pass_4x(g4[0], g4[1], low4, 4, batch=batch, vel_scale=0.7)
            a3 = MP.refine_pass_4x(g4[2], low4, a, 4, mode=3, batch=batch, vel_scale=0.7)
            b = MP.multipass_8x(g8, low8, 8, batches=(batch,) * 3)
            c = MP.single_pass_8x(g8[0], low8, None, 8, 0, batch=batch)
            torch.cuda.synchronize()
            res.setdefault((lanes, batch), []).append([_n(v) for v in (a, a3, b, c)])
    finally:
        MP.set_pass_lanes(keep)
    first = res[(1, 8)][0]
    for runs in res.values():
        for got in runs:
            for u, v in zip(got, first):
                assert np.array_equal(u, v)
    assert len(res[(2, 8)]) == 2


def test_two_pass_4x_batch_with_a_lane_pair(MP):
    lows = [_t(RN.volume(SHAPE, 4, 18 + i)) for i in range(3)]
    g = _gens_4x(MP, SHAPE, 4, 2, [None] * 3)
    want = [_n(MP.two_pass_4x(g[0], g[1], v, 4, batch=8, vel_scale=0.7)[0]) for v in lows]
    got = MP.two_pass_4x_batch(g[0], g[1], lows, 4, batch=8, vel_scale=0.7, lanes=[(g[0].clone(), g[1].clone())])
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert tuple(a.shape) == (4 * Z, 4 * Y, 4 * X) and np.array_equal(_n(a), b)


def test_wrongly_shaped_generator_is_refused_before_any_launch(MP):
    g = _gens_4x(MP, SHAPE, 1, 2, [None] * 3)
    low = _t(RN.volume(SHAPE, 1, 19))
    with pytest.raises(ValueError, match=r"two_pass_4x pass 1 runs planes of 20 x 28 \(low 5 x 7\): its generator was built "
                                         r"for 12 x 20 \(tile_low \(3, 5\)\)"):
        MP.two_pass_4x(g[1], g[1], low, 4)
    cube = MP.Generator("gen_resnet", dict(tile_low=5, up_res=4, channels=1, upsampling_mode=2), None, 2)
    with pytest.raises(ValueError, match="its generator was built for 20 x 20"):
        MP.two_pass_4x(cube, g[1], low, 4)
