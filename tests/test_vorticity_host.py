"""useVorticities without a GPU: the restatement (vorticity_ref.py) against known answers, the product's host path
(multi-pass-gan_amd/vorticity.py) against the restatement bit for bit, the widened networks' variable shapes, and the pass
functions of multipass.py on the host backend with oracle generators against slice batches assembled by hand."""
import numpy as np
import pytest
import torch

import vorticity_ref as VR
from oracle import multipass as OM
from oracle import nets as ON


def test_known_answers():
    h, w = 6, 9
    x = np.zeros((2, h, w, 4), np.float32)
    x[..., 1] = np.arange(w, dtype=np.float32)[None, None, :]             # vx = column index
    y = VR.append(x)
    assert y.shape == (2, h, w, 7) and y.dtype == np.float32
    assert np.all(y[:, 1:-1, 1:-1, 6] == -1.0)
    x = np.zeros((2, h, w, 4), np.float32)
    x[..., 2] = np.arange(h, dtype=np.float32)[None, :, None]             # vy = row index
    y = VR.append(x)
    assert np.all(y[:, 1:-1, 1:-1, 6] == 1.0)
    # the density and vz take no part
    x = VR.cases((2, h, w, 4), 0)
    z = x.copy()
    z[..., 0] += 1.0
    z[..., 3] *= 2.0
    assert np.array_equal(VR.append(x)[..., 6], VR.append(z)[..., 6])


@pytest.mark.parametrize("shape", [(3, 5, 7, 4), (2, 1, 6, 8, 6)])
def test_border_zero_channels_and_copy(shape):
    x = VR.cases(shape, 1)
    y = VR.append(x)
    c = shape[-1]
    assert np.array_equal(y[..., :c].view(np.uint32), x.view(np.uint32))   # copied bit for bit
    assert not y[..., c].any() and not y[..., c + 1].any()
    v = y[..., c + 2]
    assert not v[..., 0, :].any() and not v[..., -1, :].any() and not v[..., :, 0].any() and not v[..., :, -1].any()
    assert np.count_nonzero(v[..., 1:-1, 1:-1]) > 0
    # one pixel by hand, in the order of the statement
    i, j = 2, 3
    want = np.float32(0.5) * ((x[..., i + 1, j, 2] - x[..., i - 1, j, 2]) - (x[..., i, j + 1, 1] - x[..., i, j - 1, 1]))
    assert np.array_equal(v[..., i, j], want)


@pytest.mark.parametrize("shape", VR.NO_INTERIOR)
def test_no_interior(mpg, shape):
    from mpgan_amd import vorticity
    x = VR.cases(shape, 2) + np.float32(3.0)
    for y in (VR.append(x), vorticity.append(x)):
        assert y.shape == shape[:-1] + (7,)
        assert np.array_equal(y[..., :4], x) and not y[..., 4:].any()


@pytest.mark.parametrize("shape", [(3, 1, 5, 7, 4), (2, 1, 8, 8, 6), (4, 1, 3, 3, 4), (1, 1, 16, 12, 6)])
def test_product_host_path_equals_the_restatement(mpg, shape):
    from mpgan_amd import vorticity
    x = VR.cases(shape, 3)
    want = VR.append(x)
    got = vorticity.append(x)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    t = vorticity.append(torch.as_tensor(x))
    assert isinstance(t, torch.Tensor) and not t.is_cuda and t.dtype == torch.float32
    assert np.array_equal(t.numpy().view(np.uint32), want.view(np.uint32))
    # a view that is not contiguous gives the same
    xt = np.ascontiguousarray(np.swapaxes(x, 2, 3))
    assert np.array_equal(vorticity.append(np.swapaxes(xt, 2, 3)), want)
    with pytest.raises(TypeError):
        vorticity.append(x.astype(np.float64))
    with pytest.raises(ValueError):
        vorticity.append(x[..., :3])


def _in_channels(gen, name):
    return tuple(gen.graph.variables[name].shape)[2]          # HWIO


def test_widened_variable_shapes(mpg):
    from mpgan_amd import multipass as MP
    for mode in (2, 1):
        g = MP.Generator("gen_resnet", dict(tile_low=8, up_res=4, channels=4, upsampling_mode=mode, vorticity=True), None, 3)
        side = 8 if mode == 2 else 32
        assert g.x.shape[1] == side * side * 7
        assert _in_channels(g, "generator/g_cA0/weight") == 7 and _in_channels(g, "generator/g_s0/weight") == 7
    plain = MP.Generator("gen_resnet", dict(tile_low=8, up_res=4, channels=4, upsampling_mode=2), None, 3)
    assert plain.x.shape[1] == 8 * 8 * 4 and _in_channels(plain, "generator/g_cA0/weight") == 4
    base = dict(tile_low=4, up_res=8, channels=4, filter_size=3, start_fms=32, max_fms=32)
    first = MP.Generator("growing_gen", dict(base, first_gen=True, add_adj=True, first_nn_arch=True, vorticity=True), None, 3)
    assert first.x.shape[1] == 4 * 4 * 9
    later = MP.Generator("growing_gen", dict(base, first_gen=False, vorticity=True), None, 3)
    assert later.x.shape[1] == 4 * 4 * 7
    assert _in_channels(first, "generator/genBlock2/g_cA_first/weight") == 9
    assert _in_channels(first, "generator/genBlock2/g_s_first/weight") == 9
    assert _in_channels(later, "generator/g_cA_1/weight") == 8    # the previous pass next to the 7 resized channels
    with pytest.raises(ValueError):
        MP.Generator("gen_resnet", dict(tile_low=8, up_res=4, channels=1, upsampling_mode=2, vorticity=True), None, 3)


class OracleGen(object):
    """callable with the Generator interface and its cfg, evaluated by the numpy oracle; keeps what it was fed"""

    def __init__(self, kind, seed, cfg):
        self.kind, self.cfg, self.ps, self.fed = kind, dict(cfg), ON.ParamSource(seed=seed), []

    def __call__(self, x, y=None):
        c = self.cfg
        xn = x.numpy()
        self.fed.append(xn.copy())
        if self.kind == "gen_resnet":
            out = ON.gen_resnet(self.ps, xn, c["up_res"], c["mode"], True)
        elif c["first_gen"]:
            out = ON.growing_gen(self.ps, xn, c["up_res"], True, 3, 32, 32, True, True)
        else:
            yin = y.numpy().reshape(xn.shape[0], y.shape[1], y.shape[2], 1)
            out = ON.growing_gen(self.ps, ON.gen2_input(yin, xn, yin.shape[1]), c["up_res"], False, 3, 32, 32, False, True)
        return torch.as_tensor(out[..., 0])


def _run(ps_seed, kind, cfg, x, y=None):
    g = OracleGen(kind, ps_seed, cfg)
    return g(torch.as_tensor(x), None if y is None else torch.as_tensor(y)).numpy()


def test_plane_pass_4x_feeds_the_vorticity(mpg):
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    import cpu_backend
    sim, up, vs = 4, 4, 0.5
    low = synthetic_volume(sim, 4, 3)
    cfg = dict(up_res=up, mode=2, vorticity=True)
    g = OracleGen("gen_resnet", 5, cfg)
    got = MP.plane_pass_4x(g, torch.as_tensor(low), up, batch=3, backend=cpu_backend, vel_scale=vs, apply_cutoff=False)
    xin = VR.plane_pass_4x_input(low, vs)
    assert xin.shape == (sim, sim, sim, 7) and np.count_nonzero(xin[..., 6]) > 0
    assert np.array_equal(np.concatenate(g.fed, axis=0), xin)
    want = np.concatenate([_run(5, "gen_resnet", cfg, xin[k:k + 3]) for k in range(0, sim, 3)], axis=0)
    assert np.array_equal(got.numpy(), want)
    # without the key nothing changes
    g4 = OracleGen("gen_resnet", 5, dict(up_res=up, mode=2))
    MP.plane_pass_4x(g4, torch.as_tensor(low), up, batch=8, backend=cpu_backend, vel_scale=vs)
    assert g4.fed[0].shape[-1] == 4


@pytest.mark.parametrize("mode", [1, 3])
def test_refine_pass_4x_feeds_the_vorticity(mpg, mode):
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    import cpu_backend
    sim, up, vs = 2, 4, 0.5
    s = sim * up
    low = synthetic_volume(sim, 4, 3)
    prev = np.random.default_rng(4).random((s, s, s)).astype(np.float32)
    cfg = dict(up_res=up, mode=1, vorticity=True)
    g = OracleGen("gen_resnet", 6, cfg)
    got = MP.refine_pass_4x(g, torch.as_tensor(low), torch.as_tensor(prev), up, mode=mode, batch=8, backend=cpu_backend,
                            vel_scale=vs, apply_cutoff=True)
    xin = VR.refine_pass_4x_input(low, prev, up, mode, vs)
    assert xin.shape == (s, s, s, 7)
    assert np.array_equal(np.concatenate(g.fed, axis=0), xin)
    out = _run(6, "gen_resnet", cfg, xin)
    want = OM.cutoff(np.ascontiguousarray(out.transpose((1, 2, 0) if mode == 1 else (1, 0, 2))), MP.CUTOFF)
    assert np.array_equal(got.numpy(), want)


def test_two_pass_4x_feeds_the_vorticity_in_both_passes(mpg):
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    import cpu_backend
    sim, up, vs = 2, 4, 0.5
    low = synthetic_volume(sim, 4, 3)
    c1, c2 = dict(up_res=up, mode=2, vorticity=True), dict(up_res=up, mode=1, vorticity=True)
    g1, g2 = OracleGen("gen_resnet", 5, c1), OracleGen("gen_resnet", 6, c2)
    final, v1 = MP.two_pass_4x(g1, g2, torch.as_tensor(low), up, batch=8, backend=cpu_backend, vel_scale=vs)
    x1 = VR.first_pass_4x_input(low, up, vs)
    assert np.array_equal(np.concatenate(g1.fed, axis=0), x1)
    want1 = OM.cutoff(_run(5, "gen_resnet", c1, x1), MP.CUTOFF)
    assert np.array_equal(v1.numpy(), want1)
    x2 = VR.refine_pass_4x_input(low, want1, up, 1, vs)
    assert np.array_equal(np.concatenate(g2.fed, axis=0), x2)
    want = OM.cutoff(np.ascontiguousarray(_run(6, "gen_resnet", c2, x2).transpose(1, 2, 0)), MP.CUTOFF)
    assert np.array_equal(final.numpy(), want)


def test_multipass_8x_feeds_the_vorticity(mpg):
    from mpgan_amd import multipass as MP
    from mpgan_amd.synthetic import synthetic_volume
    import cpu_backend
    sim, up = 2, 8
    low = synthetic_volume(sim, 4, 4)
    c1 = dict(up_res=up, first_gen=True, add_adj=True, vorticity=True)
    c2 = dict(up_res=up, first_gen=False, vorticity=True)
    g1, g2 = OracleGen("growing_gen", 7, c1), OracleGen("growing_gen", 8, c2)
    got = MP.multipass_8x([g1, g2], torch.as_tensor(low), up, batches=(16, 16, 16), backend=cpu_backend, apply_cutoff=False)
    x1 = VR.first_pass_8x_input(low, up, True)
    assert x1.shape == (sim * up, sim, sim, 9)
    assert np.array_equal(np.concatenate(g1.fed, axis=0), x1)
    out1 = _run(7, "growing_gen", c1, x1)
    x2 = VR.second_pass_8x_input(low, up)
    assert x2.shape == (sim * up, sim, sim, 7)
    assert np.array_equal(np.concatenate(g2.fed, axis=0), x2)
    out2 = _run(8, "growing_gen", c2, x2, np.ascontiguousarray(out1.transpose(2, 1, 0)))
    assert np.array_equal(got.numpy(), np.ascontiguousarray(out2.transpose(2, 1, 0)))
    # the single-network driver path takes the same first batch
    g1.fed = []
    one = MP.single_pass_8x(g1, torch.as_tensor(low), None, up, 0, batch=16, backend=cpu_backend, apply_cutoff=False)
    assert np.array_equal(np.concatenate(g1.fed, axis=0), x1) and np.array_equal(one.numpy(), out1)


def test_upsample_pass_4x_refuses_vorticity(mpg):
    from mpgan_amd import multipass as MP
    import cpu_backend
    g = OracleGen("gen_resnet", 6, dict(up_res=4, mode=0, vorticity=True))
    with pytest.raises(ValueError, match="vorticity"):
        MP.upsample_pass_4x(g, torch.zeros((4, 4, 4, 4)), torch.zeros((4, 16, 16)), 4, backend=cpu_backend)


def test_training_case_keeps_its_margin(mpg, monkeypatch):
    """the 7-channel Trainer4x case of test_vorticity_train_gpu.py: no ReLU or leaky-ReLU pre-activation of its float64
    oracle lies within 1e-5 of zero, so fp32-grade arithmetic (relative error ~1e-6 on pre-activations of order 1) takes
    the same side of every kink and the gradients can be compared at the bounds of the 4-channel test"""
    import vorticity_train_cases as VC
    from mpgan_amd.train import Trainer4x
    from oracle import train_ref as TR
    tr = Trainer4x(tileSizeLow=VC.TILE, upRes=4, n_inputChannels=VC.CHANNELS, batch_norm=True, device="cpu", seed=VC.SEED)
    _, p = VC.oracle_params(tr.graph.variables)
    xs, ys = VC.tiles_4x()
    assert xs.shape == (VC.BATCH, VC.TILE * VC.TILE * 7) and np.count_nonzero(xs.reshape(-1, 7)[:, 6]) > 0
    nearest, relu, lrelu = [], torch.relu, TR.lrelu

    def seen(x):
        nearest.append(float(x.detach().abs().min()))

    monkeypatch.setattr(torch, "relu", lambda x: (seen(x), relu(x))[1])
    monkeypatch.setattr(TR, "lrelu", lambda x, leak=0.2: (seen(x), lrelu(x, leak))[1])
    with torch.no_grad():
        TR.losses_4x(p, xs, ys, VC.TILE, 4, VC.CHANNELS, batch_norm=True)
    assert len(nearest) == 16                  # every activation of the generator and of the critic's passes was seen
    print("nearest pre-activation", min(nearest))
    assert min(nearest) > VC.MARGIN, nearest
