"""The column-only fused nearest upsample (mpg_conv_seg.up_x_only) and the 4x pipeline built on it, on the GPU.

Kernel tests: a launch with up_log2 = k, up_x_only = 1 on a source [N, H, W >> k] against the same launch with
up_log2 = 0 on that source expanded along W with repeat_interleave.  Every output is the same sum of the same numbers in
the same order -- only the addresses the source pixels are fetched from differ -- so the two results are equal bit for
bit (torch.equal on the fp32 output and on both planes of the G8 output).  Random fp32 data: non-zero lo planes, and no
two source columns alike, so that a shift applied to the wrong axis, or not applied, cannot go unnoticed.  The output is
19 x 40 (two tile columns of the matrix-core kernels, ragged in both axes; 19 is no multiple of any factor), N = 2.

Network, pipeline and driver tests: against oracle.nets.gen_resnet and the restatement axis_upsample_ref.py, with the
tolerances of test_nets_gpu.py.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import axis_upsample_ref as AR
import conv_exact_ref as R
from conftest import rel_l2
from oracle import nets as ON
from test_nets_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 19, 40
KS = (1, 2, 3)


def _t(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device=DEV)      # a copy: arrays read from files are read-only


def _source(seed, k, c, rows=H):
    """[N, rows, W >> k, c]: random values plus a ramp over the columns (every column differs from every other by more
    than the noise), and the tensor expanded to W columns"""
    rng = np.random.default_rng(seed)
    ws = W >> k
    x = rng.standard_normal((N, rows, ws, c)) * 0.25 + np.arange(1, ws + 1)[None, None, :, None] * 0.75
    x = _t(x.astype(np.float32))
    return x, x.repeat_interleave(1 << k, dim=2).contiguous()


def _weights(ops, seed, kh, kw, cin, cout, prec):
    w = np.random.default_rng(seed).standard_normal((kh, kw, cin, cout)).astype(np.float32)
    return ops.pack_conv_weights(_t(w), wscale=0.1, prec=prec)


def _same_bits(a, b, what):
    ya, ga = a
    yb, gb = b
    assert ya.shape == yb.shape and torch.isfinite(ya).all() and ya.abs().max() > 0, what
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), "%s: fp32 output differs in %d values" % (
        what, int((ya != yb).sum()))
    assert torch.equal(ga.buf.view(torch.int16), gb.buf.view(torch.int16)), what + ": G8 output differs"


def _launch(ops, segs, **kw):
    bias = _t(np.linspace(-0.5, 0.5, segs[0].packed.cout))
    return ops.conv2d_fused(segs, (H, W), bias=bias, act="relu", want_f32=True, want_g8=True, **kw)


# (kh, kw, cin, cout, precisions, the launch class the case is there for)
SINGLE = {
    "a: mfma image 5x5 16->32": (5, 5, 16, 32, (3, 1), dict(kernel="mfma", direct=0)),
    "a: mfma image 3x3 8->128": (3, 3, 8, 128, (3, 1), dict(kernel="mfma", nt=4)),
    "b: f6 image 5x5 16->32": (5, 5, 16, 32, (2,), dict(kernel="f6", direct=0)),
    "c: f6 direct 1x1 16->16": (1, 1, 16, 16, (2,), dict(kernel="f6", direct=1)),
    "d: small 5x5 4->8": (5, 5, 4, 8, (3, 2), dict(kernel="small")),
    "d: small 5x5 1->2": (5, 5, 1, 2, (3,), dict(kernel="small")),
}


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_one_segment(gpu_ops, name, k):
    ops = gpu_ops
    kh, kw, cin, cout, precs, cls = SINGLE[name]
    xs, xb = _source(k, k, cin)
    for prec in precs:
        lc = R.launch_class(kh, kw, cin, cout, prec)
        assert all(lc[f] == v for f, v in cls.items()), (name, prec, lc)
        pk = _weights(ops, 7, kh, kw, cin, cout, prec)
        flagged = _launch(ops, [ops.Segment(xs, pk, up_log2=k, up_x_only=1)])
        plain = _launch(ops, [ops.Segment(xb, pk)])
        _same_bits(flagged, plain, "%s, k %d, prec %d" % (name, k, prec))
        # the register-store epilogue of a G8-only launch reads the same sources
        g = ops.conv2d_fused([ops.Segment(xs, pk, up_log2=k, up_x_only=1)], (H, W), bias=_t(np.linspace(-0.5, 0.5, cout)),
                             act="relu", want_f32=False, want_g8=True)
        assert torch.equal(g.buf.view(torch.int16), plain[1].buf.view(torch.int16))


@pytest.mark.parametrize("k", KS)
def test_small_pair(gpu_ops, k):
    """e: 1 -> 2 -> 8 with the 1x1 shortcut as one launch (resBlock 0 of the density-only mode-0 generator)"""
    ops = gpu_ops
    xs, xb = _source(10 + k, k, 1)
    for prec in (3, 2):
        pa, pb, ps = _weights(ops, 1, 5, 5, 1, 2, prec), _weights(ops, 2, 5, 5, 2, 8, prec), _weights(ops, 3, 1, 1, 1, 8, prec)
        ba, bb = _t(np.array([0.1, -0.2])), _t(np.linspace(-0.3, 0.3, 8))
        kw = dict(bias_a=ba, act_a="relu", bias_b=bb, act_b="relu", want_f32=True, want_g8=True)
        flagged = ops.conv2d_small_pair(xs, 0, k, pa, pb, ps, (H, W), up_x_only=1, **kw)
        plain = ops.conv2d_small_pair(xb, 0, 0, pa, pb, ps, (H, W), **kw)
        _same_bits(flagged, plain, "small pair, k %d, prec %d" % (k, prec))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("prec", [3, 2, 1])
def test_two_segments(gpu_ops, prec, k):
    """f: both segments flagged; g: a full-resolution 5x5 segment and a flagged 1x1 shortcut, what the second launch of a
    mode-0 resBlock 0 runs; in both orders"""
    ops = gpu_ops
    xs, xb = _source(20 + k, k, 16)
    ys, yb = _source(30 + k, k, 24)
    full = _source(40 + k, 0, 16)[0]
    p5, p1, p3 = _weights(ops, 4, 5, 5, 16, 40, prec), _weights(ops, 5, 1, 1, 24, 40, prec), _weights(ops, 6, 3, 3, 16, 40, prec)
    f = _launch(ops, [ops.Segment(xs, p5, up_log2=k, up_x_only=1), ops.Segment(ys, p1, up_log2=k, up_x_only=1)])
    _same_bits(f, _launch(ops, [ops.Segment(xb, p5), ops.Segment(yb, p1)]), "f, k %d, prec %d" % (k, prec))
    for order in (0, 1):
        segs = [ops.Segment(full, p3), ops.Segment(ys, p1, up_log2=k, up_x_only=1)]
        ref = [ops.Segment(full, p3), ops.Segment(yb, p1)]
        g = _launch(ops, segs[::-1] if order else segs)
        _same_bits(g, _launch(ops, ref[::-1] if order else ref), "g, k %d, prec %d, order %d" % (k, prec, order))


def test_both_axes_and_columns_only_in_one_launch(gpu_ops):
    """a segment upsampled in both axes next to one upsampled in its columns only (H = 20 here: both factors divide it)"""
    ops = gpu_ops
    rng = np.random.default_rng(50)
    h = 20
    a = _t(rng.standard_normal((N, h // 2, W // 2, 16)).astype(np.float32))
    b = _t(rng.standard_normal((N, h, W // 4, 16)).astype(np.float32))
    for prec in (3, 2):
        pa, pb = _weights(ops, 8, 3, 3, 16, 32, prec), _weights(ops, 9, 1, 1, 16, 32, prec)
        got = ops.conv2d_fused([ops.Segment(a, pa, up_log2=1), ops.Segment(b, pb, up_log2=2, up_x_only=1)], (h, W))
        want = ops.conv2d_fused([ops.Segment(a.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous(), pa),
                                 ops.Segment(b.repeat_interleave(4, 2).contiguous(), pb)], (h, W))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("k", KS)
def test_window_and_depth_to_space_launches(gpu_ops, k):
    """h: mpg_conv2d_fused_window (two windows of a 80-channel tensor) and mpg_conv2d_fused_d2s go through the same
    segment code"""
    ops = gpu_ops
    xs, xb = _source(60 + k, k, 16)
    for prec in (3, 2):
        pks = [_weights(ops, 11 + i, 3, 3, 16, 40, prec) for i in range(2)]
        bias = _t(np.linspace(-0.5, 0.5, 80))
        kw = dict(bias=bias, act="relu", want_f32=True, want_g8=True)
        flagged = ops.conv2d_fused_wide([([ops.Segment(xs, p, up_log2=k, up_x_only=1)], 40 * i) for i, p in enumerate(pks)],
                                        (H, W), 80, **kw)
        plain = ops.conv2d_fused_wide([([ops.Segment(xb, p)], 40 * i) for i, p in enumerate(pks)], (H, W), 80, **kw)
        _same_bits(flagged, plain, "window, k %d, prec %d" % (k, prec))
    pk = _weights(ops, 13, 1, 1, 16, 32, 3)
    flagged = ops.conv2d_fused_d2s([([ops.Segment(xs, pk, up_log2=k, up_x_only=1)], 0)], (H, W), 32, want_f32=True, want_g8=True)
    plain = ops.conv2d_fused_d2s([([ops.Segment(xb, pk)], 0)], (H, W), 32, want_f32=True, want_g8=True)
    _same_bits(flagged, plain, "depth to space, k %d" % k)


def test_error_paths(gpu_ops, mpg):
    from mpgan_amd import _lib
    ops = gpu_ops
    xs, _ = _source(70, 1, 16)
    small, _ = _source(71, 1, 1)
    pk = _weights(ops, 14, 3, 3, 16, 32, 3)
    pa, pb = _weights(ops, 1, 5, 5, 1, 2, 3), _weights(ops, 2, 5, 5, 2, 8, 3)
    # any flag but 0 and 1: MPG_ERR_ARG (1), on the matrix-core route, the small-channel route and the pair launch
    with pytest.raises(_lib.MpgError, match=r"failed \(1\).*up_x_only"):
        ops.conv2d_fused([ops.Segment(xs, pk, up_log2=1, up_x_only=2)], (H, W))
    with pytest.raises(_lib.MpgError, match=r"failed \(1\).*up_x_only"):
        ops.conv2d_fused([ops.Segment(small, pa, up_log2=1, up_x_only=2)], (H, W))
    with pytest.raises(_lib.MpgError, match=r"failed \(1\).*up_x_only"):
        ops.conv2d_small_pair(small, 0, 1, pa, pb, None, (H, W), up_x_only=2)
    with pytest.raises(_lib.MpgError, match=r"failed \(1\).*up_x_only"):
        ops.conv2d_fused([ops.Segment(xs, pk, up_log2=1, up_x_only=-1)], (H, W))
    # a width the factor does not divide: refused by the library itself (the Python shape check is bypassed by
    # handing it the descriptor of a valid launch with the width changed)
    d = ops._conv_desc([ops.Segment(xs, pk, up_log2=1, up_x_only=1)], (H, W), None, None, 0.2)
    y = torch.empty((N, H, W, 32), dtype=torch.float32, device=DEV)
    d.y, d.w = y.data_ptr(), W - 1
    assert _lib.load().mpg_conv2d_fused(None, ctypes.byref(d)) == 1          # MPG_ERR_ARG, nothing launched
    with pytest.raises(_lib.MpgError):
        ops.conv2d_fused([ops.Segment(xs, pk, up_log2=1, up_x_only=1)], (H, W - 1))
    with pytest.raises(_lib.MpgError):
        ops.conv2d_small_pair(small, 0, 1, pa, pb, None, (H, W + 1), up_x_only=1)
    # 19 rows: only the flag makes a factor of 2 acceptable
    ops.conv2d_fused([ops.Segment(xs, pk, up_log2=1, up_x_only=1)], (H, W))
    d = ops._conv_desc([ops.Segment(xs, pk, up_log2=1, up_x_only=1)], (H, W), None, None, 0.2)
    d.y = y.data_ptr()
    d.seg[0].up_x_only = 0
    assert _lib.load().mpg_conv2d_fused(None, ctypes.byref(d)) == 1
    ops.conv2d_small_pair(small, 0, 1, pa, pb, None, (H, W), up_x_only=1)


# ---- the network -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def MP(mpg):
    from mpgan_amd import multipass
    return multipass


@pytest.mark.parametrize("prec", [3, 2, 1])
@pytest.mark.parametrize("nch", [1, 4])
def test_gen_resnet_mode0(MP, prec, nch):
    low, up = 8, 4
    x = np.random.default_rng(nch * 10).random((3, low * up, low, nch)).astype(np.float32)
    ps = ON.ParamSource(seed=5)
    ref = ON.gen_resnet(ps, x, up, 0, True)[..., 0]
    gen = MP.Generator("gen_resnet", dict(tile_low=low, up_res=up, channels=nch, upsampling_mode=0, batch_norm=True),
                       params=ps.params, prec=prec)
    assert sorted(gen.graph.variables) == sorted(ps.params)
    assert "resize" not in [e["kind"] for e in gen.sess.plan_summary(gen.sampler)]
    y = gen(_t(x)).cpu().numpy()
    err = rel_l2(y, ref)
    print("gen_resnet mode 0, C %d, prec %d: rel L2 %.3e" % (nch, prec, err))
    assert y.shape == (3, 32, 32) and err < TOL[prec]


# ---- the pipeline ----------------------------------------------------------------------------------------------------
SEEDS = (23, 22)         # both reference volumes keep > 80 % of their voxels above the cutoff (checked below)


@pytest.fixture(scope="module")
def pipeline_refs():
    from mpgan_amd.synthetic import synthetic_volume
    refs = {}
    for nch in (1, 4):
        low = synthetic_volume(8, nch, 0)
        vs = 0.7 if nch > 1 else 1.0
        ps1, ps0 = ON.ParamSource(seed=SEEDS[0]), ON.ParamSource(seed=SEEDS[1])
        final, v1 = AR.two_pass(ps1, ps0, low, 4, vs)
        refs[nch] = (low, vs, ps1.params, ps0.params, final, v1)
    return refs


@pytest.mark.parametrize("nch", [1, 4])
def test_pipeline_reference_is_not_mostly_cut_off(pipeline_refs, nch):
    """at least half of the voxels of both reference volumes survive the 5e-4 cutoff: the comparison below is about values"""
    _, _, _, _, final, v1 = pipeline_refs[nch]
    assert final.shape == (32, 32, 32) and v1.shape == (8, 32, 32)
    assert np.count_nonzero(final) >= final.size // 2 and np.count_nonzero(v1) >= v1.size // 2


@pytest.mark.parametrize("prec", [3, 2])
@pytest.mark.parametrize("nch", [1, 4])
def test_two_pass_4x_axis(MP, pipeline_refs, prec, nch):
    low, vs, p1, p0, ref, ref1 = pipeline_refs[nch]
    g1 = MP.Generator("gen_resnet", dict(tile_low=8, up_res=4, channels=nch, upsampling_mode=2), p1, prec)
    g0 = MP.Generator("gen_resnet", dict(tile_low=8, up_res=4, channels=nch, upsampling_mode=0), p0, prec)
    out, v1 = MP.two_pass_4x_axis(g1, g0, _t(low), 4, batch=8, vel_scale=vs)
    e1, e = rel_l2(v1.cpu().numpy(), ref1), rel_l2(out.cpu().numpy(), ref)
    print("two_pass_4x_axis C %d prec %d: rel L2 pass 1 %.3e, final %.3e" % (nch, prec, e1, e))
    assert out.shape == (32, 32, 32) and v1.shape == (8, 32, 32)
    assert e1 < TOL[prec] and e < TOL[prec]
    # a ragged batch gives the same volume
    out2, _ = MP.two_pass_4x_axis(g1, g0, _t(low), 4, batch=5, vel_scale=vs)
    assert torch.equal(out2, out)


# ---- the driver ------------------------------------------------------------------------------------------------------
def _run(args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", "multipassGAN-4x.py")] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("vel", [0, 1])
def test_driver_two_invocations(MP, tmp_path, vel):
    from mpgan_amd import ops, uniio
    from mpgan_amd.synthetic import synthetic_volume
    sim, up = 8, 4
    d = tmp_path / "data" / "sim_1005"
    d.mkdir(parents=True)
    v = synthetic_volume(sim, 4, 0)
    uniio.writeUni(str(d / "density_low_0000.uni"), uniio.make_header(sim, sim, sim), v[..., 0:1])
    if vel:
        uniio.writeUni(str(d / "velocity_low_0000.uni"), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
    for t in ("test_0004", "test_0048"):
        (tmp_path / "models" / t).mkdir(parents=True)
    common = ["upRes", up, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
              "useVelocities", vel, "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/",
              "frame_min", 0, "frame_max", 1, "genUni", 1, "velScale", 0.7, "synthWeights", 1, "genModel", "gen_resnet"]
    _run(common + ["randSeed", 101, "load_model_test", 4, "load_model_no", 1199, "upsamplingMode", 2, "upsampledData", 0,
                   "upsampleFirst", 0], str(tmp_path))
    _run(common + ["randSeed", 102, "load_model_test", 48, "load_model_no", 799, "upsamplingMode", 0, "upsampledData", 1],
         str(tmp_path))
    h1, f1 = uniio.readUni(str(d / "density_low_2x2x1_0000.uni"))
    h0, f0 = uniio.readUni(str(d / "density_low_1x1x1_0000.uni"))
    assert (h1["dimX"], h1["dimY"], h1["dimZ"]) == (32, 32, 8) and f1.shape == (8, 32, 32, 1)
    assert (h0["dimX"], h0["dimY"], h0["dimZ"]) == (32, 32, 32) and f0.shape == (32, 32, 32, 1)
    # the library calls on the same input: what the loader hands the driver, the driver's generators
    nch = 4 if vel else 1
    low = _t(v if vel else v[..., 0:1])
    prec = ops.parse_prec("2")
    g1 = MP.Generator("gen_resnet", dict(tile_low=sim, up_res=up, channels=nch, upsampling_mode=2, batch_norm=True), None, prec, seed=101)
    g0 = MP.Generator("gen_resnet", dict(tile_low=sim, up_res=up, channels=nch, upsampling_mode=0, batch_norm=True), None, prec, seed=102)
    want1 = MP.plane_pass_4x(g1, low, up, batch=8, vel_scale=0.7)
    assert np.array_equal(f1[..., 0], want1.cpu().numpy())
    want0 = MP.upsample_pass_4x(g0, low, _t(f1[..., 0]), up, batch=8, vel_scale=0.7)
    assert np.array_equal(f0[..., 0], want0.cpu().numpy())
    assert np.count_nonzero(f0) > 0
