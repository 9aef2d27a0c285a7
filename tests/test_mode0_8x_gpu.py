"""8x upsamplingMode 0 on the GPU: mpg_bicubic_cols_add, the launch plan of the mode-0 growing generator, the generator,
the two-pass pipeline and the driver, against the float64 restatement upsample_mode0_8x_ref.py.

mpg_bicubic_cols_add, bound.  test_elem_gpu.py::test_resize_bicubic_bounded holds mpg_resize_bicubic to the oracle within
elem_ref.bicubic_bound = SLACK * 40 U (sum |wy|) (sum |wx|) max |tap| + TINY elementwise; the same array, taken for the
source channel at [h, wl * f] (sum |wy| = 1 at row scale 1), bounds this kernel.  Its output carries one rounding more,
that of dens + cols, worth U / 2 (|dens| + |cols|).  The data keep that inside the same bound by construction and not by
a wider one: |src| in [0.5, 1.5], so max |tap| >= 0.5, and |dens| <= 1 <= 2 (sum |wx|) max |tap|; with |cols| <= (sum |wx|)
max |tap| the extra rounding is at most 1.5 U (sum |wx|) max |tap|, and the four products, three adds and the weights'
2 ulp of the four-tap sum stay below 10 U (sum |wx|) max |tap| by the counting of bicubic_bound's docstring.
Small integers (|src| <= 8, integer dens): the weights at factors 2, 4, 8 are dyadic with at most 11 fraction bits, every
product and sum is exact, and the result equals the restatement bit for bit.

Generator, pipeline: rel L2 below TOL[prec] of test_nets_gpu.py (3: 1e-4, 2: 5e-4, 1: 5e-3), the tolerance of the existing
8x generator parity tests (test_nets_gpu.py::test_growing_gen) and of test_wide_conv_gpu.py (3: 1e-4, 2: 5e-4).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import elem_ref as R
import upsample_mode0_8x_ref as MR
from conftest import rel_l2
from oracle import nets as ON
from test_nets_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
N, H, C = 2, 5, 5
PAD = 64                                   # floats of NaN sentinel on either side of the output (256 bytes)
NARROW = dict(filter_size=3, start_fms=32, max_fms=16, use_res_net=True)


def _t(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device=DEV)


@pytest.fixture(scope="module")
def MP(mpg):
    from mpgan_amd import multipass
    return multipass


# ---- mpg_bicubic_cols_add --------------------------------------------------------------------------------------------
def _between_sentinels(total, shift):
    """a [total] view `shift` floats past a 16-byte boundary inside a buffer of NaNs, and the buffer"""
    buf = torch.full((PAD + shift + total + PAD,), float("nan"), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[PAD + shift:PAD + shift + total], buf


def _shifted(a, shift):
    """the array on the GPU, its first element `shift` floats past a 16-byte boundary"""
    flat = torch.zeros(a.size + shift, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    flat[shift:] = _t(a).reshape(-1)
    return flat[shift:].view(*a.shape)


def _run_kernel(ops, src, c_src, f, dens, shifts):
    """(result, the NaN zones untouched?) of one launch with the source / dens / out pointers shifted by `shifts` floats"""
    total = dens.size
    out, buf = _between_sentinels(total, shifts[2])
    got = ops.bicubic_cols_add(_shifted(src, shifts[0]), c_src, f, _shifted(dens, shifts[1]), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == dens.shape
    lo, hi = buf[:PAD + shifts[2]], buf[PAD + shifts[2] + total:]
    return got.cpu().numpy(), bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())


# (source, dens, out) shifts in floats: all aligned; the source one float off (scalar loads either way); dens or out off a
# 16-byte boundary (the scalar kernel)
SHIFTS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 3)]


@pytest.mark.parametrize("f", [2, 4, 8])
@pytest.mark.parametrize("c_src", [0, 4])
@pytest.mark.parametrize("wl", [3, 8])
def test_bicubic_cols_add(gpu_ops, wl, c_src, f):
    """wl 3, f 2: rows of 6 floats, no multiple of 4 -> the scalar kernel whatever the alignment; every other case runs
    the 16-byte kernel when dens and out are aligned"""
    ops = gpu_ops
    rng = np.random.default_rng(100 * wl + 10 * c_src + f)
    wo = wl * f
    src = (rng.uniform(0.5, 1.5, (N, H, wl, C)) * rng.choice([-1.0, 1.0], (N, H, wl, C))).astype(F32)
    dens = rng.uniform(-1.0, 1.0, (N, H, wo, 1)).astype(F32)
    want = MR.bicubic_cols_add(src, c_src, f, dens)
    bound = R.bicubic_bound(src[..., c_src:c_src + 1], H, wo)
    ints = rng.integers(-8, 9, (N, H, wl, C)).astype(F32)
    idens = rng.integers(-64, 65, (N, H, wo, 1)).astype(F32)
    iwant = MR.bicubic_cols_add(ints, c_src, f, idens)
    assert np.array_equal(iwant.astype(F32).astype(np.float64), iwant)           # representable: nothing to round
    for shifts in SHIFTS:
        name = "bicubic_cols_add wl %d c_src %d f %d shifts %s" % (wl, c_src, f, shifts)
        got, clean = _run_kernel(ops, src, c_src, f, dens, shifts)
        assert not np.isnan(got).any(), name + ": elements left unwritten"
        assert clean, name + ": wrote outside the output"
        ratio = R.worst(got, want, bound)
        print("elem-error %-58s %.3f" % (name, ratio))
        assert ratio <= 1.0, name
        again, _ = _run_kernel(ops, src, c_src, f, dens, shifts)
        assert np.array_equal(got.view(np.int32), again.view(np.int32)), name + ": two runs differ"
        igot, clean = _run_kernel(ops, ints, c_src, f, idens, shifts)
        assert clean and np.array_equal(igot.view(np.int32), iwant.astype(F32).view(np.int32)), name + ": integers"


def test_bicubic_cols_add_more_than_one_block_and_the_unfused_composition(gpu_ops):
    """[2, 67, 24 * 4]: 3216 four-wide units, more than one block; the composition slice, mpg_resize_bicubic, add stays
    within twice the bound of the kernel (its sixteen-term sum may round differently: no bit equality asked)"""
    ops = gpu_ops
    rng = np.random.default_rng(7)
    n, h, wl, f = 2, 67, 24, 4
    src = (rng.uniform(0.5, 1.5, (n, h, wl, C)) * rng.choice([-1.0, 1.0], (n, h, wl, C))).astype(F32)
    dens = rng.uniform(-1.0, 1.0, (n, h, wl * f, 1)).astype(F32)
    got = ops.bicubic_cols_add(_t(src), 4, f, _t(dens)).cpu().numpy()
    want = MR.bicubic_cols_add(src, 4, f, dens)
    bound = R.bicubic_bound(src[..., 4:5], h, wl * f)
    assert R.worst(got, want, bound) <= 1.0
    unfused = ops.add_act(ops.resize_bicubic(_t(src)[..., 4:5].contiguous(), h, wl * f), _t(dens)).cpu().numpy()
    assert R.worst(unfused, got, 2 * bound) <= 1.0


def test_bicubic_cols_add_refusals(gpu_ops):
    from mpgan_amd import _lib
    ops = gpu_ops
    src, dens = torch.zeros((1, 2, 3, 5), device=DEV), torch.zeros((1, 2, 6, 1), device=DEV)
    for c_src, f, d in ((5, 2, dens), (-1, 2, dens), (0, 3, torch.zeros((1, 2, 9, 1), device=DEV)),
                        (0, 128, torch.zeros((1, 2, 384, 1), device=DEV))):
        with pytest.raises(_lib.MpgError, match=r"mpg_bicubic_cols_add failed \(1\)"):
            ops.bicubic_cols_add(src, c_src, f, d)
        assert not ops.bicubic_cols_add_ok(src.shape, c_src, f)
    with pytest.raises(_lib.MpgError, match="a buffer of its own"):
        ops.bicubic_cols_add(src, 0, 2, dens, out=dens)
    with pytest.raises(_lib.MpgError, match="dens"):
        ops.bicubic_cols_add(src, 0, 2, torch.zeros((1, 2, 5, 1), device=DEV))
    assert ops.bicubic_cols_add_ok(src.shape, 4, 8)


# ---- planner ---------------------------------------------------------------------------------------------------------
def _mode0_gen(MP, low, prec, params=None, **kw):
    cfg = dict(tile_low=low, up_res=8, channels=4, upsampling_mode=0, **NARROW)
    cfg.update(kw)
    return MP.Generator("growing_gen", cfg, params, prec=prec)


def test_block_launches_are_bit_equal_to_host_expanded_input(gpu_ops):
    """the first unit of a default-width block as the plan runs it: convA 128 -> 256 (two channel windows, pixel norm) on the
    G8 source through up_log2 = 1, up_x_only = 1, then convB 256 -> 256 with the flagged 1x1 shortcut as second segment;
    against the same launches on the source expanded along the columns on the host.  Same sums in the same order, so equal
    bit for bit, as test_axis_upsample_gpu.py asks of the launches of the 4x case."""
    ops = gpu_ops
    rng = np.random.default_rng(9)
    n, h, w = 1, 9, 12
    xs = _t(rng.standard_normal((n, h, w // 2, 128)) * 0.5)
    xb = xs.repeat_interleave(2, dim=2).contiguous()
    for prec in (3, 2):
        wins = ops.wide_chunks(256)
        # the planner's own condition for an F16F6 launch (Session._launch_prec); these shapes are the default-width ones
        assert prec != 2 or ops.f6_available(wins[0][1], [(3, 3, 128), (3, 3, 256), (1, 1, 128)])

        def pk(seed, k, cin):
            wt = _t(np.random.default_rng(seed).standard_normal((k, k, cin, 256)))
            return [ops.pack_conv_weights(wt[..., co:co + cw].contiguous(), wscale=0.03, prec=prec) for co, cw in wins]

        pa, pb, psc = pk(1, 3, 128), pk(2, 3, 256), pk(3, 1, 128)
        bias = _t(np.linspace(-0.2, 0.2, 256))
        res = []
        for src, flag in ((xs, dict(up_log2=1, up_x_only=1)), (xb, {})):
            a = ops.conv2d_fused_wide([([ops.Segment(src, p, **flag)], co) for p, (co, _) in zip(pa, wins)], (h, w), 256,
                                      bias=bias, act="relu", pixel_norm=True, want_f32=False, want_g8=True)
            b = ops.conv2d_fused_wide([([ops.Segment(a, p), ops.Segment(src, q, **flag)], co)
                                       for p, q, (co, _) in zip(pb, psc, wins)], (h, w), 256, bias=bias, act="relu",
                                      pixel_norm=True, want_f32=True, want_g8=True)
            res.append((a, b))
        (a0, (y0, g0)), (a1, (y1, g1)) = res
        assert torch.equal(a0.buf.view(torch.int16), a1.buf.view(torch.int16)), "convA, prec %d" % prec
        assert torch.isfinite(y0).all() and y0.abs().max() > 0
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)), "convB + shortcut, prec %d" % prec
        assert torch.equal(g0.buf.view(torch.int16), g1.buf.view(torch.int16))


@pytest.mark.parametrize("prec", [3, 2, 1])
@pytest.mark.parametrize("widths", [(32, 16), (512, 256)])
def test_plan_and_network_against_standalone_depools(MP, monkeypatch, prec, widths):
    """start_fms 32 / max_fms 16 on two planes and one default-width network (512 / 256, tileSizeLow 4, one plane): the plan
    shows up_log2 = 1, up_x_only = 1 on the first unit of every block, no resize step and the residual kernel; and the
    output agrees with the same weights in a session whose planner cannot fuse the depools, so that every block reads a
    tensor that mpg_resize_nearest expanded and the residual runs as slice, mpg_resize_bicubic and post-add"""
    from mpgan_amd import session
    low, planes = 4, (2 if widths[0] == 32 else 1)
    g = _mode0_gen(MP, low, prec, start_fms=widths[0], max_fms=widths[1])
    plan = g.sess.plan_summary(g.sampler)
    kinds = [e["kind"] for e in plan]
    assert "resize" not in kinds and kinds.count("bicubic_cols_add") == 1
    up = sorted((s["weight"], s["up_log2"], s.get("up_x_only", 0)) for e in plan if "segments" in e for s in e["segments"]
                if s["up_log2"])
    assert up == sorted(("generator/genBlock%d/g_%s_first/weight" % (b, t), 1, 1) for b in (2, 4, 8) for t in ("cA", "s"))
    x = np.random.default_rng(3).standard_normal((planes, 32, low, 5)).astype(F32)
    y = g(_t(x))
    # the comparison session: no power-of-two factor is recognised, no column residual either
    plain = _mode0_gen(MP, low, prec, params=g.params(), start_fms=widths[0], max_fms=widths[1])
    monkeypatch.setattr(session, "_is_pow2", lambda v: False)
    monkeypatch.setattr(session.Session, "_cols_residual", staticmethod(lambda n: None))
    kinds2 = [e["kind"] for e in plain.sess.plan_summary(plain.sampler)]
    assert kinds2.count("resize") == 4 and "bicubic_cols_add" not in kinds2     # three depools and the bicubic residual
    y2 = plain(_t(x))
    monkeypatch.undo()
    err = rel_l2(y.cpu().numpy(), y2.cpu().numpy())
    print("mode-0 8x generator %s prec %d: fused plan against standalone depools rel L2 %.3e" % (widths, prec, err))
    assert y.shape == (planes, 32, 32) and torch.isfinite(y).all() and err < TOL[prec]


# ---- generator against the restatement ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gen_ref(low, use_res_net, widths):
    """(input, parameters, float64-restatement output) of one generator case, computed once for every prec"""
    x = np.random.default_rng(low).standard_normal((2, low * 8, low, 5)).astype(F32)
    ps = ON.ParamSource(seed=11)
    ref = MR.growing_gen_mode0(ps, x, 8, filter_size=3, start_fms=widths[0], max_fms=widths[1], use_res_net=use_res_net)
    return x, ps.params, ref[..., 0]


# Which networks a parity tolerance means something on.  The widths are this file's choice; TOL comes from
# test_nets_gpu.py::test_growing_gen, which runs networks 96 to 256 channels wide.
#  * A residual unit ends in relu and pixel norm.  With start_fms 32 / max_fms 16 the stem's first unit and the last block's
#    second unit are 2 channels wide: where both pre-activations lie below zero the restatement's pixel is exactly 0, and an
#    error that lifts one of them above zero by d comes out as d * rsqrt(d^2 / 2 + 1e-8), up to 1.41 at d = 1e-3 and a gain
#    of 1e4 below 1e-4.  One such pixel of planes 64x8 (restatement 0.0, every plane of the plan 1.27, the fused plan and the
#    plan with standalone depools alike, the unit before it at 6.8e-6) puts the output 6e-3 off at prec 3.  No tolerance is
#    meaningful there, so the residual units run at 192 / 192 (no pixel norm under 12 channels), the widths of that test's
#    second network.  The 32 / 16 network stays with use_res_net 0: lrelu never zeroes a pixel, and its narrowest norm has 4
#    channels.
#  * MPG_PREC_F16X1 rounds every convolution input to one fp16.  On the 32 / 16 network the FORMAT misses TOL[1] = 5e-3,
#    whatever computes it: the restatement with its convolution inputs rounded to fp16 in numpy is 1.8e-2 (planes 32x4) and
#    3.3e-2 (64x8) off the float64 one; on 192 / 192 it is 7e-4 to 1e-3.  So prec 1 runs at 192 / 192 only.
GEN_CASES = [((192, 192), rn, p) for rn in (True, False) for p in (3, 2, 1)] + [((32, 16), False, p) for p in (3, 2)]


@pytest.mark.parametrize("widths,use_res_net,prec", GEN_CASES)
@pytest.mark.parametrize("low", [4, 8])
def test_growing_gen_mode0(MP, low, widths, use_res_net, prec):
    high = low * 8
    x, params, ref = _gen_ref(low, use_res_net, widths)
    gen = _mode0_gen(MP, low, prec, params=params, use_res_net=use_res_net, start_fms=widths[0], max_fms=widths[1])
    assert sorted(gen.graph.variables) == sorted(params)
    y = gen(_t(x)).cpu().numpy()
    err = rel_l2(y, ref)
    print("growing_gen mode 0, planes %dx%d, widths %s, use_res_net %d, prec %d: rel L2 %.3e" % (
        high, low, widths, use_res_net, prec, err))
    assert y.shape == (2, high, high) and err < TOL[prec]


# ---- pipeline ----------------------------------------------------------------------------------------------------
# both networks 192 / 192 with residual units (see GEN_CASES: the widths at which TOL holds).  The seeds are the first pair
# from 31 / 32 upwards whose RESTATEMENT keeps most of the final volume above the storage cutoff (31 / 32: 1.4 %, 33: none,
# 34: 9 %, 35: 69 %, 36: all but 66 voxels): the comparison is about values, checked below
WIDE = dict(filter_size=3, start_fms=192, max_fms=192, use_res_net=True)
CFG1 = dict(WIDE, first_nn_arch=False)
SEEDS = (31, 36)


@pytest.fixture(scope="module")
def pipeline_ref():
    from mpgan_amd.synthetic import synthetic_volume
    low = synthetic_volume(8, 4, 0)
    ps1, ps0 = ON.ParamSource(seed=SEEDS[0]), ON.ParamSource(seed=SEEDS[1])
    final, v1 = MR.two_pass(ps1, ps0, CFG1, WIDE, low, 8, 0)
    return low, ps1.params, ps0.params, final, v1


def _gens(MP, prec, p1=None, p0=None, seeds=(None, None), widths=WIDE):
    kw1 = {} if seeds[0] is None else dict(seed=seeds[0])
    kw0 = {} if seeds[1] is None else dict(seed=seeds[1])
    g1 = MP.Generator("growing_gen", dict(tile_low=8, up_res=8, channels=4, first_gen=True, first_nn_arch=False, **widths),
                      p1, prec, **kw1)
    g0 = MP.Generator("growing_gen", dict(tile_low=8, up_res=8, channels=4, upsampling_mode=0, **widths), p0, prec, **kw0)
    return g1, g0


def test_pipeline_reference_is_not_mostly_cut_off(pipeline_ref):
    """at least half of the voxels of both reference volumes survive the 5e-4 cutoff"""
    _, _, _, final, v1 = pipeline_ref
    assert final.shape == (64, 64, 64) and v1.shape == (8, 64, 64)
    assert np.count_nonzero(final) >= final.size // 2 and np.count_nonzero(v1) >= v1.size // 2


@pytest.mark.parametrize("prec", [3, 2])
def test_two_pass_8x_axis(MP, pipeline_ref, prec):
    """8^3 -> 64^3 through both passes against the restatement; single_pass_8x through .uni files gives the same bits"""
    low, p1, p0, ref, ref1 = pipeline_ref
    assert ref.shape == (64, 64, 64) and ref1.shape == (8, 64, 64)
    g1, g0 = _gens(MP, prec, p1, p0)
    out, v1 = MP.two_pass_8x_axis(g1, g0, _t(low), 8, batches=(2, 2))
    e1, e = rel_l2(v1.cpu().numpy(), ref1), rel_l2(out.cpu().numpy(), ref)
    print("two_pass_8x_axis prec %d: rel L2 pass 1 %.3e, final %.3e; voxels above the cutoff %d / %d" % (
        prec, e1, e, np.count_nonzero(ref), ref.size))
    assert out.shape == (64, 64, 64) and v1.shape == (8, 64, 64)
    assert e1 < TOL[prec] and e < TOL[prec]
    # a ragged batch gives the same volume
    out2, _ = MP.two_pass_8x_axis(g1, g0, _t(low), 8, batches=(3, 5))
    assert torch.equal(out2, out)


def test_single_pass_through_files_equals_the_pipeline(MP, pipeline_ref, tmp_path):
    from mpgan_amd import uniio
    low, p1, p0, _, _ = pipeline_ref
    g1, g0 = _gens(MP, 2, p1, p0)
    out, v1 = MP.two_pass_8x_axis(g1, g0, _t(low), 8)
    a = MP.single_pass_8x(g1, _t(low), None, 8, 0, upsample_first=False)
    uniio.writeUni(str(tmp_path / "a.uni"), uniio.make_header(64, 64, 8), a.cpu().numpy().reshape(8, 64, 64, 1))
    _, back = uniio.readUni(str(tmp_path / "a.uni"))
    assert back.shape == (8, 64, 64, 1) and np.array_equal(back[..., 0], v1.cpu().numpy())
    b = MP.single_pass_8x(g0, _t(low), _t(back[..., 0]), 8, 0)
    assert torch.equal(b, out)
    # transposeAxis 2 stores [z, y, x]
    b2 = MP.single_pass_8x(g0, _t(low), _t(back[..., 0]), 8, 2)
    assert torch.equal(b2, out.permute(2, 1, 0))


# ---- driver ----------------------------------------------------------------------------------------------------------
def _run(args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", "multipassGAN-8x.py")] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_driver_two_invocations(MP, tmp_path):
    import glob
    from mpgan_amd import ops, uniio
    from mpgan_amd.synthetic import synthetic_volume
    sim, up = 8, 8
    s = sim * up
    d = tmp_path / "data" / "sim_1005"
    d.mkdir(parents=True)
    v = synthetic_volume(sim, 4, 0)
    uniio.writeUni(str(d / "density_low_0000.uni"), uniio.make_header(sim, sim, sim), v[..., 0:1])
    uniio.writeUni(str(d / "velocity_low_0000.uni"), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
    (tmp_path / "models").mkdir()
    common = ["upRes", up, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
              "useVelocities", 1, "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/",
              "frame_min", 0, "frame_max", 1, "genUni", 1, "velScale", 0.7, "synthWeights", 1, "startFms", 32, "maxFms", 16,
              "filterSize", 3, "use_res_net", 1, "addBicubicUpsample", 1, "pixelNorm", 1]
    first = common + ["randSeed", 101, "load_model_test", 4, "load_model_no", 1199, "upsamplingMode", 2, "upsampledData", 0,
                      "upsampleFirst", 0]
    second = common + ["randSeed", 102, "load_model_test", 48, "load_model_no", 799, "upsamplingMode", 0, "upsampledData", 1,
                       "outNNTestNo", 4]
    _run(first, str(tmp_path))
    _run(second, str(tmp_path))
    assert not glob.glob(str(tmp_path / "models" / "**" / "*.png"), recursive=True)
    h1, f1 = uniio.readUni(str(d / "density_low_t0004_2x2x1_0000.uni"))
    h0, f0 = uniio.readUni(str(d / "density_low_t0048_1x1x1_0000.uni"))
    assert (h1["dimX"], h1["dimY"], h1["dimZ"]) == (s, s, sim) and f1.shape == (sim, s, s, 1)
    assert (h0["dimX"], h0["dimY"], h0["dimZ"]) == (s, s, s) and f0.shape == (s, s, s, 1)
    # the library calls on the same input: what the loader hands the driver (velScale applied), the driver's generators
    low = np.array(v, dtype=F32)
    low[..., 1:4] = F32(0.7) * low[..., 1:4]
    g1, g0 = _gens(MP, ops.parse_prec("2"), seeds=(101, 102), widths=NARROW)
    want1 = MP.plane_pass_8x(g1, _t(low), up, batch=2)
    assert np.array_equal(f1[..., 0], want1.cpu().numpy())
    want0 = MP.upsample_pass_8x(g0, _t(low), _t(f1[..., 0]), up, 0, batch=2)
    assert np.array_equal(f0[..., 0], want0.cpu().numpy()) and np.count_nonzero(f0) > 0
    # once more with previews 1: a source_%04d.png per invocation, the same volumes -- written this time by the device
    # codecs with the unit index, the 2x2x1 one read back on the GPU (uniCodec, uniIndex, deviceRead as in the other modes)
    out = _run(first + ["previews", 1, "uniCodec", 2, "uniIndex", 1], str(tmp_path))
    assert np.array_equal(uniio.readUni(str(d / "density_low_t0004_2x2x1_0000.uni"))[1], f1)
    out += _run(second + ["previews", 1, "uniCodec", 1, "uniIndex", 1, "deviceRead", 1], str(tmp_path))
    pngs = sorted(os.path.relpath(p, str(tmp_path / "models")) for p in
                  glob.glob(str(tmp_path / "models" / "**" / "*.png"), recursive=True))
    assert pngs == ["test_0004/out_0004-1199_0000/source_0000.png", "test_0048/out_0048-0799_0000/source_0000.png"], pngs
    assert out.count("1 pngs written") == 2
    assert np.array_equal(uniio.readUni(str(d / "density_low_t0048_1x1x1_0000.uni"))[1], f0)
