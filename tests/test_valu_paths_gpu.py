"""Every dispatch branch of the vector-ALU kernels (mpgan_elem.hip, mpgan_bn.hip, mpgan_train_conv.hip, mpgan_train_elem.hip)
called directly and held against the plain references of tests/valu_ref.py (checked on the CPU by test_valu_ref_host.py).

The host entry points choose a kernel by channel count, 16-byte pointer alignment, element count or a grid cap with a
grid-stride loop.  The conditions are copied here; a case names the one it is there for in its id.  When a constant changes
in the source, this table says which shapes have to move with it.  ("chan_sum4", "apply4", "cutoff4", "space_to_depth4":
the V = 4 instantiation of chan_sum_kernel, bn_apply_kernel, cutoff_kernel, space_to_depth_kernel.)  The branches of
mpgan_train_conv.hip (mpg_conv2d_wgrad, mpg_conv2d_dgrad, mpg_fc_forward) are not in this file: they are covered bit for
bit by test_train_conv_gpu.py, and those of mpgan_optim.hip by test_optim_gpu.py, each with a table of its own.

  constant                  value   source (file: constant or function)          cases that cross it
  BLK                       256     mpgan_valu.h: BLK
  chan_sum4 condition       c >= 16, c % 4 == 0, 16-byte pointers     mpgan_bn.hip: launch_chan_sum   BN_SHAPES ("chan_sum4" / "scalar")
  chan_sum4 block cap       512     mpgan_bn.hip: launch_chan_sum (mpgan_valu.h: split_pixels)   (66001, 128): ppi 8 -> 516 blocks asked
  chan_sum block cap        1024    mpgan_bn.hip: launch_chan_sum, CHAN_SUM_MAX_BLOCKS           (530001, 5): ppi 32 -> 1036 blocks asked
  CHAN_SUM_MAX_BLOCKS       1024    mpgan_bn.hip: CHAN_SUM_MAX_BLOCKS
  chan_sum4 unroll          8 pixels in flight (MODE 0, 3), 4 (MODE 2)   mpgan_bn.hip: chan_sum_kernel, UN   (4099, 32): 456 pixels a block, ppi 32
  sum_partials 8-deep loop  nblocks > 7 * 16 = 112    mpgan_valu.h: ordered_partials_sum           both capped cases
  BN4_CMAX                  512     mpgan_valu.h: BN4_CMAX; mpgan_bn.hip: launch_bn_apply     (300, 516), (64, 1028) take bn_apply_kernel<1>
  lanes cap                 256 channel quads a block  mpgan_valu.h: split_pixels  (64, 1028): 257 quads, two channel blocks
  BN_SHIFT_PIX              64 pixels, every pixel when npix < 64   mpgan_bn.hip: BN_SHIFT_PIX   npix 1, 5, 7, 37: fewer than 64
  AMAX_GRID                 2048    mpgan_valu.h: AMAX_GRID; mpgan_bn.hip: mpg_bn_train_bwd_ordered; mpgan_train_elem.hip: mpg_act_bwd   bn_bwd: npix * c > 524288; act_bwd: n > 2097152
  act_bwd float4 body       16-byte dy, y, dx; tail n % 4   mpgan_train_elem.hip: act_bwd_kernel
  pair_reduce cap           1024 blocks of 8 * BLK    mpgan_train_elem.hip: mpg_pair_reduce      n = 2100003 asks 1026
  channel_gather cap        16384 blocks  mpgan_elem.hip: mpg_channel_gather      1050000 * 5 > 16384 * 256
  cutoff4                   n >= 1024, 16-byte pointers; tail n % 4   mpgan_elem.hip: mpg_cutoff
  transpose_tiled4          c == 1, perm[2] != 2, extents % 4 == 0, 16-byte pointers, 64 x 64 tiles   mpgan_elem.hip: mpg_volume_transpose
  swap01_rows               perm (1, 0, 2), d2 % 4 == 0, 16-byte pointers   mpgan_elem.hip: mpg_volume_transpose
  space_to_depth4           c % 4 == 0, 16-byte x and y   mpgan_elem.hip: mpg_space_to_depth
  bn_infer / bwd2 float4    c % 4 == 0, 16-byte pointers  mpgan_bn.hip: mpg_bn_train_bwd2_ordered, mpg_bn_infer_act

Tolerances are the project's: 1e-5 relative L2 for fp32 kernels whose accumulation order differs (tests/test_train_gpu.py),
1e-4 on the variance (test_conv_layer_fn), 1e-6 for elementwise kernels and the ordered channel sum, exact where a kernel
only moves or multiplies once.  A misaligned tensor is buf[1:1 + numel] of a contiguous float32 buffer: contiguous, 4-byte
but not 16-byte aligned, as a view into a flat parameter or gradient buffer is."""
import itertools

import numpy as np
import pytest
import torch

import valu_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-3
LEAK = 0.2


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _misaligned(t):
    """a contiguous copy of t that starts 4 bytes behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _misaligned_empty(shape, fill=None):
    n = int(np.prod(shape))
    buf = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    v = buf[1:1 + n].view(shape)
    if fill is not None:
        v.fill_(fill)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _aligned(t):
    assert t.data_ptr() % 16 == 0
    return t


def _abi():
    from mpgan_amd import _lib, ops
    return _lib.load(), _lib, ops._stream, ops._ptr


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. batch norm, first derivative
BN_SHAPES = [
    # npix, c, misaligned, activations, id = the branches the shape is there for
    (1, 4, False, (None, "relu", "lrelu"), "npix1-below_BN_SHIFT_PIX-one_sample"),
    (5, 3, False, (None, "relu", "lrelu"), "npix5-below_BN_SHIFT_PIX-scalar"),
    (7, 16, False, (None, "relu", "lrelu"), "npix7-below_BN_SHIFT_PIX-chan_sum4"),
    (37, 5, False, (None,), "c5-scalar_sums-scalar_apply"),
    (37, 12, False, (None,), "c12-scalar_sums-apply4"),
    (37, 16, False, (None,), "c16-chan_sum4-apply4"),
    (37, 20, False, (None,), "c20-chan_sum4-half_filled_lanes"),
    (37, 130, False, (None,), "c130-scalar_throughout"),
    (4099, 32, False, (None,), "chan_sum4-unroll_tails-odd_npix"),
    (66001, 128, False, (None, "relu", "lrelu"), "chan_sum4-cap512-ragged_last_block-amax_stride"),
    (530001, 5, False, (None,), "scalar-cap1024-partials_unroll8-amax_stride"),
    (300, 516, False, (None,), "chan_sum4-scalar_apply-c_above_BN4_CMAX"),
    (64, 1028, False, (None,), "chan_sum4-two_channel_blocks"),
    (4099, 32, True, (None,), "unaligned-x_dy-scalar_throughout"),
]
BN_CASES = [pytest.param(npix, c, mis, act, id="%s-%s" % (name, act))
            for npix, c, mis, acts, name in BN_SHAPES for act in acts]


def _bn_inputs(npix, c, misaligned):
    gen = torch.Generator(device=DEV).manual_seed(1000 * c + npix % 997)
    x = torch.randn((npix, c), device=DEV, generator=gen) * 1.7 + 0.4
    dy = torch.randn((npix, c), device=DEV, generator=gen) * 1e-2
    gamma = torch.randn((c,), device=DEV, generator=gen)
    gamma[0] = 0.0
    gamma[1] = -abs(float(gamma[1])) - 0.5
    beta = torch.randn((c,), device=DEV, generator=gen)
    mm0 = torch.randn((c,), device=DEV, generator=gen)
    mv0 = torch.rand((c,), device=DEV, generator=gen) + 0.5
    if misaligned:
        x, dy = _misaligned(x), _misaligned(dy)
    else:
        _aligned(x), _aligned(dy)
    return x, dy, gamma, beta, mm0, mv0


_BN_REF = {}


def _bn_reference(npix, c, misaligned):
    """float64 statistics and gradients of one shape, computed once and shared by its activation cases"""
    key = (npix, c, misaligned)
    if key not in _BN_REF:
        x, dy, gamma, _, _, _ = _bn_inputs(npix, c, misaligned)
        xn = _np(x).astype(np.float64)
        mean = xn.mean(axis=0)
        var = ((xn - mean) ** 2).mean(axis=0)
        _BN_REF[key] = (mean, var) + VR.bn_train_bwd(_np(dy), xn, _np(gamma), EPS)
    return _BN_REF[key]


@pytest.mark.parametrize("npix,c,misaligned,act", BN_CASES)
def test_bn_train_fwd_bwd(gpu_ops, npix, c, misaligned, act):
    from mpgan_amd import train_ops
    x, dy, gamma, beta, mm0, mv0 = _bn_inputs(npix, c, misaligned)
    mean64, var64, dx64, dgamma64, dbeta64 = _bn_reference(npix, c, misaligned)
    decay = 0.9
    runs = []
    for _ in range(2):
        mm, mv = mm0.clone(), mv0.clone()
        y, mean, var = train_ops.bn_train_fwd(x, gamma, beta, EPS, act, LEAK, mm, mv, decay)
        dx, dgamma, dbeta, amax = train_ops.bn_train_bwd(dy, x, mean, var, gamma, EPS, want_amax=True)
        runs.append((y, mean, var, mm, mv, dx, dgamma, dbeta, amax))
    names = ("y", "mean", "var", "moving_mean", "moving_var", "dx", "dgamma", "dbeta", "amax")
    for name, a, b in zip(names, runs[0], runs[1]):
        assert torch.equal(a, b), name                        # block sums added in a fixed order: the same bits
        assert torch.isfinite(a).all(), name
    y, mean, var, mm, mv, dx, dgamma, dbeta, amax = runs[0]
    xn, gn, bn = _np(x).astype(np.float64), _np(gamma).astype(np.float64), _np(beta).astype(np.float64)
    y64 = VR.act_fwd((xn - mean64) / np.sqrt(var64 + EPS) * gn + bn, act, LEAK)
    checks = [("y", y, y64, 1e-5), ("mean", mean, mean64, 1e-5), ("var", var, var64, 1e-4),
              ("moving_mean", mm, VR.moving_average(_np(mm0), mean64, decay), 1e-5),
              ("moving_var", mv, VR.moving_average(_np(mv0), var64, decay), 1e-5),
              ("dx", dx, dx64, 1e-5), ("dgamma", dgamma, dgamma64, 1e-5), ("dbeta", dbeta, dbeta64, 1e-5)]
    if npix == 1:
        # one pixel: x - mean is zero, and so are the variance, dgamma and dx, in the reference and to the bit in the kernel
        for name, got, want, _ in checks:
            if name in ("var", "dx", "dgamma"):
                assert not np.any(want) and not _np(got).any(), name
        checks = [ch for ch in checks if ch[0] not in ("var", "dx", "dgamma")]
    errs = [(name, VR.rel(_np(got), want), tol) for name, got, want, tol in checks]
    print("bn npix=%d c=%d act=%s: %s" % (npix, c, act, " ".join("%s %.2e" % (n, e) for n, e, _ in errs)))
    for name, e, tol in errs:
        assert e < tol, (name, e)
    assert amax.dim() == 0 and torch.equal(amax, dx.abs().max())      # a maximum has no rounding


@pytest.mark.parametrize("kind", ["offset", "border", "sampled"])
def test_bn_shifted_one_pass_variance(gpu_ops, kind):
    """The batch variance comes from ONE pass over x: sums of (x - k) and (x - k)^2 around a shift k taken from a few pixels
    (bn_shift_kernel).  Two data sets at (4099, 32) aim at the shift (VR.shift_case): "offset" has mean 50 and sigma 0.5,
    "border" is N(0, 1) with the pixels q, 3q, 5q, 7q (q = npix >> 3) at +8 sigma in every channel: the four pixels the shift
    was first taken from, which put it 8 sigma from the mean.  "sampled" puts the same four outliers on rows the 64-pixel
    shift does read (rows j * npix / 64, j = 8, 24, 40, 56): k then sits 4 * 8 / 64 = 0.5 sigma from the mean, the most
    that four such pixels can do to it.
    The yardstick is a plain float32 two-pass variance (mean, then centred sum of squares; test_valu_ref_host.py prints it):
    its relative L2 error against float64 is 9.76e-07 (offset), 7.95e-07 (border) and 7.38e-07 (sampled); the kernel adds
    one subtraction and one fused multiply per element and folds 16 x blocks partials, and may exceed that by a factor of 8:
    bounds 7.81e-06 (offset), 6.36e-06 (border) and 5.90e-06 (sampled).  Measured on an MI355X with the four-pixel shift:
    9.64e-08 (offset), 7.69e-06 (border: over the bound), which is why the shift is now the mean of 64 pixels; with that:
    5.98e-08 (offset), 6.16e-08 (border), 1.04e-07 (sampled).
    The mean is held to the usual 1e-5 relative L2."""
    from mpgan_amd import train_ops
    xn, var64, err32 = VR.shift_case_reference(kind)
    x = _aligned(_dev(xn))
    gamma, beta = torch.ones(VR.SHIFT_C, device=DEV), torch.zeros(VR.SHIFT_C, device=DEV)
    _, mean, var = train_ops.bn_train_fwd(x, gamma, beta, EPS)
    _, mean2, var2 = train_ops.bn_train_fwd(x, gamma, beta, EPS)
    e_var = VR.rel(_np(var), var64)
    e_mean = VR.rel(_np(mean), xn.astype(np.float64).mean(axis=0))
    print("bn_shift %s: variance error %.3e (float32 two-pass %.3e, bound %.3e), mean error %.3e"
          % (kind, e_var, err32, 8 * err32, e_mean))
    assert torch.equal(mean, mean2) and torch.equal(var, var2)
    assert e_mean < 1e-5
    assert e_var <= 8 * err32


# ---------------------------------------------------------------------------------------------- 2. activation backward
ACT_N = [(1, "n1-tail_only"), (3, "n3-tail_only"), (4, "n4-one_float4"), (5, "n5-float4_plus_tail"), (1023, "n1023-tail3"),
         (1025, "n1025-two_blocks-tail1"), (2_100_003, "n2100003-amax_stride-tail3")]


def _act_data(n, act):
    rng = np.random.default_rng(7 * n + len(str(act)))
    dy = rng.standard_normal(n).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    v[rng.random(n) < 0.125] = 0.0                            # exact zeros among positive and negative outputs
    v[-3:] = np.array([0.0, 0.75, -0.375], np.float32)[-n:]   # and in the last three elements (the scalar tail)
    y = np.tanh(v).astype(np.float32) if act == "tanh" else v
    return dy, y


@pytest.mark.parametrize("act", [None, "relu", "lrelu", "tanh"])
@pytest.mark.parametrize("n", [pytest.param(n, id=name) for n, name in ACT_N])
def test_act_bwd_and_abs_max(gpu_ops, n, act):
    lib, _lib, stream, ptr = _abi()
    dyn, yn = _act_data(n, act)
    assert (yn[-min(n, 3):] == 0).any() or n < 3
    want32 = VR.act_bwd32(dyn, yn, act, LEAK)
    want64 = VR.act_bwd64(dyn, yn, act, LEAK)
    # aligned: the float4 body and the scalar tail; one pointer unaligned at a time: all-scalar
    for which in ("aligned", "unaligned-dy", "unaligned-y", "unaligned-dx"):
        dy = _misaligned(_dev(dyn)) if which == "unaligned-dy" else _aligned(_dev(dyn))
        y = _misaligned(_dev(yn)) if which == "unaligned-y" else _aligned(_dev(yn))
        dx = _misaligned_empty((n,), 3.0) if which == "unaligned-dx" else _aligned(torch.full((n,), 3.0, device=DEV))
        amax = torch.full((), 7.0, device=DEV)
        _lib.check(lib.mpg_act_bwd(stream(), ptr(dy), ptr(y), n, _lib.act_id(act), LEAK, ptr(dx), ptr(amax)), "mpg_act_bwd")
        got = _np(dx)
        if act == "tanh":
            assert VR.rel(got, want64) < 1e-6, which
        else:
            assert np.array_equal(got, want32), which         # one fp32 multiply by an exact or once-rounded constant
        assert float(amax) == float(np.abs(got).max()), which
        assert torch.equal(amax, dx.abs().max()), which
        # dy = 0: the entry point clears the abs-max it is given
        amax.fill_(7.0)
        zero = torch.zeros_like(dy) if which != "unaligned-dy" else _misaligned(torch.zeros((n,), device=DEV))
        _lib.check(lib.mpg_act_bwd(stream(), ptr(zero), ptr(y), n, _lib.act_id(act), LEAK, ptr(dx), ptr(amax)), "mpg_act_bwd")
        assert float(amax) == 0.0, which
        assert not dx.any(), which


def test_act_bwd_wrapper(gpu_ops):
    """the wrapper of train_ops (what the training step calls) on the strided size"""
    from mpgan_amd import train_ops
    n = 2_100_003
    dyn, yn = _act_data(n, "lrelu")
    dx, amax = train_ops.act_bwd(_dev(dyn), _dev(yn), "lrelu", LEAK, want_amax=True)
    assert np.array_equal(_np(dx), VR.act_bwd32(dyn, yn, "lrelu", LEAK))
    assert torch.equal(amax, dx.abs().max())
    assert torch.equal(train_ops.act_bwd(_dev(dyn), _dev(yn), "lrelu", LEAK), dx)


# ---------------------------------------------------------------------------------------------- 3. reductions
SUM_CASES = [pytest.param(npix, c, mis, id="%s%s" % (name, "-unaligned" if mis else ""))
             for npix, c, name in [(s[0], s[1], s[4]) for s in BN_SHAPES if not s[2]] + [(120, 12, "c12-scalar_sums-small")]
             for mis in (False, True)]


@pytest.mark.parametrize("npix,c,misaligned", SUM_CASES)
def test_channel_sum_ordered(gpu_ops, npix, c, misaligned):
    from mpgan_amd import train_ops
    gen = torch.Generator(device=DEV).manual_seed(77 * c + npix % 991)
    x = torch.randn((npix, c), device=DEV, generator=gen) * 1.7 + 0.4
    x = _misaligned(x) if misaligned else _aligned(x)
    s, again = train_ops.channel_sum(x), train_ops.channel_sum(x)
    assert torch.equal(s, again)                              # fixed order
    e = VR.rel(_np(s), VR.channel_sum(_np(x)))
    print("channel_sum npix=%d c=%d unaligned=%s rel %.3e" % (npix, c, misaligned, e))
    assert e < 1e-6


@pytest.mark.parametrize("with_b", [True, False], ids=["b", "b_null"])
@pytest.mark.parametrize("mode", [0, 1], ids=["abs", "square"])
@pytest.mark.parametrize("n", [pytest.param(1, id="n1"), pytest.param(255, id="n255-part_block"),
                               pytest.param(2049, id="n2049-two_blocks"), pytest.param(2_100_003, id="n2100003-cap1024-stride")])
def test_pair_reduce(gpu_ops, n, mode, with_b):
    from mpgan_amd import train_ops
    lib, _lib, stream, ptr = _abi()
    rng = np.random.default_rng(n + mode)
    an, bn = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    a, b = _dev(an), (_dev(bn) if with_b else None)
    want = VR.pair_reduce(an, bn if with_b else None, mode)
    # the terms are non-negative: no cancellation, 1e-5 relative holds for any order of the block sums
    got = float(train_ops.pair_reduce(a, b, mode))
    assert abs(got - want) <= 1e-5 * want, (got, want)
    out = torch.full((), 7.0, device=DEV)                     # twice into one buffer: the entry point clears it
    for _ in range(2):
        _lib.check(lib.mpg_pair_reduce(stream(), ptr(a), ptr(b), n, mode, ptr(out)), "mpg_pair_reduce")
        assert abs(float(out) - want) <= 1e-5 * want, (float(out), want)


# ---------------------------------------------------------------------------------------------- 4. marshalling (exact)
VOL_CASES = [
    ((68, 36, 100), False, "tiled4-ragged_tiles-swap01"),
    ((64, 128, 64), False, "tiled4-full_tiles-swap01"),
    ((68, 35, 100), False, "d1_not_mult4-scalar_tile"),
    ((68, 36, 70), False, "d2_not_mult4-scalar_tile-generic_swap01"),
    ((68, 36, 100), True, "unaligned-scalar_tile-generic_swap01"),
]
_VOL = {}


def _vol_data(shape):
    if shape not in _VOL:
        v = (np.abs(np.random.default_rng(sum(shape)).standard_normal(shape)) * 0.001).astype(np.float32)
        v[1, 2, :8] = np.float32(0.0005)                      # values equal to the threshold stay
        _VOL[shape] = v
    return _VOL[shape]


@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))), ids=lambda p: "perm%d%d%d" % p)
@pytest.mark.parametrize("shape,misaligned", [pytest.param(s, m, id=name) for s, m, name in VOL_CASES])
def test_volume_transpose_paths(gpu_ops, shape, misaligned, perm):
    vn = _vol_data(shape)
    v = _misaligned(_dev(vn)) if misaligned else _aligned(_dev(vn))
    for thr in (0.0, 0.0005):
        got = _np(gpu_ops.volume_transpose(v, perm, cutoff=thr))
        want = VR.volume_transpose(vn, perm, thr)
        assert got.shape == want.shape
        assert np.array_equal(got, want), thr
        if thr > 0:
            assert (got == 0).any() and (got == np.float32(0.0005)).sum() == 8


@pytest.mark.parametrize("which", ["aligned", "unaligned-in", "unaligned-out"])
@pytest.mark.parametrize("n", [pytest.param(1023, id="n1023-scalar"), pytest.param(1024, id="n1024-cutoff4-no_tail"),
                               pytest.param(1027, id="n1027-cutoff4-tail3"), pytest.param(70_001, id="n70001-cutoff4-many_blocks-tail1")])
def test_cutoff_paths(gpu_ops, n, which):
    rng = np.random.default_rng(n)
    vn = (rng.random(n) * 0.001).astype(np.float32)
    vn[::7] = np.float32(0.0005)                              # x < cutoff is strict: these stay
    vn[-1] = np.float32(0.0005)
    vn[-2] = np.float32(0.0004)
    v = _misaligned(_dev(vn)) if which == "unaligned-in" else _aligned(_dev(vn))
    out = _misaligned_empty((n,), 3.0) if which == "unaligned-out" else _aligned(torch.full((n,), 3.0, device=DEV))
    got = gpu_ops.cutoff(v, 0.0005, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = VR.cutoff(vn, 0.0005)
    assert (want == 0).any() and (want == np.float32(0.0005)).sum() >= n // 7
    assert np.array_equal(_np(got), want)


def test_channel_gather_strided(gpu_ops):
    """1050000 pixels x 5 output channels > 16384 blocks x 256 threads: the grid-stride loop goes round"""
    npix, cmap = 1_050_000, [1, 4, 3, 0, 4]
    scale, scale2 = [4.0, 1.0, 0.3, 2.0, 0.5], [1.0, 0.3, 0.3, 1.0, 3.0]
    rng = np.random.default_rng(11)
    an, bn = rng.standard_normal((npix, 4)).astype(np.float32), rng.standard_normal((npix, 1)).astype(np.float32)
    assert npix * len(cmap) > 16384 * 256
    got = _np(gpu_ops.channel_gather(_dev(an), _dev(bn), cmap, scale, scale2))
    assert np.array_equal(got, VR.channel_gather(an, bn, cmap, scale, scale2))


@pytest.mark.parametrize("c,which", [pytest.param(8, "aligned", id="c8-float4"), pytest.param(8, "unaligned-in", id="c8-unaligned-in-scalar"),
                                     pytest.param(8, "unaligned-out", id="c8-unaligned-out-scalar"),
                                     pytest.param(6, "aligned", id="c6-scalar")])
def test_space_to_depth_paths(gpu_ops, c, which):
    lib, _lib, stream, ptr = _abi()
    n, h, w, r = 2, 6, 10, 2
    xn = np.random.default_rng(c).standard_normal((n, h, w, c)).astype(np.float32)
    want = VR.space_to_depth(xn, r)
    x = _misaligned(_dev(xn)) if which == "unaligned-in" else _aligned(_dev(xn))
    if which == "unaligned-out":
        y = _misaligned_empty(want.shape, 3.0)
        _lib.check(lib.mpg_space_to_depth(stream(), ptr(x), n, h, w, c, r, ptr(y)), "mpg_space_to_depth")
    else:
        y = gpu_ops.space_to_depth(x, r)
    assert np.array_equal(_np(y), want)
    back = gpu_ops.depth_to_space(y, r)                        # the inverse, from the same (possibly unaligned) tensor
    assert np.array_equal(_np(back), xn)
    assert np.array_equal(_np(gpu_ops.depth_to_space(_dev(want), r)), VR.depth_to_space(want, r))


def test_bn_infer_act_unaligned_input(gpu_ops):
    """c = 32 takes the float4 apply; from a 4-byte aligned view it has to take the scalar one (tests/test_eval_gpu.py)"""
    from mpgan_amd import train_ops
    c, npix = 32, 4099
    rng = np.random.default_rng(c)
    xn = rng.standard_normal((1, npix, 1, c)).astype(np.float32)
    mean, var = rng.standard_normal(c).astype(np.float32), rng.uniform(0.2, 3.0, c).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    want = VR.act_fwd((xn.astype(np.float64) - mean) / np.sqrt(var.astype(np.float64) + 1e-3) * gamma + beta, "lrelu", LEAK)
    x = _misaligned(_dev(xn))
    y = train_ops.bn_infer_act(x, _dev(mean), _dev(var), _dev(gamma), _dev(beta), 1e-3, "lrelu", LEAK)
    assert VR.rel(_np(y), want) < 1e-6                       # an elementwise fp32 kernel


def test_bn_train_bwd2_unaligned_input(gpu_ops):
    """(4099, 32) with x and dz as 4-byte aligned views: bn_bwd2 falls to its one-channel kernels; the reference and the
    tolerance of test_bn_train_bwd2_matches_float64_autograd"""
    from mpgan_amd import train_ops
    m, c = 4099, 32
    gen = torch.Generator(device=DEV).manual_seed(1000 * c + m % 997)
    x = _misaligned(torch.randn((m, c), device=DEV, generator=gen) * 1.7 + 0.4)
    dz = _misaligned(torch.randn((m, c), device=DEV, generator=gen) * 1e-2)
    gamma = torch.randn((c,), device=DEV, generator=gen)
    gamma[0] = 0.0
    gamma[1] = -abs(float(gamma[1])) - 0.5
    beta = torch.randn((c,), device=DEV, generator=gen)
    gdx = torch.randn((m, c), device=DEV, generator=gen)
    gdg, gdb = torch.randn((c,), device=DEV, generator=gen), torch.randn((c,), device=DEV, generator=gen)
    _, mean, var = train_ops.bn_train_fwd(x, gamma, beta, EPS)
    got = train_ops.bn_train_bwd2(dz, x, mean, var, gamma, EPS, gdx, gdg, gdb)
    again = train_ops.bn_train_bwd2(dz, x, mean, var, gamma, EPS, gdx, gdg, gdb)
    want = VR.bn_double_backward_64(dz, x, gamma, gdx, gdg, gdb, EPS)
    for name, a, a2, b in zip(("g_dz", "g_x", "g_gamma"), got, again, want):
        assert torch.equal(a, a2), name
        assert torch.isfinite(a).all(), name
        r = VR.rel(_np(a), _np(b))
        assert r <= 1e-4, (name, r)
