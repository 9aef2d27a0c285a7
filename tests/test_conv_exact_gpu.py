"""mpg_conv2d_fused compared bit for bit with its definition, across every launch class of the three kernel families.

The relative-L2 checks of test_kernels_gpu.py cannot see a local fault (one halo pixel at a tile corner, the last channel
of a ragged cout tile, a correction product lost in one padded tap slot), and their exact checks use small integers, for
which every lo plane and every bf6 correction product is zero.  The data here (conv_exact_ref.py) has non-zero lo parts
and is still exact: hi = +-1, lo = hi l 2^-f, every product of a_hi w_hi + a_lo w_hi + a_hi w_lo a multiple of 2^-f and
every fp32 partial sum exact in any order, every value an exact bf6 (e3m2) code under the kernels' block scales.  The
expectation is the float64 sum of the three products (one at MPG_PREC_F16X1), and the assertion is np.array_equal: it
pins the addressing of the lo images, the w_lo fragments, the bf6 planes, and the second and third products of F16X3; the
"scales" cases, whose channel groups differ by powers of two, also pin which block scale goes with which block.
conv_small_kernel multiplies hi + lo in fp32, so its cases use small integers.

test_conv_exact_host.py proves on the CPU, for every case below, that the data splits as intended, that the bound holds,
that the expectation is an fp32 number, and that the case is in the launch class its comment names.

A failure says where: the number of mismatches, the first (n, y, x, c) and its (tile row, tile column, cout tile).
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_exact_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _segments(ops, case, d, prec, scale=1.0, amax=None, pad_hi=None):
    """the launch's segments: an fp32 tensor where the segment reads all of it, a channel window of a wider G8 tensor
    otherwise; `scale` (a power of two) multiplies the activations, `amax` is the device scalar they are converted with"""
    segs = []
    for s, x, w in zip(case.segs, d.x, d.w):
        pk = ops.pack_conv_weights(_t(w), prec=prec)
        xt = _t(x * np.float32(scale))
        if amax is not None or s.c_off or s.c_total != s.cin:
            assert s.c_off % 8 == 0
            xt = ops.to_g8(xt, amax=amax)
        segs.append(ops.Segment(xt, pk, c_off=s.c_off, up_log2=s.up_log2, pad_hi=s.pad_hi if pad_hi is None else pad_hi))
    return segs


def _check(ops, case, prec, segs, want, what, **kw):
    """one launch with both outputs: the fp32 result equals `want` bit for bit, the G8 result holds the same values, and
    the channels of its last group beyond cout are zero"""
    th, tw = R.tile_hw(case, prec)
    what = "%s, prec %d%s" % (case.name, prec, what)
    if not case.g8:
        y = ops.conv2d_fused(segs, (case.h, case.w), act=case.act, **kw)
        msg = R.mismatch_report(y.cpu().numpy(), want, th, tw, what)
        assert not msg, msg
        return y
    assert np.array_equal(R.g8_roundtrip(want), want)
    y, g = ops.conv2d_fused(segs, (case.h, case.w), act=case.act, want_f32=True, want_g8=True, **kw)
    msg = R.mismatch_report(y.cpu().numpy(), want, th, tw, what)
    assert not msg, msg
    msg = R.mismatch_report(ops.from_g8(g).cpu().numpy(), want, th, tw, what + ", G8 output")
    assert not msg, msg
    # without the fp32 output (and without post_add) the MFMA kernels store the G8 planes from registers, no LDS staging
    g2 = ops.conv2d_fused(segs, (case.h, case.w), act=case.act, want_f32=False, want_g8=True, **kw)
    assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16)), what + ": G8-only launch differs"
    g = g2
    assert g.c == case.cout and g.groups == (case.cout + 7) // 8
    if case.cout % 8:
        assert not g.buf[:, -1, :, :, :, case.cout % 8:].any().item(), what + ": channels beyond cout are not zero"
    return y


def test_minimal_case_every_precision(gpu_ops):
    """1x1, 16 -> 32 channels, one 16x32 tile, one weight stage: whether the fp16 MFMA (precisions 1 and 3) and the
    block-scaled bf6 MFMA (precision 2) accumulate lo-exact data exactly.  Everything else in this module rests on it."""
    case = R.MINIMAL
    d = R.case_data(case)
    for prec in (1, 3, 2):
        want = d.expected(prec)
        y = gpu_ops.conv2d_fused(_segments(gpu_ops, case, d, prec), (case.h, case.w)).cpu().numpy()
        dev = np.abs(y.astype(np.float64) - d.expected64(prec))
        print("minimal case, prec %d: max |y - expectation| = %.6e (lo terms reach %.3e)"
              % (prec, dev.max(), np.abs(d.corr[0]).max()))
        msg = R.mismatch_report(y, want, 16, 32, "%s, prec %d" % (case.name, prec))
        assert not msg, msg
    # the corrections are in the result: precision 1 lacks them
    assert not np.array_equal(d.expected(1), d.expected(3))


@pytest.mark.parametrize("case", R.CASES[1:], ids=repr)
def test_launch_class_bit_exact(gpu_ops, case):
    d = R.case_data(case)
    for prec in case.precs:
        _check(gpu_ops, case, prec, _segments(gpu_ops, case, d, prec), d.expected(prec), "")


@pytest.mark.parametrize("case", R.SEG_CASES, ids=repr)
def test_segments_in_every_rotation(gpu_ops, case):
    """three and four segments with different filters, up_log2 0 / 1 / 4, channel windows at offsets 8 and 16 of wider
    G8 tensors and pad_hi 0 / 1 in one launch; partial sums are exact, so every order of the segments gives the same bits"""
    d = R.case_data(case)
    for prec in case.precs:
        segs = _segments(gpu_ops, case, d, prec)
        first = None
        for k, rot in enumerate(R.rotations(segs)):
            y = _check(gpu_ops, case, prec, rot, d.expected(prec), ", rotation %d" % k)
            first = y if first is None else first
            assert torch.equal(y.view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("case", R.PAD_HI_ODD, ids=repr)
def test_pad_hi_changes_nothing_for_odd_filters(gpu_ops, case):
    d = R.case_data(case)
    for prec in case.precs:
        want = d.expected(prec)
        for pad_hi in (0, 1):
            _check(gpu_ops, case, prec, _segments(gpu_ops, case, d, prec, pad_hi=pad_hi), want, ", pad_hi %d" % pad_hi)


@pytest.mark.parametrize("e", R.AMAX_EXPONENTS)
@pytest.mark.parametrize("case", R.AMAX_CASES, ids=repr)
def test_in_amax_undoes_the_power_of_two_scale(gpu_ops, case, e):
    """activations times 2^e, converted with to_g8(..., amax = max |x|) and convolved with in_amax: the expectation times
    2^e, bit for bit (a gradient of magnitude 2^-30 would vanish in the fp16 split without the scale)"""
    d = R.case_data(case)
    amax = gpu_ops.absmax(_t(d.x[0] * np.float32(2.0 ** e)))
    assert float(amax) == float(np.abs(d.x[0]).max()) * 2.0 ** e
    for prec in case.precs:
        want = (d.expected64(prec) * 2.0 ** e).astype(np.float32)
        assert want.any()
        _check(gpu_ops, case, prec, _segments(gpu_ops, case, d, prec, scale=2.0 ** e, amax=amax), want, ", 2^%d" % e,
               in_amax=amax)


@pytest.mark.parametrize("case", R.POST_ADD_CASES, ids=repr)
def test_post_add_into_a_channel_window(gpu_ops, case):
    """post_add reads channels post_add_coff .. post_add_coff + cout of a wider fp32 tensor; integer addends keep the
    sum exact, and NaNs in every other channel show that nothing outside the window is read into the result"""
    d = R.case_data(case)
    rng = np.random.default_rng(5)
    pa = rng.integers(-8, 9, size=(case.n, case.h, case.w, R.POST_ADD_STRIDE)).astype(np.float32)
    win = slice(R.POST_ADD_COFF, R.POST_ADD_COFF + case.cout)
    poisoned = np.full_like(pa, np.nan)
    poisoned[..., win] = pa[..., win]
    for prec in case.precs:
        want = (d.expected(prec).astype(np.float64) + pa[..., win]).astype(np.float32)
        _check(gpu_ops, case, prec, _segments(gpu_ops, case, d, prec), want, ", post_add", post_add=_t(poisoned),
               post_add_coff=R.POST_ADD_COFF)


def test_bad_arguments_are_refused_not_launched(gpu_ops):
    """post_add_coff + cout > post_add_stride, nseg = 5 and an up_log2 that does not divide the output return
    MPG_ERR_ARG from the library (MpgError through the checked binding) and nothing is written.  nseg and up_log2 are
    checked for a launch of the MFMA kernels (24 -> 40) and of conv_small_kernel (3 -> 5); a launch with post_add never
    takes conv_small_kernel, so its range check is that of the MFMA launch for both shapes."""
    from mpgan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9)
    for cin, cout in ((24, 40), (3, 5)):
        n, h, w = 1, 19, 40
        x = _t(rng.integers(-3, 4, size=(n, h, w, cin)))
        pk = gpu_ops.pack_conv_weights(_t(rng.integers(-2, 3, size=(3, 3, cin, cout))), prec=3)
        segs = [gpu_ops.Segment(x, pk)]
        pa = torch.zeros((n, h, w, 12), dtype=torch.float32, device=DEV)
        y = torch.full((n, h, w, cout), 7.0, dtype=torch.float32, device=DEV)

        def desc():
            d = gpu_ops._conv_desc(segs, (h, w), None, None, 0.2)
            d.y = y.data_ptr()
            return d

        def refused(d, what):
            rc = lib.mpg_conv2d_fused(gpu_ops._stream(), ctypes.byref(d))
            assert rc == 1, (what, rc)      # MPG_ERR_ARG
            with pytest.raises(_lib.MpgError):
                _lib.check(rc, what)
            assert lib.mpg_last_error()
            torch.cuda.synchronize()
            assert bool((y == 7.0).all()), what + ": the output was written"

        d = desc()
        d.post_add, d.post_add_stride, d.post_add_coff = pa.data_ptr(), 12, 12 - cout + 1
        refused(d, "post_add window past the stride")
        d = desc()
        d.nseg = 5
        refused(d, "nseg 5")
        d = desc()
        d.seg[0].up_log2 = 1            # 19 rows are not divisible by 2
        refused(d, "up_log2 that does not divide the output")
        # the unchanged descriptor does launch
        d = desc()
        assert lib.mpg_conv2d_fused(gpu_ops._stream(), ctypes.byref(d)) == 0
        torch.cuda.synchronize()
        assert not bool((y == 7.0).all())
