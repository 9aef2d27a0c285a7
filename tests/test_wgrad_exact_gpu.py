"""The matrix-core weight gradient (wgrad_ring_kernel, wgrad_mfma_kernel of csrc/mpgan_wgrad_mfma.hip) compared bit for
bit with its definition, across every kernel instantiation and every run-time branch of its host planner.

The relative-L2 checks of test_train_gpu.py run Gaussian data: a fault confined to a few of the kh kw cin cout outputs
(the lo plane dropped on one edge tap, a halo row of the neighbouring image where a zero belongs, a ragged last k-step
that takes pad pixels) changes them by about 2^-13 relative and hides under the bound.  The data here
(wgrad_exact_ref.py) has non-zero lo parts and is still exact in fp32 under any summation order, so the assertion is
np.array_equal against the float64 sum of the three products (one at MPG_PREC_F16X1), at dy magnitudes 1 and 2^-20.
The three entries -- fp32 tensors with the maxima computed inside, fp32 tensors with max |dy| handed in and x unscaled
(the training step's call), and G8 operands -- must all give those bits: with exact partial sums the order of the
atomics that combine row ranges does not matter.

test_wgrad_exact_host.py proves on the CPU, for every case below, that the data splits as intended, that the bound holds,
that the expectation is an fp32 number, and that the case is in the launch class it names.

A failure says where: the number of mismatches, the first (ky, kx, ci, co), the taps and the ci / cout tiles hit.
"""
import ctypes

import numpy as np
import pytest
import torch

import wgrad_exact_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64          # floats on both sides of dw in the guarded call


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _params(cases):
    return [pytest.param(c, p, id="%s-x%d" % (c.name, p)) for c in cases for p in c.precs]


@pytest.mark.parametrize("e", R.EXPONENTS, ids=lambda e: "e%d" % e)
@pytest.mark.parametrize("case,prec", _params(R.CASES))
def test_wgrad_is_exact(gpu_ops, case, prec, e):
    from mpgan_amd import train_ops
    d = R.case_data(case)
    want = d.expected(prec, e)
    x, dy = _t(d.x), _t(d.dy(e))
    kh, kw = case.kh, case.kw
    what = "%s, prec %d, dy 2^%d" % (case.name, prec, e)
    # both maxima computed inside: x is scaled by its own maximum
    dw = train_ops.conv2d_wgrad_mfma(x, dy, kh, kw, R.WSCALE, prec)
    msg = R.mismatch_report(dw.cpu().numpy(), want, what + ", no amax given")
    assert not msg, msg
    # the training step's call: max |dy| from its producer, x split unscaled
    am = gpu_ops.absmax(dy)
    dw = train_ops.conv2d_wgrad_mfma(x, dy, kh, kw, R.WSCALE, prec, am, train_ops.unit_amax(dy.device))
    msg = R.mismatch_report(dw.cpu().numpy(), want, what + ", dy_amax given, x unscaled")
    assert not msg, msg
    # the G8 tensors a training step already holds
    dw = train_ops.conv2d_wgrad_g8(gpu_ops.to_g8(x), gpu_ops.to_g8(dy, amax=am), kh, kw, R.WSCALE, prec, None, am)
    msg = R.mismatch_report(dw.cpu().numpy(), want, what + ", G8 operands")
    assert not msg, msg


@pytest.mark.parametrize("case,prec", _params(R.GUARD_CASES))
def test_wgrad_stays_inside_dw(gpu_ops, case, prec):
    """the raw ABI call with dw inside a larger NaN-filled buffer: the guard floats on both sides are still NaN and every
    element of dw is finite and right, so the zeroing reached all of dw and no atomic of a ragged cout tile left it"""
    from mpgan_amd import _lib
    from mpgan_amd.ops import _ptr, _stream
    lib = _lib.load()
    d = R.case_data(case)
    x, dy = _t(d.x), _t(d.dy(0))
    xg, dg = gpu_ops.to_g8(x), gpu_ops.to_g8(dy)
    size = case.kh * case.kw * case.cin * case.cout
    buf = torch.full((GUARD + size + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    dw_ptr = ctypes.c_void_p(buf.data_ptr() + 4 * GUARD)
    _lib.check(lib.mpg_conv2d_wgrad_g8(_stream(), _ptr(xg.buf), case.n, case.h, case.w, case.cin, _ptr(dg.buf), case.cout, case.kh,
                                       case.kw, R.WSCALE, prec, None, None, dw_ptr), "mpg_conv2d_wgrad_g8")
    got = buf.cpu().numpy()
    assert np.isnan(got[:GUARD]).all(), "%s, prec %d: written in front of dw" % (case.name, prec)
    assert np.isnan(got[GUARD + size:]).all(), "%s, prec %d: written behind dw" % (case.name, prec)
    dw = got[GUARD:GUARD + size].reshape(case.kh, case.kw, case.cin, case.cout)
    assert np.isfinite(dw).all(), "%s, prec %d: %d elements of dw are not finite" % (case.name, prec, int((~np.isfinite(dw)).sum()))
    msg = R.mismatch_report(dw, d.expected(prec, 0), "%s, prec %d, guarded call, both operands unscaled" % (case.name, prec))
    assert not msg, msg


@pytest.mark.parametrize("case,prec", _params(R.NORMAL_CASES))
def test_wgrad_normal_data(gpu_ops, case, prec):
    """arbitrary mantissas at the launch classes the Gaussian tests of test_train_gpu.py do not reach, at their bounds"""
    from mpgan_amd import train_ops
    from test_train_gpu import ref_conv_grads, rel
    x, dy = R.normal_data(case)
    wt = np.zeros((case.kh, case.kw, case.cin, case.cout), np.float32)
    _, dw_ref = ref_conv_grads(x, wt, dy, 1, R.NORMAL_WSCALE)
    dyd = _t(dy)
    am = gpu_ops.absmax(dyd)
    calls = (("no amax given", lambda: train_ops.conv2d_wgrad_mfma(_t(x), dyd, case.kh, case.kw, R.NORMAL_WSCALE, prec)),
             ("dy_amax given, x unscaled", lambda: train_ops.conv2d_wgrad_mfma(_t(x), dyd, case.kh, case.kw, R.NORMAL_WSCALE, prec, am,
                                                                                train_ops.unit_amax(dyd.device))),
             ("G8 operands", lambda: train_ops.conv2d_wgrad_g8(gpu_ops.to_g8(_t(x)), gpu_ops.to_g8(dyd, amax=am), case.kh, case.kw,
                                                               R.NORMAL_WSCALE, prec, None, am)))
    for name, call in calls:
        dw = call().cpu().numpy()
        assert dw.shape == dw_ref.shape
        err = rel(dw, dw_ref)
        print("%s, prec %d, %s: relative L2 %.3e" % (case.name, prec, name, err))
        assert err < R.NORMAL_BOUND[prec], (case, prec, name, err)
