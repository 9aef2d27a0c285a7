"""ConvFn / ConvDgradFn / ConvWgradFn (mpgan_amd/train.py) driven directly, to second order, against the float64
autograd reference of conv_triad_ref.py: the nine outputs y, dx, dw, db, gw1, gu1, gx2, gu2, gu3 of every case, each of
them what one kernel path of the triad wrote.

* exact: small-integer data, every output equal to the reference bit for bit (np.array_equal).  A mismatch is a fault to
  locate: no factor on any of these paths is anything but a power of two.
* normal / small: seeded normal data, and the same with u and px at 1e-6.  Relative L2 per output, at the project's
  bounds: 2e-5 for an output of an MFMA kernel at F16X3, 1e-5 for one of an fp32 vector-ALU kernel.  Relative L2 has no
  scale, so "small" has the same bounds: a path that splits a 1e-6 tensor into fp16 without its power-of-two scale fails.
* one shape at MPG_PREC_F16F6: forward and data-gradient outputs within 1.5e-4 and at most half the F16X1 error.
* the G8 forms cached on a tensor follow in-place changes of it.

Every test prints the measured error of every output ("triad-error ..." lines; profiles/r10/conv_triad_errors.txt is
their collection on an MI355X).
"""
import numpy as np
import pytest
import torch

import conv_triad_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.tensor(a, dtype=torch.float32, device=DEV)      # a copy: the shared arrays are read-only


def make_cfg(case, wscale, prec):
    s = case.launch[4]
    return {"stride": (s, s), "wscale": wscale, "prec": prec, "fc": case.fc}


def hip_outputs(case, kind, prec):
    """the outputs of conv_triad_ref.derivatives with ConvFn as TrainSession applies it (a 4x4 stride-2 layer on an even
    image as the 3x3 stride-1 convolution over the space-to-depth input), as float32 arrays"""
    from mpgan_amd.train import ConvFn, space_to_depth2, strided4_as_3x3
    d, wscale = R.make_data(case, kind)
    t = {k: dev(v).requires_grad_(k in R.LEAVES) for k, v in d.items()}
    cfg = make_cfg(case, wscale, prec)
    if case.s2d:
        fn = lambda x, w, b: ConvFn.apply(space_to_depth2(x), strided4_as_3x3(w), b, cfg)      # noqa: E731
    else:
        fn = lambda x, w, b: ConvFn.apply(x, w, b, cfg)      # noqa: E731
    out = R.derivatives(fn, t)
    torch.cuda.synchronize()
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in out.items()}


def check_zeros(got, problems):
    for name in R.ZEROS:
        if got[name] is not None and got[name].any():
            problems.append("%s: structurally zero, got max |v| %.3e" % (name, float(np.abs(got[name]).max())))


def report(case, kind, prec, name, err, bound):
    print("triad-error %-26s %-6s prec %d %-3s %.3e (bound %.1e)" % (case.name, kind, prec, name, err, bound))


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_triad_exact(gpu_ops, case):
    got = hip_outputs(case, "exact", gpu_ops.PREC_F16X3)
    want = R.reference(case, "exact")
    problems = []
    for name in R.OUTPUTS:
        w32 = want[name].astype(np.float32)
        msg = R.mismatch_report(got[name], w32, name)
        report(case, "exact", gpu_ops.PREC_F16X3, name, R.rel_l2(got[name], want[name]) if msg else 0.0, 0.0)
        if msg:
            problems.append(msg)
        else:
            assert np.array_equal(got[name], w32)
    check_zeros(got, problems)
    assert not problems, "\n".join([repr(case)] + problems)


@pytest.mark.parametrize("kind", ["normal", "small"])
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_triad_rel_l2(gpu_ops, case, kind):
    got = hip_outputs(case, kind, gpu_ops.PREC_F16X3)
    want = R.reference(case, kind)
    problems = []
    for name in R.OUTPUTS:
        assert got[name].shape == want[name].shape and got[name].dtype == np.float32, name
        err, bound = R.rel_l2(got[name], want[name]), case.tol(name)
        report(case, kind, gpu_ops.PREC_F16X3, name, err, bound)
        if not err < bound:
            problems.append("%s: relative L2 %.3e, bound %.1e" % (name, err, bound))
    check_zeros(got, problems)
    assert not problems, "\n".join([repr(case), kind] + problems)


@pytest.mark.parametrize("kind", ["normal", "small"])
def test_triad_f16f6(gpu_ops, kind):
    """the one shape at which _conv_prec keeps MPG_PREC_F16F6: forward and data-gradient outputs (y, gu1, gu2; dx, gx2)
    within the per-layer F16F6 bound and at most half the F16X1 error on the same data; weight gradients at F16X3"""
    case = R.F16F6_CASE
    want = R.reference(case, kind)
    got6 = hip_outputs(case, kind, gpu_ops.PREC_F16F6)
    got1 = hip_outputs(case, kind, gpu_ops.PREC_F16X1)
    problems = []
    for name in R.OUTPUTS:
        e6 = R.rel_l2(got6[name], want[name])
        if R.PATH_OF[name] in ("fwd", "dgrad"):
            e1 = R.rel_l2(got1[name], want[name])
            report(case, kind, gpu_ops.PREC_F16F6, name, e6, R.TOL_F16F6)
            report(case, kind, gpu_ops.PREC_F16X1, name, e1, float("nan"))
            if not e6 < R.TOL_F16F6:
                problems.append("%s: F16F6 relative L2 %.3e, bound %.1e" % (name, e6, R.TOL_F16F6))
            if not e6 <= 0.5 * e1:
                problems.append("%s: F16F6 relative L2 %.3e is more than half of F16X1's %.3e" % (name, e6, e1))
        else:
            bound = case.tol(name)
            report(case, kind, gpu_ops.PREC_F16F6, name, e6, bound)
            if not e6 < bound:
                problems.append("%s: relative L2 %.3e, bound %.1e" % (name, e6, bound))
    check_zeros(got6, problems)
    assert not problems, "\n".join([repr(case), kind] + problems)


def test_cached_g8_follows_the_tensor(gpu_ops):
    """_cached_g8 keeps the G8 form of a tensor on the tensor object.  An in-place change of the tensor must make a new
    one (twice the input: exactly twice the output, the hi/lo split and the abs-max scale being exact under a power of
    two), an unchanged tensor must reuse it and give the same bits."""
    from mpgan_amd import train
    case = R.CASES[0]
    # the plain forward splits x unscaled (the G8 form lives on a temporary); integer data, whose lo plane is zero: the
    # lo plane of 2x is twice that of x only while neither is an fp16 subnormal.  The abs-max scaled forward
    # (ConvDgradFn.backward's) caches on x itself; normal data: 2x has the G8 bits of x and twice its scale
    for kind, scaled in (("exact", False), ("normal", True)):
        d, wscale = R.make_data(case, kind)
        cfg = dict(make_cfg(case, wscale, gpu_ops.PREC_F16X3), rescale_fwd=scaled)
        x, w = dev(d["x"]).requires_grad_(True), dev(d["w"]).requires_grad_(True)
        y1 = train.ConvFn.apply(x, w, None, cfg).detach()
        g1 = x._mpg_g8[True][0] if scaled else None
        with torch.no_grad():
            x.mul_(2)
        y2 = train.ConvFn.apply(x, w, None, cfg).detach()
        g2 = x._mpg_g8[True][0] if scaled else None
        assert float(y1.abs().max()) > 0 and torch.equal(y2, 2 * y1), kind
        y3 = train.ConvFn.apply(x, w, None, cfg).detach()
        assert torch.equal(y3, y2), kind
        if scaled:
            assert g2 is not g1 and x._mpg_g8[True][0] is g2      # converted again after the change, not without one
    # the weight gradient's scaled forms of both operands; integer data: the atomics that combine the row ranges and the
    # images add exact numbers, so the bits do not depend on their order
    d, wscale = R.make_data(case, "exact")
    cfg = make_cfg(case, wscale, gpu_ops.PREC_F16X3)
    x, u = dev(d["x"]), dev(d["u"])
    dw1 = train._conv_wgrad(x, u, cfg, case.kh, case.kw)
    gx1, gu1 = x._mpg_g8[True][0], u._mpg_g8[True][0]
    want = R.reference(case, "exact")["dw"].astype(np.float32)
    assert np.array_equal(dw1.cpu().numpy(), want)
    u.mul_(0.5)
    dw2 = train._conv_wgrad(x, u, cfg, case.kh, case.kw)
    assert torch.equal(dw2, 0.5 * dw1) and np.array_equal(dw2.cpu().numpy(), 0.5 * want)
    assert x._mpg_g8[True][0] is gx1 and u._mpg_g8[True][0] is not gu1
    gu2 = u._mpg_g8[True][0]
    dw3 = train._conv_wgrad(x, u, cfg, case.kh, case.kw)
    assert torch.equal(dw3, dw2)
    assert x._mpg_g8[True][0] is gx1 and u._mpg_g8[True][0] is gu2
