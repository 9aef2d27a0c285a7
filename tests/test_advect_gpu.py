"""The advection and resample kernels (csrc/mpgan_advect.hip, mpg_semilagr_positions of csrc/mpgan_tiles.hip) and the
autograd Functions around them, bit for bit against the float64 oracles on the exact data of advect_ref.py: at the
borders (clamped indices, weights from the clamped indices), on every side the look-up can leave, with both signs, on
non-square grids, on ties on the MacCormack clamp bound, in all-obstacle neighbourhoods, with more batch rows than
columns, and at resolution ratios 1, 2, 4 and 8.  test_advect_host.py proves that every fp32 partial sum of these cases
is exact, so np.array_equal is the assertion and there is no list of exceptions.  Ratios that are no powers of two
(6 -> 16, 12 -> 16) run on normal data within the bounds test_train_gpu.py holds these quantities to."""
import numpy as np
import pytest
import torch

import advect_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MPG_ERR_ARG = 1            # include/mpgan.h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def same(got, want):
    """bit-equal as numbers (the expectation is float64 holding fp32 values)"""
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.shape == np.shape(want) and np.array_equal(got.astype(np.float64), np.asarray(want, np.float64))


def _maccormack(src, fwd, bwd, flags, disp, strength, n, h, w):
    """mpg_maccormack as _MacCormackFn.forward calls it -> (rc, out, keep)"""
    from mpgan_amd import _lib, train_ops
    out, keep = torch.full_like(src, -1.0), torch.full_like(src, -1.0)
    rc = _lib.load().mpg_maccormack(train_ops._stream(), train_ops._ptr(src), train_ops._ptr(fwd), train_ops._ptr(bwd),
                                    train_ops._ptr(flags), train_ops._ptr(disp), n, h, w, float(strength), train_ops._ptr(out),
                                    train_ops._ptr(keep))
    return rc, out, keep


@pytest.mark.parametrize("case", R.ADVECT_CASES, ids=repr)
def test_advect_exact(gpu_ops, case):
    """GAN.advect of order 1 and 2 through train_ops.advect: displacement field, forward, backward, MacCormack out and
    keep, and d out / d source of both orders for an integer upstream gradient"""
    from mpgan_amd import _lib, train_ops
    d, e = R.advect_data(case), R.advect_expect(case)
    n, h = case.n, case.h
    src, vel, flags, g = dev(d["src"]), dev(d["vel"]), dev(d["flags"]), dev(d["g"])
    disp = train_ops.advect_velocity(vel, h, h, R.DT)
    assert same(disp, e["disp"])
    s1 = src.clone().requires_grad_(True)
    fwd = train_ops.advect(s1, vel, flags, R.DT, 1)
    assert same(fwd, e["forward"])
    (d1,) = torch.autograd.grad(fwd, [s1], g)
    assert same(d1, e["dsrc1"])
    bwd = train_ops.semi_lagrange(fwd.detach(), disp, -1.0)
    assert same(bwd, e["backward"])
    s2 = src.clone().requires_grad_(True)
    out = train_ops.advect(s2, vel, flags, R.DT, 2, case.strength, start_bz=n)
    assert same(out, e["out"])
    rc, out_k, keep = _maccormack(src, fwd.detach(), bwd, flags, disp, case.strength, n, h, h)
    assert rc == _lib.MPG_OK
    assert same(out_k, e["out"])
    assert same(keep, e["keep"])
    (d2,) = torch.autograd.grad(out, [s2], g)
    assert same(d2, e["dsrc2"])


@pytest.mark.parametrize("case", R.LOOKUP_CASES, ids=repr)
def test_semi_lagrange_exact(gpu_ops, case):
    """mpg_semi_lagrange / _bwd on a displacement field, either sign, any h and w: the look-up against the oracle, its
    gradient against the explicit transposed gather, and the adjoint identity in float64, exactly"""
    from mpgan_amd import train_ops
    d, e = R.lookup_data(case), R.lookup_expect(case)
    src, disp, g = dev(d["src"]), dev(d["disp"]), dev(d["g"])
    out = train_ops.semi_lagrange(src, disp, case.sign)
    assert same(out, e["out"])
    ds = train_ops.semi_lagrange_bwd(g, disp, case.sign)
    assert same(ds, e["dsrc"])
    lhs = (host(out).astype(np.float64) * d["g"]).sum()
    rhs = (d["src"].astype(np.float64) * host(ds)).sum()
    assert lhs == rhs and lhs != 0
    # through the Function
    s = src.clone().requires_grad_(True)
    y = train_ops._SemiLagrangeFn.apply(s, disp, case.sign)
    (dsf,) = torch.autograd.grad(y, [s], g)
    assert same(y, e["out"]) and same(dsf, e["dsrc"])


@pytest.mark.parametrize("case", R.VELOCITY_CASES, ids=repr)
def test_advect_velocity(gpu_ops, case, capsys):
    from mpgan_amd import train_ops
    d, e = R.velocity_data(case), R.velocity_expect(case)
    disp = train_ops.advect_velocity(dev(d["vel"]), case.h, case.w, R.DT)
    if case.exact:
        assert same(disp, e["disp"])
        return
    err_v = float(np.abs(host(disp) - e["disp"]).max())
    fwd = train_ops.advect(dev(d["src"]), dev(d["vel"]), None, R.DT, 1)
    err_f = float(np.abs(host(fwd) - e["forward"]).max())
    with capsys.disabled():
        print("\nadvect_velocity %s: displacement max abs error %.3e, look-up max abs error %.3e" % (case, err_v, err_f))
    assert err_v < R.TOL_DISPLACEMENT
    assert err_f < R.TOL_LOOKUP


@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=repr)
def test_tensor_resample_exact(gpu_ops, case):
    from mpgan_amd import train_ops
    from mpgan_amd.train import ResampleFn
    d, e = R.resample_data(case), R.resample_expect(case)
    v = dev(d["value"]).requires_grad_(True)
    pos, g = dev(d["pos"]), dev(d["g"])
    out = ResampleFn.apply(v, pos, case.clamp)
    assert same(out, e["out"])
    (dv,) = torch.autograd.grad(out, [v], g)
    assert same(dv, e["dvalue"])
    assert same(train_ops.tensor_resample_bwd(g, pos, case.clamp), e["dvalue"])


@pytest.mark.parametrize("case", R.POSITIONS_CASES, ids=repr)
def test_semilagr_positions(gpu_ops, case, capsys):
    from mpgan_amd import tiles_device
    d, e = R.positions_data(case), R.positions_expect(case)
    pos = tiles_device.semilagr_positions(dev(d["vel"]), dev(d["dt"]), case.n_out)
    if case.exact:
        assert same(pos, e)
        return
    got = host(pos).astype(np.float64)
    with capsys.disabled():
        print("\nsemilagr_positions %s: max abs error %.3e" % (case, float(np.abs(got - e).max())))
    assert np.allclose(got, e, rtol=R.TOL_POSITIONS, atol=R.TOL_POSITIONS)


@pytest.mark.parametrize("which", ["semi_lagrange", "maccormack", "resample"])
def test_advect_functions_refuse_second_derivative(gpu_ops, which):
    """their backward passes are kernel calls without a tape: a second derivative has to raise, not read as zero (the
    product with `a` gives the first gradient a grad_fn of its own, so nothing else can raise here)"""
    from mpgan_amd import train_ops
    from mpgan_amd.train import ResampleFn
    case = R.ADVECT_CASES[0]
    d, e = R.advect_data(case), R.advect_expect(case)
    a = dev(d["src"]).requires_grad_(True)
    disp = dev(e["disp"])
    if which == "semi_lagrange":
        z = train_ops._SemiLagrangeFn.apply(a, disp, 1.0) * a
    elif which == "maccormack":
        z = train_ops._MacCormackFn.apply(a, disp, dev(d["flags"]), 1.0) * a
    else:
        z = ResampleFn.apply(a, dev(R.grid(case.h, case.h) - e["disp"] - np.float32(0.5)), True) * a
    (g,) = torch.autograd.grad(z.sum(), a, create_graph=True)
    assert g.grad_fn is not None
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g.sum().backward()


@pytest.mark.parametrize("h,w", [(8, 16), (16, 8)])
def test_maccormack_refuses_a_grid_that_is_not_square(gpu_ops, h, w):
    """three clamp corners clip their row index to w-1, as the reference writes it: for h < w that leaves the batch
    entry.  The entry refuses on the host and launches nothing: the outputs keep what they held."""
    from mpgan_amd import _lib
    n, m = 3, max(h, w)
    t = [torch.zeros((n, m, m, 1), dtype=torch.float32, device=DEV) for _ in range(4)]       # room for either reading of the shape
    disp = torch.zeros((n, m, m, 2), dtype=torch.float32, device=DEV)
    rc, out, keep = _maccormack(t[0], t[1], t[2], t[3], disp, 1.0, n, h, w)
    assert rc == MPG_ERR_ARG
    msg = _lib.load().mpg_last_error().decode()
    assert "square" in msg and "mpg_maccormack" in msg, msg
    torch.cuda.synchronize()
    assert (host(out) == -1.0).all() and (host(keep) == -1.0).all()
    with pytest.raises(_lib.MpgError, match="square"):
        _lib.check(rc, "mpg_maccormack")
