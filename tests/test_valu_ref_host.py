"""The references of tests/valu_ref.py checked on the CPU: batch norm forward / backward against float64 autograd, the
activation derivative (y = 0 included) against autograd of the header's activations, the index-statement transposes against
numpy.transpose / reshape, and the float32 two-pass variance whose error bounds the kernel in test_valu_paths_gpu.py."""
import itertools

import numpy as np
import pytest
import torch

import valu_ref as VR

DT = torch.float64


@pytest.mark.parametrize("act", [None, "relu", "lrelu"])
@pytest.mark.parametrize("npix,c", [(1, 4), (5, 3), (37, 12), (300, 20)])
def test_bn_forward_backward_against_float64_autograd(npix, c, act):
    rng = np.random.default_rng(100 * npix + c)
    x = (rng.standard_normal((npix, c)) * 1.7 + 0.4).astype(np.float32)
    dy = rng.standard_normal((npix, c)).astype(np.float32)
    gamma = rng.standard_normal(c).astype(np.float32)
    gamma[0], gamma[1] = 0.0, -abs(gamma[1]) - 0.5
    beta = rng.standard_normal(c).astype(np.float32)
    eps = 1e-3
    xt, gt, bt = (torch.tensor(a, dtype=DT, requires_grad=True) for a in (x, gamma, beta))
    mu = xt.mean(0)
    var = ((xt - mu) ** 2).mean(0)
    z = (xt - mu) * torch.rsqrt(var + eps) * gt + bt
    yt = z if act is None else torch.relu(z) if act == "relu" else 0.6 * z + 0.4 * z.abs()
    y, mean, v = VR.bn_train_fwd(x, gamma, beta, eps, act, 0.2)
    assert np.allclose(y, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(mean, mu.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(v, var.detach().numpy(), rtol=1e-12, atol=1e-14)
    # the backward takes the gradient at the normalised output z (before the activation)
    gx, gg, gb = torch.autograd.grad(z, (xt, gt, bt), torch.tensor(dy, dtype=DT))
    dx, dgamma, dbeta = VR.bn_train_bwd(dy, x, gamma, eps)
    assert np.allclose(dx, gx.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(dgamma, gg.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(dbeta, gb.numpy(), rtol=1e-10, atol=1e-12)


def test_moving_average_uses_the_float32_decay():
    m = VR.moving_average(np.array([2.0]), np.array([1.0]), 0.9)
    d = float(np.float32(0.9))
    assert m[0] == d * 2.0 + (1.0 - d) * 1.0 and m[0] != 0.9 * 2.0 + 0.1


@pytest.mark.parametrize("act", [None, "relu", "lrelu", "tanh"])
def test_activation_derivative_through_the_output(act):
    """act'(v) stated through y = act(v), against float64 autograd of the header's activations; at v = 0 the header's rule:
    relu 0, lrelu 0.5 (1 + leak) (the zero gradient of |v| there), none and tanh 1"""
    leak = 0.2
    v = np.array([-2.0, -0.25, 0.0, 0.0, 0.5, 3.0, -1e-3, 1e-3], np.float64)
    vt = torch.tensor(v, dtype=DT, requires_grad=True)
    lk = float(np.float32(leak))
    yt = {None: vt * 1.0, "relu": torch.relu(vt), "lrelu": 0.5 * (1 + lk) * vt + 0.5 * (1 - lk) * vt.abs(),
          "tanh": torch.tanh(vt)}[act]
    (want,) = torch.autograd.grad(yt.sum(), vt)
    y = yt.detach().numpy()
    assert np.allclose(VR.act_fwd(v, act, lk), y, rtol=1e-15, atol=0)
    d32 = VR.act_deriv32(y.astype(np.float32), act, leak)
    assert d32.dtype == np.float32
    # float32 statement: one rounding, and for tanh the rounding of y (an absolute 2^-24 on 1 - y^2)
    assert np.allclose(d32, want.numpy(), rtol=2e-7, atol=1.2e-7 if act == "tanh" else 0)
    at0 = {None: 1.0, "relu": 0.0, "lrelu": float(np.float32(0.5) * (np.float32(1) + np.float32(leak))), "tanh": 1.0}[act]
    assert d32[2] == np.float32(at0) and d32[3] == np.float32(at0)
    dy = np.array([1.5, -2.0, 3.0, -4.0, 0.5, 1.0, 2.0, -1.0], np.float32)
    assert np.array_equal(VR.act_bwd32(dy, y.astype(np.float32), act, leak), dy * d32)
    assert np.allclose(VR.act_bwd64(dy, y, act, leak), dy * want.numpy(), rtol=2e-7, atol=1e-12)


@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_transposes_against_numpy(perm):
    rng = np.random.default_rng(5)
    v = (np.abs(rng.standard_normal((6, 5, 9))) * 0.001).astype(np.float32)
    v[0, 0, :3] = np.float32(0.0005)
    assert np.array_equal(VR.volume_transpose(v, perm), v.transpose(perm))
    want = v.transpose(perm).copy()
    want[want < np.float32(0.0005)] = 0
    got = VR.volume_transpose(v, perm, 0.0005)
    assert np.array_equal(got, want)
    assert (got == np.float32(0.0005)).sum() == 3          # strict comparison: the threshold itself stays


def test_space_depth_and_gather_against_numpy():
    rng = np.random.default_rng(6)
    for c in (6, 8):
        x = rng.standard_normal((2, 4, 6, c)).astype(np.float32)
        n, h, w, _ = x.shape
        y = VR.space_to_depth(x, 2)
        assert np.array_equal(y, x.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4 * c))
        assert np.array_equal(VR.depth_to_space(y, 2), x)
    a, b = rng.standard_normal((7, 4)).astype(np.float32), rng.standard_normal((7, 1)).astype(np.float32)
    got = VR.channel_gather(a, b, [1, 4, 3, 0, 4], [4.0, 1.0, 0.3, 2.0, 0.5], [1.0, 0.3, 0.3, 1.0, 3.0])
    cat = np.concatenate([a, b], axis=1)
    assert np.array_equal(got[:, 2], (cat[:, 3] * np.float32(0.3)) * np.float32(0.3))
    assert np.array_equal(got[:, 4], (cat[:, 4] * np.float32(0.5)) * np.float32(3.0))
    assert VR.pair_reduce([1.0, -2.0], None, 0) == 3.0 and VR.pair_reduce([1.0, -2.0], [0.5, 0.0], 1) == 4.25
    assert np.array_equal(VR.cutoff(np.array([0.0004, 0.0005, 0.0006], np.float32), 0.0005),
                          np.array([0.0, 0.0005, 0.0006], np.float32))


@pytest.mark.parametrize("kind", ["offset", "border", "sampled"])
def test_two_pass_float32_variance_error(kind):
    """The yardstick of the shifted one-pass variance test: the relative L2 error (over the 32 channels) of a plain float32
    two-pass variance against float64, on the data of VR.shift_case.  Printed; the kernel may exceed it by a factor of 8."""
    x, var64, err = VR.shift_case_reference(kind)
    q = VR.SHIFT_NPIX >> 3
    if kind == "offset":
        assert abs(float(x.mean()) - 50.0) < 0.05 and abs(float(x.std()) - 0.5) < 0.01
    else:
        rows = [q, 3 * q, 5 * q, 7 * q] if kind == "border" else VR.SHIFT_SAMPLED_ROWS
        assert len(set(rows)) == 4 and all(r in [j * VR.SHIFT_NPIX // 64 for j in range(64)] for r in VR.SHIFT_SAMPLED_ROWS)
        assert np.all(x[rows] == 8.0) and abs(float(np.delete(x, rows, 0).std()) - 1.0) < 0.01
    print("fp32 two-pass variance, case %s: relative L2 error %.3e against float64 -> kernel bound %.3e" % (kind, err, 8 * err))
    # numpy adds the 4099 rows one after the other: not exact, and within sqrt(npix) * 2^-24 = 3.8e-6 of float64
    assert 0.0 < err < np.sqrt(VR.SHIFT_NPIX) * 2.0 ** -24
