"""What test_conv_triad_gpu.py relies on, proven without a GPU: the exact data of conv_triad_ref.py gives fp32 results
whose every partial sum is exact, every case sits in the branch of _conv_fwd / _conv_dgrad / _conv_wgrad it names, the
float64 reference agrees with a loop convolution written from the definition, and the two pure-torch helpers that turn a
4x4 stride-2 layer into a 3x3 stride-1 one (space_to_depth2, strided4_as_3x3) are exact to second order."""
import numpy as np
import pytest
import torch

import conv_triad_ref as R

ALL = R.CASES + [R.F16F6_CASE]


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_exact_data_is_exact(case):
    d, wscale = R.make_data(case, "exact")
    assert wscale == R.EXACT_WSCALE and np.log2(wscale) == round(np.log2(wscale))
    for name, v in d.items():
        assert v.dtype == np.float32 and v.shape == R.shapes(case)[name]
        m = R.WMAX if name in ("w", "pw") else R.BMAX if name in ("b", "pb") else R.XMAX
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= m, name
        assert np.abs(v).max() > 0, name
    # every partial sum of every contraction, in any order, is a multiple of wscale below 2^24 of them
    for path, bound in R.term_bounds(case).items():
        assert bound + R.BMAX / wscale < 2 ** 24, (path, bound)
    ref = R.reference(case, "exact")
    for name in R.OUTPUTS:
        e = ref[name]
        assert e is not None and np.abs(e).max() > 0, name
        assert np.array_equal(e.astype(np.float32).astype(np.float64), e), name
        assert np.array_equal(e / wscale ** 2, np.round(e / wscale ** 2)), name
    for name in R.ZEROS:
        assert ref[name] is None or not ref[name].any(), name
    # the identities of the module docstring, bit for bit
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in d.items()}
    assert np.array_equal(ref["gu1"], R.conv(t["px"], t["w"] * wscale, case.stride).numpy())
    assert np.array_equal(ref["gu2"], R.conv(t["x"], t["pw"] * wscale, case.stride).numpy())
    assert np.array_equal(ref["gu3"], np.broadcast_to(d["pb"].astype(np.float64), ref["gu3"].shape))
    assert np.array_equal(ref["db"], d["u"].astype(np.float64).reshape(-1, case.cout).sum(0))


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_normal_and_small_data(case):
    dn, ws = R.make_data(case, "normal")
    ds, ws2 = R.make_data(case, "small")
    assert ws == ws2 and abs(ws - np.sqrt(2.0 / (case.kh * case.kw * case.cin))) < 1e-7 * ws
    for name in dn:
        f = np.float32(1e-6) if name in ("u", "px") else np.float32(1.0)
        assert np.array_equal(ds[name], dn[name] * f), name
    # the magnitudes the "small" pass is about: u, px 1e-6, everything else O(1)
    assert 0.5e-6 < ds["u"].std() < 2e-6 and 0.5e-6 < ds["px"].std() < 2e-6
    assert all(0.5 < ds[k].std() < 2 for k in ("x", "w", "pw"))


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_case_is_in_the_branch_it_names(case):
    from mpgan_amd import train, train_ops
    cin, cout, kh, kw, s = case.launch
    stride = (s, s)
    fwd = "fc" if case.fc else "mfma" if train._mfma_ok(kh, kw, cout, stride) else "direct"
    dgrad = "mfma" if train._mfma_ok(kh, kw, cin, stride) and not case.fc else "valu"
    wgrad = "valu"
    if train_ops.wgrad_mfma_ok(kh, kw, stride) and not case.fc:
        wgrad = "ring" if kh == kw and kh in (3, 4, 5) else "row"      # wgrad_launches (csrc/mpgan_wgrad_mfma.hip)
    chunks = (len(range(0, cout, 128)) if fwd == "mfma" else 0, len(range(0, cin, 128)) if dgrad == "mfma" else 0)
    assert (fwd, dgrad, wgrad, chunks) == (case.fwd, case.dgrad, case.wgrad, case.chunks)
    if case.s2d:
        assert (case.kh, case.kw, case.stride) == (4, 4, 2) and case.h % 2 == 0 and case.w % 2 == 0
    if case.fc:
        assert (case.h, case.w, case.kh, case.kw) == (1, 1, 1, 1)


def test_the_list_reaches_every_branch():
    assert {c.fwd for c in R.CASES} == {"mfma", "direct", "fc"}
    assert {c.dgrad for c in R.CASES} == {"mfma", "valu"}
    assert {c.wgrad for c in R.CASES} == {"ring", "row", "valu"}
    assert any(c.chunks[0] > 1 for c in R.CASES) and any(c.chunks[1] > 1 for c in R.CASES)
    assert any(c.s2d for c in R.CASES) and any(c.stride == 2 and not c.s2d for c in R.CASES)
    assert any(c.kh % 2 == 0 and c.stride == 1 for c in R.CASES)
    assert len({c.name for c in R.CASES}) == len(R.CASES)


def test_f16f6_case_is_where_conv_prec_picks_f16f6():
    """forward (one launch of 128 output channels) and data gradient (136 = 128 + 8 of them over a 128-channel input) run
    at MPG_PREC_F16F6, no other case of the list does, and weight gradients never do"""
    from mpgan_amd import ops, train
    c = R.F16F6_CASE
    assert (c.kh, c.kw, c.cin, c.cout) == (4, 4, 136, 128)
    assert train._conv_prec(ops.PREC_F16F6, c.kh, c.kw, c.cin, c.cout) == ops.PREC_F16F6
    for c0 in range(0, c.cin, 128):
        assert train._conv_prec(ops.PREC_F16F6, c.kh, c.kw, c.cout, min(c.cin, c0 + 128) - c0) == ops.PREC_F16F6
    assert train._conv_prec(ops.PREC_F16X3, c.kh, c.kw, c.cin, c.cout) == ops.PREC_F16X3
    assert train._wgrad_prec(ops.PREC_F16F6) == ops.PREC_F16X3 and train._wgrad_prec(ops.PREC_F16X1) == ops.PREC_F16X1


@pytest.mark.parametrize("shape,stride", [((2, 5, 4, 3, 2, 4, 4), 1), ((2, 5, 7, 3, 2, 4, 4), 2), ((1, 4, 6, 2, 3, 4, 4), 2),
                                          ((1, 4, 5, 2, 3, 3, 3), 1), ((1, 5, 4, 2, 3, 3, 2), 2), ((2, 3, 3, 4, 2, 1, 1), 1)])
def test_reference_against_loop_convolution(shape, stride):
    """conv() against the definition in numpy loops: the 4x4 SAME pads (1 before / 2 after at stride 1; at stride 2 one
    before and one after on even sizes, 1 / 2 on odd ones), an odd filter and 1x1"""
    n, h, w, cin, cout, kh, kw = shape
    rng = np.random.default_rng(7 * h + w)
    x = rng.integers(-3, 4, size=(n, h, w, cin)).astype(np.float64)
    wt = rng.integers(-2, 3, size=(kh, kw, cin, cout)).astype(np.float64)
    got = R.conv(torch.tensor(x), torch.tensor(wt), stride).numpy()
    want = R.conv_loop(x, wt, stride)
    assert got.shape == want.shape == (n, -(-h // stride), -(-w // stride), cout)
    assert np.array_equal(got, want)


def _ints(rng, shape, m):
    return torch.tensor(rng.integers(-m, m + 1, size=shape).astype(np.float64))


@pytest.mark.parametrize("hw", [(8, 10), (2, 6)])
def test_strided4_as_3x3_forward(hw):
    from mpgan_amd.train import space_to_depth2, strided4_as_3x3
    rng = np.random.default_rng(hw[0])
    x, w = _ints(rng, (2, hw[0], hw[1], 3), 3), _ints(rng, (4, 4, 3, 5), 2)
    z, w3 = space_to_depth2(x), strided4_as_3x3(w)
    assert tuple(z.shape) == (2, hw[0] // 2, hw[1] // 2, 12) and tuple(w3.shape) == (3, 3, 12, 5)
    # channel (r*2+s)*C + c of z[Y, X] holds x[2Y+r, 2X+s, c]
    assert torch.equal(z[:, :, :, 1 * 6 + 0 * 3 + 2], x[:, 1::2, 0::2, 2])
    assert torch.equal(R.conv(z, w3, 1), R.conv(x, w, 2))


def test_strided4_as_3x3_carries_16_of_36_positions():
    from mpgan_amd.train import strided4_as_3x3
    w3 = strided4_as_3x3(torch.ones(4, 4, 1, 1, dtype=torch.float64))
    abrs = w3.reshape(3, 3, 2, 2)           # (a, b, r, s): 4 C = 4 channels at C = 1
    assert int((abrs != 0).sum()) == 16 and abrs.numel() == 36
    # tap 2a + r - 1 in 0..3: a = 0 holds r = 1 only, a = 1 both, a = 2 r = 0 only -- the same along the columns
    rows = torch.tensor([[0, 1], [1, 1], [1, 0]], dtype=torch.float64)
    assert torch.equal(abrs, torch.einsum("ar,bs->abrs", rows, rows))
    # every tap of the 4x4 filter lands in exactly one position
    w = torch.arange(1, 17, dtype=torch.float64).reshape(4, 4, 1, 1)
    assert sorted(strided4_as_3x3(w).flatten().tolist()) == [0.0] * 20 + [float(i) for i in range(1, 17)]


def test_strided4_as_3x3_first_and_second_derivatives():
    """autograd flows through the two helpers: every output of conv_triad_ref.derivatives with respect to the ORIGINAL
    x and w equals that of the stride-2 convolution, bit for bit (float64 integers)"""
    from mpgan_amd.train import space_to_depth2, strided4_as_3x3
    case = next(c for c in R.CASES if c.s2d)
    d, wscale = R.make_data(case, "exact")
    want = R.reference(case, "exact")
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k in R.LEAVES) for k, v in d.items()}
    got = R.derivatives(lambda x, w, b: R.conv(space_to_depth2(x), strided4_as_3x3(w) * wscale, 1) + b, t)
    for name in R.OUTPUTS:
        assert torch.equal(got[name].detach(), torch.tensor(want[name])), name
    for name in R.ZEROS:
        assert got[name] is None or not bool(got[name].any()), name


def test_mismatch_report():
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    assert R.mismatch_report(a, a.copy()) == ""
    assert R.mismatch_report(np.float32([0.0]), np.float32([-0.0])) == ""
    b = a.copy()
    b[1, 0, 2] *= 2
    b[1, 2, 3] += 1
    msg = R.mismatch_report(b, a, "dx")
    assert "dx: 2 of 24 values differ" in msg and "(1, 0, 2)" in msg and "ratio 2" in msg
    assert "shape" in R.mismatch_report(a[:1], a)
    assert "float32" in R.mismatch_report(a.astype(np.float64), a)
