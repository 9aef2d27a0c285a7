"""What test_advect_gpu.py relies on, proven without a GPU: the exact data of advect_ref.py gives results whose every term
is an integer at the case's power of two with the sum of |term| below 2^24 (so every fp32 partial sum, in any order, is
exact and the expectation is an fp32 number), the vectorised oracle agrees with its scalar loop on non-square grids, and
every case holds at least 16 pixels of each path it names.

Two properties of doClampComponent that follow from its own clipping are proven here too, because they decide what a
test of the kernel can see: truncating or flooring the look-up position gives the same clamped index (they differ only
below zero, where both are clipped to 0), and a neighbourhood without a fluid cell is rejected by `corrected < lo`
alone (lo is still float32(sys.maxsize)), with or without the test on the untouched bounds."""
import numpy as np
import pytest

import advect_ref as R
from oracle import advect as A

LIMIT = 2.0 ** 24
MIN_PIXELS = 16


def _integers(v, scale):
    v = np.asarray(v, np.float64) * scale
    return np.array_equal(v, np.round(v))


def _fp32(v):
    v = np.asarray(v)
    return np.array_equal(v.astype(np.float32).astype(np.float64), v.astype(np.float64))


@pytest.mark.parametrize("case", R.ADVECT_CASES, ids=repr)
def test_advect_data_is_exact(case):
    d, e = R.advect_data(case), R.advect_expect(case)
    src, g, flags = d["src"], d["g"], d["flags"]
    assert all(np.array_equal(v, np.round(v)) and v.dtype == np.float32 for v in d.values())
    assert set(np.unique(flags)) == {0.0, 1.0} and src.min() == 0 and src.max() == 7 and np.abs(g).max() == R.GMAX
    r = case.h // case.hv
    assert _integers(e["disp"], 4 * r) and _fp32(e["disp"])              # the 1/4 grid at hv == h, the 1/8 grid at hv == h/2
    mp, mm = R.sl_matrix(e["disp"], 1.0), R.sl_matrix(e["disp"], -1.0)
    assert _integers(mp, 2 ** 6) and _integers(mm, 2 ** 6)
    # the terms of forward, backward and corrected, and the sum of their magnitudes per output
    fwd_abs = R.apply_matrix(np.abs(mp), np.abs(src))
    bwd_abs = R.apply_matrix(np.abs(mm), fwd_abs)
    half = 0.5 * case.strength
    corr_abs = fwd_abs + half * (np.abs(src) + bwd_abs)
    assert fwd_abs.max() * 2 ** 6 < LIMIT and bwd_abs.max() * 2 ** 12 < LIMIT and corr_abs.max() * case.scale < LIMIT
    assert _integers(e["forward"], 2 ** 6) and _integers(e["backward"], 2 ** 12)
    assert _integers(e["corrected"], case.scale) and _integers(e["out"], case.scale)
    assert np.array_equal(R.apply_matrix(mp, src), e["forward"]) and np.array_equal(R.apply_matrix(mm, e["forward"]), e["backward"])
    # the scatter-adds of the two gradients: d source = g1 + SL^T(+v)[g - SL^T(-v)[g1]], g1 = keep * strength/2 * g
    g1_abs = e["keep"] * half * np.abs(g)
    dfwd_abs = np.abs(g) + R.apply_matrix(np.abs(mm), g1_abs, transpose=True)
    d2_abs = g1_abs + R.apply_matrix(np.abs(mp), dfwd_abs, transpose=True)
    d1_abs = R.apply_matrix(np.abs(mp), np.abs(g), transpose=True)
    assert d1_abs.max() * 2 ** 6 < LIMIT and d2_abs.max() * case.scale < LIMIT
    assert _integers(e["dsrc1"], 2 ** 6) and _integers(e["dsrc2"], case.scale)
    for name in ("forward", "backward", "corrected", "out", "keep", "dsrc1", "dsrc2"):
        assert _fp32(e[name]) and np.abs(e[name]).max() > 0, name
    # autograd of the restatement is the transposed matrices
    assert np.array_equal(e["dsrc1"], R.apply_matrix(mp, g, transpose=True))
    g1 = e["keep"] * half * g
    assert np.array_equal(e["dsrc2"], g1 + R.apply_matrix(mp, g - R.apply_matrix(mm, g1, transpose=True), transpose=True))


@pytest.mark.parametrize("case", R.ADVECT_CASES, ids=repr)
def test_advect_case_holds_its_paths(case):
    counts = R.clamp_paths(case)
    assert case.paths and all(counts[p] >= MIN_PIXELS for p in case.paths), counts
    assert counts["changed"] >= MIN_PIXELS                          # kept corrections that differ from `forward`
    e = R.advect_expect(case)
    assert (e["out"] != e["forward"]).sum() == counts["changed"]


@pytest.mark.parametrize("case", R.ADVECT_CASES[::2], ids=repr)
def test_clamp_identities_of_the_reference(case):
    d, e = R.advect_data(case), R.advect_expect(case)
    h = case.h
    p = A.positions(h, h) - e["disp"]
    differ = np.trunc(p) != np.floor(p)
    assert differ.any() and np.array_equal(np.clip(np.trunc(p), 0, h - 1), np.clip(np.floor(p), 0, h - 1))
    assert (p[differ] < 0).all()
    # without the comparison of lo / hi with their initial values
    n = case.n
    fluid = d["flags"][..., 0] < np.float32(A.THRESHOLD_FLAGS)
    i0 = np.clip(np.trunc(p).astype(np.int64), 0, h - 1)
    b = np.broadcast_to(np.arange(n)[:, None, None], i0.shape[:3])
    lo = np.full(i0.shape[:3], np.float32(A.BIG))
    hi = np.full(i0.shape[:3], np.float32(-A.BIG - 1))
    for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bb, ii, jj = (b, i0[..., 0], i0[..., 1]) if (di, dj) == (0, 0) else \
            (np.clip(b, 0, h - 1), np.clip(i0[..., 0] + di, 0, h - 1), np.clip(i0[..., 1] + dj, 0, h - 1))
        lo = np.where(fluid[bb, ii, jj], np.minimum(lo, d["src"][bb, ii, jj, 0]), lo)
        hi = np.where(fluid[bb, ii, jj], np.maximum(hi, d["src"][bb, ii, jj, 0]), hi)
    corr = e["corrected"][..., 0]
    assert np.array_equal((corr < lo) | (corr > hi), e["rejected"][..., 0])


@pytest.mark.parametrize("case", R.LOOKUP_CASES, ids=repr)
def test_lookup_data_is_exact(case):
    d, e = R.lookup_data(case), R.lookup_expect(case)
    n, h, w, c = case.shape
    assert _integers(d["disp"], 8) and np.abs(d["disp"]).max() == case.reach and _integers(d["src"], 1) and _integers(d["g"], 1)
    m = e["matrix"]
    assert _integers(m, R.LOOKUP_SCALE)
    assert R.apply_matrix(np.abs(m), np.abs(d["src"])).max() * R.LOOKUP_SCALE < LIMIT
    assert R.apply_matrix(np.abs(m), np.abs(d["g"]), transpose=True).max() * R.LOOKUP_SCALE < LIMIT
    assert _integers(e["out"], R.LOOKUP_SCALE) and _integers(e["dsrc"], R.LOOKUP_SCALE) and _fp32(e["out"]) and _fp32(e["dsrc"])
    assert np.array_equal(R.apply_matrix(m, d["src"]), e["out"])
    # the scalar loop, on a grid that is not square
    assert np.array_equal(A.semi_lagrange_loop(d["src"], np.float32(case.sign) * d["disp"], R.grid(h, w)), e["out"])
    counts = R.lookup_paths(d["disp"], case.sign)
    assert case.paths and all(counts[p] >= MIN_PIXELS for p in case.paths), counts
    # weights from the clamped indices are no partition of unity where the look-up leaves the grid
    assert (np.abs(m.sum(axis=2) - 1.0) > 0).sum() >= MIN_PIXELS


@pytest.mark.parametrize("case", R.VELOCITY_CASES, ids=repr)
def test_velocity_data(case):
    d, e = R.velocity_data(case), R.velocity_expect(case)
    assert e["disp"].shape == (case.n, case.h, case.w, 2) and case.n % 3 == 0
    if not case.exact:
        assert (case.h / case.hv) != 2 ** round(np.log2(case.h / case.hv))
        return
    up = max(case.h // case.hv, case.w // case.wv)
    assert _integers(d["vel"], 1) and _integers(e["disp"], case.scale) and _fp32(e["disp"])
    assert 2 * np.abs(d["vel"]).max() * up * case.scale < LIMIT            # two terms of at most max|v| * up each
    assert not e["disp"][1::3].any() and e["disp"][0::3].any() and e["disp"][2::3].any()
    # the successor past the last row / column is zero: those outputs are half the resized value
    assert e["disp"][0::3, -1, :, 0].any() and e["disp"][0::3, :, -1, 1].any()
    if case.path == "max_is_w":
        assert case.w // case.wv > case.h // case.hv


@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=repr)
def test_resample_data_is_exact(case):
    d, e = R.resample_data(case), R.resample_expect(case)
    n, h, w, c = case.shape
    counts = R.resample_paths(case)
    assert _integers(d["pos"], 8) and counts["furthest"] == 3.0
    m = e["matrix"]
    assert _integers(m, R.RESAMPLE_SCALE)
    assert R.apply_matrix(np.abs(m), np.abs(d["value"])).max() * R.RESAMPLE_SCALE < LIMIT
    assert R.apply_matrix(np.abs(m), np.abs(d["g"]), transpose=True).max() * R.RESAMPLE_SCALE < LIMIT
    assert _fp32(e["out"]) and _fp32(e["dvalue"]) and np.abs(e["out"]).max() > 0 and np.abs(e["dvalue"]).max() > 0
    assert np.array_equal(R.apply_matrix(m, d["value"]), e["out"])
    assert np.array_equal(R.apply_matrix(m, d["g"], transpose=True), e["dvalue"])
    assert all(counts[p] >= MIN_PIXELS for p in case.paths), counts
    if not case.paths:        # the one-row case: a handful of every kind
        assert all(counts[p] >= 3 for p in ("top", "bottom", "left", "right", "centre", "edge")), counts


@pytest.mark.parametrize("case", R.POSITIONS_CASES, ids=repr)
def test_positions_data(case):
    d, e = R.positions_data(case), R.positions_expect(case)
    assert e.shape == (R.POSITIONS_BATCH, case.n_out, case.n_out, 2)
    if not case.exact:
        return
    assert _integers(d["vel"], 1) and _integers(d["dt"], 4)
    assert _integers(e, case.scale) and _fp32(e) and np.abs(e).max() * case.scale < LIMIT
    yy, xx = np.meshgrid(np.arange(case.n_out) + 0.5, np.arange(case.n_out) + 0.5, indexing="ij")
    cells = np.stack([yy, xx], -1)
    assert np.array_equal(e[1::3], np.broadcast_to(cells, e[1::3].shape))             # dt == 0
    assert (e[0::3] != cells).any() and (e[2::3] != cells).any()
