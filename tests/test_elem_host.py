"""tests/elem_ref.py checked on the CPU: the references agree with the oracle and with float64 autograd, the exact data sets
are exact in float32 (the float64 and the float32 evaluation of a reference agree bit for bit), the adjoints are adjoints,
the cases are what their names claim, and every bound is positive and finite.  No GPU."""
import numpy as np
import pytest
import torch

import elem_ref as R
from oracle import ops as O

F32 = np.float32


def same_bits(a64, a32):
    assert a32.dtype == F32
    return np.array_equal(a64, a32.astype(np.float64))


def good_bound(b):
    return bool(np.all(np.isfinite(b)) and np.all(b > 0))


# ---------------------------------------------------------------------------------------------- resize
def test_float32_coordinate_edge_differs_from_exact_arithmetic():
    """2 -> 82 row 41 and 6 -> 74 column 37: the float32 coordinate lies below the integer that exact arithmetic gives, so
    nearest takes the source pixel before it and bilinear / bicubic a fraction near 1 instead of 0"""
    assert R.RESIZE_GEOMS[-1] == (2, 6, 82, 74)
    for (in_size, out_size, o), want, exact in zip(R.F32_EDGE, (0, 2), (1, 3)):
        assert o * in_size % out_size == 0 and o * in_size // out_size == exact
        assert O._nearest_index(out_size, in_size)[o] == want
        assert R.exact_floor_index(out_size, in_size)[o] == exact
        lo, frac = R.src_coord(out_size, in_size)
        assert lo[o] == want and 1 - 2.0 ** -21 < frac[o] < 1        # 0.99999994 and 2.9999998
        idx, _ = O.bicubic_taps_tf1(out_size, in_size)
        assert idx[o, 1] == want
    # and the outputs differ: a source whose rows and columns are all distinct
    x = np.arange(2 * 6, dtype=F32).reshape(1, 2, 6, 1) * F32(10.0)
    y = R.resize_nearest(x, 82, 74)
    exact = x[:, R.exact_floor_index(82, 2)][:, :, R.exact_floor_index(74, 6)]
    assert y[0, 41, 0, 0] != exact[0, 41, 0, 0] and y[0, 0, 37, 0] != exact[0, 0, 37, 0]
    assert np.sum(y != exact) == 74 + 82 - 1


@pytest.mark.parametrize("geom", R.RESIZE_GEOMS, ids=lambda g: "%dx%d-%dx%d" % g)
@pytest.mark.parametrize("c", R.RESIZE_C)
def test_resize_references_round_to_the_oracle(geom, c):
    h, w, oh, ow = geom
    x = R.resize_input(h, w, c, "normal")
    assert np.array_equal(R.resize_bilinear(x, oh, ow).astype(F32), O.resize_bilinear_tf1(x, oh, ow))
    assert np.array_equal(R.resize_bicubic(x, oh, ow).astype(F32), O.resize_bicubic_tf1(x, oh, ow))
    assert good_bound(R.bilinear_bound(x, oh, ow)) and good_bound(R.bicubic_bound(x, oh, ow))
    if (h, w) == (oh, ow):
        assert np.array_equal(R.resize_nearest(x, oh, ow), x) and np.array_equal(R.resize_bilinear(x, oh, ow), x)


@pytest.mark.parametrize("geom", R.BILINEAR_EXACT_GEOMS + [(1, 1, 5, 3)], ids=lambda g: "%dx%d-%dx%d" % g)
@pytest.mark.parametrize("c", R.RESIZE_C)
def test_bilinear_integer_data_is_exact_at_dyadic_ratios(geom, c):
    h, w, oh, ow = geom
    x = R.resize_input(h, w, c, "int")
    assert np.all(x == np.rint(x)) and np.abs(x).max() <= 64
    assert same_bits(R.resize_bilinear(x, oh, ow), R.resize_bilinear(x, oh, ow, F32))


@pytest.mark.parametrize("kind", ["row", "column"])
def test_bilinear_edge_input_is_one_rounded_product(kind):
    """every lerp of the edge case has a zero addend or a zero difference (so an FMA and a multiply-add agree), and the edge
    row / column holds the float below v where the exact-arithmetic coordinate would give v"""
    x = R.bilinear_edge_input(kind)
    taps, fy, fx = R._bilinear_taps(x, 82, 74)
    tl, tr, bl, br = taps
    assert np.all((tl == 0) | (tr == tl)) and np.all((bl == 0) | (br == bl))
    lx = fx[None, None, :, None]
    top, bot = tl + (tr - tl) * lx, bl + (br - bl) * lx
    assert top.dtype == F32 and np.all((top == 0) | (bot == top))
    y = R.resize_bilinear(x, 82, 74, F32)
    v = x[:, 1, 5, :]
    below = np.nextafter(v, F32(0))
    if kind == "row":
        assert np.array_equal(y[:, 41], np.broadcast_to(below[:, None, :], y[:, 41].shape)) and np.array_equal(y[:, 42, 0], v)
    else:
        assert np.all(y[:, :, 37] != v[:, None, :]) and np.all(np.abs(y[:, :, 37] / v[:, None, :] - 1) < 2.0 ** -21)
        assert np.array_equal(y[:, :, 38], np.broadcast_to(v[:, None, :], y[:, :, 38].shape))
    assert np.abs(y.astype(np.float64) - R.resize_bilinear(x, 82, 74)).max() <= 2.0 ** -24 * np.abs(v).max()


def test_bicubic_tie_geometry():
    """17 -> 347, output 344: the table offset depends on whether the coordinate is rounded to float32 before its fraction
    is taken (it is: mpgan.h), and the two offsets give weights far beyond the bound apart"""
    from fractions import Fraction
    in_size, out_size, o, off_rounded, off_unrounded = R.BICUBIC_TIE
    assert R.BICUBIC_TIE_GEOM == (in_size, 1, out_size, 1)
    lo, frac = R.src_coord(out_size, in_size)
    assert frac[o] * F32(1024) == F32(off_rounded - 0.5) and int(np.rint(frac[o] * F32(1024))) == off_rounded
    unrounded = Fraction(o) * Fraction(float(F32(in_size) / F32(out_size))) - int(lo[o])
    assert int(np.rint(F32(float(unrounded)) * F32(1024))) == off_unrounded
    lut = O._bicubic_lut()
    _, wt = O.bicubic_taps_tf1(out_size, in_size)
    assert wt[o, 1] == lut[2 * off_rounded] and abs(float(lut[2 * off_rounded]) - float(lut[2 * off_unrounded])) > 1e-4


def test_bicubic_abs_weight_sum_is_at_most_1_375():
    """Keys A = -0.75: sum |w| peaks at the half-way fraction, 1.375"""
    worst = 0.0
    for in_size, out_size in [(1024, 1024 * 1024 // 1024)] + [(g[0], g[2]) for g in R.RESIZE_GEOMS] + [(g[1], g[3]) for g in R.RESIZE_GEOMS]:
        worst = max(worst, float(R.bicubic_abs_weight_sums(out_size, in_size).max()))
    lut = O._bicubic_lut().astype(np.float64)
    table = max(abs(lut[2 * i + 1]) + abs(lut[2 * i]) + abs(lut[2 * (1024 - i)]) + abs(lut[2 * (1024 - i) + 1]) for i in range(1025))
    assert worst <= table <= 1.375 + 1e-6 and table >= 1.375 - 1e-6


@pytest.mark.parametrize("factors", R.NEAREST_BWD_FACTORS, ids=lambda f: "x%dx%d" % f)
@pytest.mark.parametrize("c", R.NEAREST_BWD_C)
def test_nearest_bwd_is_the_adjoint_and_exact(factors, c):
    n, h, w = R.NEAREST_BWD_SRC
    oh, ow = h * factors[0], w * factors[1]
    x, dy = R.ints(1, (n, h, w, c)), R.ints(2, (n, oh, ow, c))
    dx = R.resize_nearest_bwd(dy, h, w)
    assert np.sum(R.resize_nearest(x, oh, ow).astype(np.float64) * dy) == np.sum(x.astype(np.float64) * dx)
    assert same_bits(dx, R.resize_nearest_bwd(dy, h, w, F32))
    # integer factors: the sum of the fy x fx block
    block = dy.astype(np.float64).reshape(n, h, factors[0], w, factors[1], c).sum(axis=(2, 4))
    assert np.array_equal(dx, block)
    assert n * h * w * max(R.NEAREST_BWD_C) > 256


def test_nearest_bwd_adjoint_at_a_non_integer_ratio():
    x, dy = R.ints(3, (2, 2, 6, 3)), R.ints(4, (2, 82, 74, 3))
    assert np.sum(R.resize_nearest(x, 82, 74).astype(np.float64) * dy) == np.sum(x * R.resize_nearest_bwd(dy, 2, 6))


# ---------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("hw", R.AVG_POOL_HW, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("c", R.AVG_POOL_C)
def test_avg_pool_reference_adjoint_and_exactness(hw, c):
    h, w = hw
    x, dy = R.ints(5, (R.AVG_POOL_N, h, w, c)), R.ints(6, (R.AVG_POOL_N, h // 2, w // 2, c))
    y = R.avg_pool2(x)
    assert np.array_equal(y.astype(F32), O.avg_pool(x, 2, 2)) and same_bits(y, R.avg_pool2(x, F32))
    dx = R.avg_pool2_bwd(dy, h, w)
    assert same_bits(dx, R.avg_pool2_bwd(dy, h, w, F32))
    assert np.sum(y * dy) == np.sum(x.astype(np.float64) * dx)
    if h % 2:
        assert not dx[:, h - 1].any()
    if w % 2:
        assert not dx[:, :, w - 1].any()


@pytest.mark.parametrize("geom", R.MAX_POOL_GEOMS, ids=lambda g: "%s-k%d-s%d" % ("x".join(map(str, g[0])), g[1], g[2]))
def test_max_pool_arg_statements_agree_and_bwd_is_exact(geom):
    shape, k, s = geom
    n, h, w, c = shape
    for kind in R.MAX_POOL_DATA:
        x = R.max_pool_data(kind, shape)
        arg = R.max_pool_arg(x, k, s)
        if shape[0] * shape[3] * k * k <= 250 or kind == "ties":
            assert np.array_equal(arg, R.max_pool_arg_loop(x, k, s))
        y = R.max_pool(x, k, s)
        assert arg.shape == y.shape and arg.max() < k * k
        win = R._pool_windows(x, k, s)
        assert np.array_equal(np.take_along_axis(win, arg[None].astype(np.int64), axis=0)[0], y)
        if kind == "equal":
            assert not arg.any()
        if kind == "negative":
            assert y.max() < 0
        if kind == "ties" and k > 1:
            tied = (win == win.max(axis=0, keepdims=True)).sum(axis=0)
            assert (tied > 1).any()
        dy = R.ints(8, y.shape)
        dx = R.max_pool_bwd(dy, arg, h, w, k, s)
        assert same_bits(dx, R.max_pool_bwd(dy, arg, h, w, k, s, F32)) and dx.sum() == dy.astype(np.float64).sum()
    if (k, s) == (15, 15):
        assert y.shape[1:3] == (1, 1)
    if (k, s) == (5, 3) and h == 9:
        assert (h - k) % s != 0


# ---------------------------------------------------------------------------------------------- pixel norm
def test_pixel_norm_lane_groups():
    """largest power of two <= min(c, 64), restated here from the rule"""
    want = {1: 1, 2: 2, 3: 2, 5: 4, 31: 16, 32: 32, 33: 32, 64: 64, 65: 64, 100: 64, 128: 64, 200: 64}
    assert set(want) == set(R.PN_C)
    for c, lanes in want.items():
        assert R.pn_lanes(c) == lanes == max(p for p in (1, 2, 4, 8, 16, 32, 64) if p <= min(c, 64))
        # 37 pixels leave the last wave part-filled (with 64 lanes a pixel IS a wave); 1031 pixels fill more than one block,
        # the last of them in part
        assert ((37 * lanes) % 64 != 0 or lanes == 64) and 1031 * lanes > 256 and (1031 * lanes) % 256 != 0
    assert {R.pn_lanes(c) for c in R.PN_C} >= {1, 2, 32, 64} and max(R.PN_C) > 64


@pytest.mark.parametrize("c", R.PN_C)
def test_pixel_norm_references(c):
    for npix in (1, 37):
        x, dy = R.pn_data(npix, c)
        y = R.pixel_norm(x)
        assert np.array_equal(y.astype(F32), O.pixel_norm(x.reshape(1, 1, npix, c), float(F32(R.PN_EPS)))[0, 0])
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        yt = xt * torch.rsqrt((xt * xt).mean(dim=-1, keepdim=True) + float(F32(R.PN_EPS)))
        (dx,) = torch.autograd.grad(yt, [xt], torch.tensor(dy, dtype=torch.float64))
        ref = R.pixel_norm_bwd(dy, x)
        assert np.abs(ref - dx.numpy()).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
        assert good_bound(R.pixel_norm_bound(x)) and good_bound(R.pixel_norm_bwd_bound(dy, x))


def test_pixel_norm_zero_pixel():
    x = np.zeros((3, 5), dtype=F32)
    dy = R.normal(9, (3, 5))
    assert not R.pixel_norm(x).any()
    assert np.allclose(R.pixel_norm_bwd(dy, x), dy.astype(np.float64) / np.sqrt(np.float64(F32(1e-8))), rtol=1e-14)
    assert good_bound(R.pixel_norm_bound(x)) and good_bound(R.pixel_norm_bwd_bound(dy, x))


# ---------------------------------------------------------------------------------------------- minibatch stddev
@pytest.mark.parametrize("case", R.MBSTD_CASES, ids=lambda c: "n%d-g%d-%dx%dx%d" % c)
def test_mbstd_references(case):
    n, group, h, w, c = case
    x, dy = R.mbstd_data(case)
    y, stat = R.mbstd(x, group)
    assert np.array_equal(y.astype(F32), O.minibatch_stddev(x, group))
    yt, dx = R.mbstd_bwd(x, dy, group)
    assert np.abs(yt - y).max() <= 1e-13 * np.abs(y).max()
    assert good_bound(R.mbstd_stat_bound(x, group)) and good_bound(R.mbstd_bwd_bound(x, dy, group))
    g = min(group, n)
    if g == 1:
        assert np.allclose(stat, np.sqrt(1e-8), rtol=1e-12)
    if n // g > 1 and g > 1:
        assert np.abs(np.diff(stat)).min() > 0.1 * stat.max()      # stat[n % m] and stat[n / g] cannot be confused


def test_mbstd_case_table():
    n, group, h, w, c = R.MBSTD_CASES[0]
    assert -(-h * w * c // 1024) > 1 and -(-min(group, n) * h * w // 1024) > 1 and -(-h * w * c // 256) == 7
    assert R.MBSTD_CASES[1][1] > R.MBSTD_CASES[1][0]
    assert R.MBSTD_CASES[2][1] == 1 and R.MBSTD_CASES[3][0] == R.MBSTD_CASES[3][1] and R.MBSTD_CASES[4][4] == 1
    x, _ = R.mbstd_data(R.MBSTD_CASES[0], R.MBSTD_OFFSET)
    x0, _ = R.mbstd_data(R.MBSTD_CASES[0])
    assert x.min() > 900 and good_bound(R.mbstd_stat_bound(x, group))
    # the offset moves the statistic of the float32 inputs by less than their own rounding allows, 2^-14 relative to 1000
    assert np.abs(R.mbstd_stat(x, group)[0] / R.mbstd_stat(x0, group)[0] - 1).max() < 1e-4


# ---------------------------------------------------------------------------------------------- add_act, lerp, zoom, adjacent
@pytest.mark.parametrize("n", R.ELEM_N)
def test_add_act_and_lerp_references(n):
    a, b = R.special_values(n), R.normal(32, (n,))
    for bb in (None, b):
        for act in R.ACTS:
            v = a if bb is None else (a + bb).astype(F32)
            if act == "lrelu":      # the oracle's leak is the double 0.2, the C ABI's the float32 0.2
                assert np.allclose(R.add_act(a, bb, act), O.activation(v, act), rtol=2.0 ** -23, atol=0)
            else:
                assert np.array_equal(R.add_act(a, bb, act).astype(F32), O.activation(v, act))
            if act in ("lrelu", "tanh"):
                assert good_bound(R.add_act_bound(a, bb, act))
    assert np.all(R.add_act(a, None, "lrelu")[a == 0] == 0)
    assert np.all(np.abs(np.abs(R.add_act(a, None, "tanh")[np.abs(a) == 20]) - 1) < 2.0 ** -23)
    x, y = R.ints(33, (n,)), R.ints(34, (n,))
    for xx in (None, x):
        for t in R.LERP_T_EXACT + (1.7,):
            assert same_bits(R.lerp(xx, y, t), R.lerp(xx, y, t, F32))
        assert np.array_equal(R.lerp(xx, y, 1.7), y) and np.array_equal(R.lerp(xx, y, 1.0), y)
        assert np.array_equal(R.lerp(xx, y, 0.0), np.zeros(n) if xx is None else x)
        assert good_bound(R.lerp_bound(xx, R.normal(35, (n,)) + F32(3.0)))


@pytest.mark.parametrize("case", R.ZOOM_CASES, ids=lambda c: "%s-axis%d-x%s" % ("x".join(map(str, c[0])), c[1], c[2]))
def test_zoom_reference(case):
    shape, axis, factor = case
    v = R.normal(41, shape) + F32(0.25)
    ref, bound = R.zoom(v, axis, factor)
    assert np.array_equal(ref.astype(F32), O.zoom_axis_linear(v, axis, factor)) and good_bound(bound)
    n = shape[axis]
    if factor == 1:
        assert np.array_equal(ref, v)
    if n == 1:
        assert np.array_equal(ref, np.repeat(v, 4, axis=axis))
    if factor == 1.5:
        assert ref.shape[axis] == 9


def test_zoom_case_table():
    inner = [int(np.prod(s[a + 1:])) for s, a, _ in R.ZOOM_CASES]
    outer = [int(np.prod(s[:a])) for s, a, _ in R.ZOOM_CASES]
    assert 1 in inner and 1 in outer
    for n, f in ((1, 4), (2, 8), (6, 1), (6, 1.5)):
        assert {a for s, a, ff in R.ZOOM_CASES if s[a] == n and ff == f} == {0, 1, 2}


@pytest.mark.parametrize("s", R.ADJ_S)
@pytest.mark.parametrize("c", R.ADJ_C)
def test_add_adjacent_reference(s, c):
    x = R.normal(51, (s,) + R.ADJ_HW + (c,))
    full = R.add_adjacent(x)
    assert full.shape == (s,) + R.ADJ_HW + (c + 2,)
    assert not full[0, ..., c].any() and not full[-1, ..., c + 1].any()
    for i in range(s):
        assert np.array_equal(full[i, ..., :c], x[i])
        if i > 0:
            assert np.array_equal(full[i, ..., c], x[i - 1, ..., 0])
        if i + 1 < s:
            assert np.array_equal(full[i, ..., c + 1], x[i + 1, ..., 0])
    for off, cnt in R.adj_windows(s):
        assert np.array_equal(R.add_adjacent(x, off, cnt), full[off:off + cnt])
    if s == 6:
        assert (2, 3) in R.adj_windows(s)
