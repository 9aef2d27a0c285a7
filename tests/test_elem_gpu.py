"""The resize, pooling, pixel-norm, minibatch-stddev, add_act / lerp, axis-zoom and add_adjacent kernels (mpgan_elem.hip,
mpgan_train_elem.hip) called through ops.*, train_ops.* and the autograd Functions of train.py, and held against the
references of tests/elem_ref.py (checked on the CPU by test_elem_host.py) at the edges of their index arithmetic.

* exact: np.array_equal, no exception list.  Nearest resize and max pool with their arg bytes on any data; bilinear resize,
  average pool, the three adjoints (nearest-resize, average-pool, max-pool backward) and lerp at t in {0, 0.5, 1} on integer
  data; add_act none / relu (one float32 add); add_adjacent; the feature channels of minibatch_stddev.
* bounded: |y - ref| <= bound for every element, the bound array from elem_ref.py (roundings x 2^-24 x magnitude x 2).
  Every such case prints "elem-error <case> <worst err / bound>"; profiles/r12/elem_errors.txt is their collection on an
  MI355X.  A ratio above 1 is a defect of the kernel or of the bound's derivation, never a reason for a larger factor."""
import numpy as np
import pytest
import torch

import elem_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)       # a copy: shared inputs are read-only


def _t_u8(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.uint8, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bounded(name, y, ref, bound):
    assert y.shape == ref.shape == bound.shape, (name, y.shape, ref.shape, bound.shape)
    ratio = R.worst(y, ref, bound)
    print("elem-error %-58s %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: worst err / bound %.3f at %s" % (
        name, ratio, np.unravel_index(np.argmax(np.abs(y - ref) / bound), y.shape))


def _geom_id(g):
    return "%dx%d-%dx%d" % g


@pytest.fixture(scope="module")
def ops(gpu_ops):
    return gpu_ops


@pytest.fixture(scope="module")
def tops(gpu_ops):
    from mpgan_amd import train_ops
    return train_ops


@pytest.fixture(scope="module")
def MpgError(gpu_ops):
    from mpgan_amd import _lib
    return _lib.MpgError


# ---------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("c", R.RESIZE_C)
@pytest.mark.parametrize("geom", R.RESIZE_GEOMS, ids=_geom_id)
def test_resize_nearest_exact(ops, geom, c):
    h, w, oh, ow = geom
    x = R.resize_input(h, w, c, "normal")
    assert np.array_equal(_np(ops.resize_nearest(_t(x), oh, ow)), R.resize_nearest(x, oh, ow))
    assert np.array_equal(_np(ops.resize_images(_t(x), oh, ow, 1)), R.resize_nearest(x, oh, ow))


@pytest.mark.parametrize("c", R.RESIZE_C)
@pytest.mark.parametrize("geom", R.RESIZE_GEOMS, ids=_geom_id)
def test_resize_bilinear_bounded(ops, geom, c):
    h, w, oh, ow = geom
    x = R.resize_input(h, w, c, "normal")
    y = _np(ops.resize_images(_t(x), oh, ow, 0))
    _bounded("bilinear %s c%d" % (_geom_id(geom), c), y, R.resize_bilinear(x, oh, ow), R.bilinear_bound(x, oh, ow))


@pytest.mark.parametrize("c", R.RESIZE_C)
@pytest.mark.parametrize("geom", R.BILINEAR_EXACT_GEOMS + [(1, 1, 5, 3)], ids=_geom_id)
def test_resize_bilinear_exact_on_integers(ops, geom, c):
    h, w, oh, ow = geom
    x = R.resize_input(h, w, c, "int")
    assert np.array_equal(_np(ops.resize_bilinear(_t(x), oh, ow)), R.resize_bilinear(x, oh, ow, F32))


@pytest.mark.parametrize("kind", ["row", "column"])
def test_resize_bilinear_float32_coordinate_edge_exact(ops, kind):
    """2x6 -> 82x74 on data whose every lerp has a zero addend or a zero difference (elem_ref.bilinear_edge_input), so that
    each output is ONE rounded product whatever the contraction: output row 41 (column 37) is v * 0.99999994 (0.99999976)
    rounded, the float below v, and not the v that a coordinate taken in exact arithmetic gives"""
    x = R.bilinear_edge_input(kind)
    want = R.resize_bilinear(x, 82, 74, F32)
    y = _np(ops.resize_bilinear(_t(x), 82, 74))
    assert np.array_equal(y, want)


@pytest.mark.parametrize("c", R.RESIZE_C)
@pytest.mark.parametrize("geom", R.RESIZE_GEOMS + [R.BICUBIC_TIE_GEOM], ids=_geom_id)
def test_resize_bicubic_bounded(ops, geom, c):
    h, w, oh, ow = geom
    x = R.resize_input(h, w, c, "normal")
    y = _np(ops.resize_images(_t(x), oh, ow, 2))
    _bounded("bicubic %s c%d" % (_geom_id(geom), c), y, R.resize_bicubic(x, oh, ow), R.bicubic_bound(x, oh, ow))


@pytest.mark.parametrize("c", R.NEAREST_BWD_C)
@pytest.mark.parametrize("factors", R.NEAREST_BWD_FACTORS, ids=lambda f: "x%dx%d" % f)
def test_resize_nearest_bwd_exact(tops, factors, c):
    from mpgan_amd.train import ResizeNearestFn
    n, h, w = R.NEAREST_BWD_SRC
    oh, ow = h * factors[0], w * factors[1]
    dy = R.ints(2, (n, oh, ow, c))
    want = R.resize_nearest_bwd(dy, h, w)
    assert np.array_equal(_np(tops.resize_nearest_bwd(_t(dy), h, w)), want)
    x = _t(R.ints(1, (n, h, w, c))).requires_grad_(True)
    (dx,) = torch.autograd.grad(ResizeNearestFn.apply(x, oh, ow), [x], _t(dy))
    assert np.array_equal(_np(dx), want)


def test_resize_nearest_bwd_refuses_a_non_integer_factor(tops, MpgError):
    with pytest.raises(MpgError):
        tops.resize_nearest_bwd(_t(R.ints(2, (2, 4, 5, 1))), 3, 5)


# ---------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("c", R.AVG_POOL_C)
@pytest.mark.parametrize("hw", R.AVG_POOL_HW, ids=lambda s: "%dx%d" % s)
def test_avg_pool_forward_backward_exact(ops, tops, hw, c):
    h, w = hw
    x, dy = R.ints(5, (R.AVG_POOL_N, h, w, c)), R.ints(6, (R.AVG_POOL_N, h // 2, w // 2, c))
    assert np.array_equal(_np(ops.avg_pool2(_t(x))), R.avg_pool2(x))
    dx = _np(tops.avg_pool2_bwd(_t(dy), h, w))
    assert np.array_equal(dx, R.avg_pool2_bwd(dy, h, w))
    if (h, w) == (7, 9):
        assert not dx[:, 6].any() and not dx[:, :, 8].any()


@pytest.mark.parametrize("c", R.AVG_POOL_C)
def test_avg_pool_second_derivative_exact(ops, c):
    """AvgPoolFn on 7x9: the gradient (zero in the dropped row and column), and the gradient of that gradient with respect
    to dy, which is the pool again"""
    from mpgan_amd.train import AvgPoolFn
    n, h, w = R.AVG_POOL_N, 7, 9
    x, dy, gg = R.ints(5, (n, h, w, c)), R.ints(6, (n, 3, 4, c)), R.ints(7, (n, h, w, c))
    xt, dyt = _t(x).requires_grad_(True), _t(dy).requires_grad_(True)
    y = AvgPoolFn.apply(xt)
    (dx,) = torch.autograd.grad(y, [xt], dyt, create_graph=True)
    (g_dy,) = torch.autograd.grad(dx, [dyt], _t(gg))
    assert np.array_equal(_np(y), R.avg_pool2(x))
    assert np.array_equal(_np(dx), R.avg_pool2_bwd(dy, h, w))
    assert np.array_equal(_np(g_dy), R.avg_pool2(gg))


@pytest.mark.parametrize("geom", R.MAX_POOL_GEOMS, ids=lambda g: "%s-k%d-s%d" % ("x".join(map(str, g[0])), g[1], g[2]))
def test_max_pool_forward_arg_backward_exact(ops, tops, geom):
    from mpgan_amd.train import MaxPoolFn
    shape, k, s = geom
    n, h, w, c = shape
    for kind in R.MAX_POOL_DATA:
        x = R.max_pool_data(kind, shape)
        want, want_arg = R.max_pool(x, k, s), R.max_pool_arg(x, k, s)
        y, arg = ops.max_pool(_t(x), k, s, want_arg=True)
        assert np.array_equal(_np(y), want), kind
        assert np.array_equal(_np(arg), want_arg), kind
        assert np.array_equal(_np(ops.max_pool(_t(x), k, s)), want), kind
        dy = R.ints(8, want.shape)
        want_dx = R.max_pool_bwd(dy, want_arg, h, w, k, s)
        assert np.array_equal(_np(tops.max_pool_bwd(_t(dy), _t_u8(want_arg), h, w, k, s)), want_dx), kind
        xt = _t(x).requires_grad_(True)
        (dx,) = torch.autograd.grad(MaxPoolFn.apply(xt, k, s), [xt], _t(dy))
        assert np.array_equal(_np(dx), want_dx), kind


def test_max_pool_refuses_bad_windows(ops, MpgError):
    x = _t(R.normal(1, (1, 17, 17, 2)))
    with pytest.raises(MpgError):
        ops.max_pool(x, 16, 1)
    with pytest.raises(MpgError):
        ops.max_pool(_t(R.normal(1, (1, 4, 9, 2))), 5, 1)


# ---------------------------------------------------------------------------------------------- pixel norm
@pytest.mark.parametrize("npix", R.PN_NPIX)
@pytest.mark.parametrize("c", R.PN_C, ids=lambda c: "c%d-lanes%d" % (c, R.pn_lanes(c)))
def test_pixel_norm_forward_backward_bounded(ops, c, npix):
    from mpgan_amd.train import PixelNormFn
    x, dy = R.pn_data(npix, c)
    xt = _t(x).requires_grad_(True)
    y = PixelNormFn.apply(xt, R.PN_EPS)
    (dx,) = torch.autograd.grad(y, [xt], _t(dy))
    name = "c%d npix%d" % (c, npix)
    _bounded("pixel_norm " + name, _np(y), R.pixel_norm(x), R.pixel_norm_bound(x))
    _bounded("pixel_norm_bwd " + name, _np(dx), R.pixel_norm_bwd(dy, x), R.pixel_norm_bwd_bound(dy, x))


def test_pixel_norm_zero_pixel(ops, tops):
    """eps = 1e-8 alone under the root: forward 0, backward dy * rsqrt(eps)"""
    x, dy = R.pn_data(5, 5)
    x[2] = 0
    y = _np(ops.pixel_norm(_t(x), 1e-8))
    dx = _np(tops.pixel_norm_bwd(_t(dy), _t(x), 1e-8))
    assert not y[2].any()
    _bounded("pixel_norm zero-pixel", y, R.pixel_norm(x, 1e-8), R.pixel_norm_bound(x, 1e-8))
    _bounded("pixel_norm_bwd zero-pixel", dx, R.pixel_norm_bwd(dy, x, 1e-8), R.pixel_norm_bwd_bound(dy, x, 1e-8))
    assert np.all(np.abs(dx[2] / dy[2]) > 9.9e3)


# ---------------------------------------------------------------------------------------------- minibatch stddev
def _mbstd_forward_check(name, y, x, group):
    n, c = x.shape[0], x.shape[3]
    ref, stat = R.mbstd(x, group)
    assert np.array_equal(y[..., :c], x), name
    bound = R.mbstd_stat_bound(x, group)
    m = stat.shape[0]
    _bounded("mbstd stat " + name, y[..., c], ref[..., c],
             np.broadcast_to(bound[np.arange(n) % m][:, None, None], y.shape[:3]))


@pytest.mark.parametrize("case", R.MBSTD_CASES, ids=lambda c: "n%d-g%d-%dx%dx%d" % c)
def test_minibatch_stddev_forward_backward(ops, case):
    from mpgan_amd.train import MinibatchStddevFn
    n, group, h, w, c = case
    name = "n%d g%d %dx%dx%d" % case
    x, dy = R.mbstd_data(case)
    xt = _t(x).requires_grad_(True)
    y = MinibatchStddevFn.apply(xt, group)
    (dx,) = torch.autograd.grad(y, [xt], _t(dy))
    _mbstd_forward_check(name, _np(y), x, group)
    _, want_dx = R.mbstd_bwd(x, dy, group)
    _bounded("mbstd bwd " + name, _np(dx), want_dx, R.mbstd_bwd_bound(x, dy, group))


def test_minibatch_stddev_large_common_offset(ops):
    """1000 added to every input: the statistic of the float32 inputs stays within its bound (the two-pass variance)"""
    case = R.MBSTD_CASES[0]
    x, _ = R.mbstd_data(case, R.MBSTD_OFFSET)
    _mbstd_forward_check("n%d g%d %dx%dx%d offset 1000" % case, _np(ops.minibatch_stddev(_t(x), case[1])), x, case[1])


def test_minibatch_stddev_refuses_an_indivisible_batch(ops, tops, MpgError):
    x = _t(R.normal(1, (6, 3, 3, 2)))
    with pytest.raises(MpgError):
        ops.minibatch_stddev(x, 4)
    with pytest.raises(MpgError):
        tops.minibatch_stddev_bwd(_t(R.normal(2, (6, 3, 3, 3))), x, 4)


# ---------------------------------------------------------------------------------------------- add_act, lerp
@pytest.mark.parametrize("with_b", [False, True], ids=["b_null", "b_given"])
@pytest.mark.parametrize("n", R.ELEM_N)
def test_add_act(ops, n, with_b):
    a = R.special_values(n)
    b = R.normal(32, (n,)) if with_b else None
    bt = _t(b) if with_b else None
    for act in R.ACTS:
        y = _np(ops.add_act(_t(a), bt, act, R.LEAK))
        ref = R.add_act(a, b, act)
        if act in (None, "relu"):
            assert np.array_equal(y, ref), act
        else:
            _bounded("add_act %s n%d %s" % (act, n, "b" if with_b else "-"), y, ref, R.add_act_bound(a, b, act))
        if not with_b:
            if act == "lrelu":
                assert np.all(y[a == 0] == 0)
            if act == "tanh":
                assert np.all(np.abs(np.abs(y[np.abs(a) == 20]) - 1) <= 2.0 ** -23)
                assert np.array_equal(np.sign(y[np.abs(a) == 20]), np.sign(a[np.abs(a) == 20]))


@pytest.mark.parametrize("with_x", [False, True], ids=["x_null", "x_given"])
@pytest.mark.parametrize("n", R.ELEM_N)
def test_lerp(tops, n, with_x):
    from mpgan_amd.train import LerpFn
    xi, yi = (R.ints(33, (n,)) if with_x else None), R.ints(34, (n,))
    xr, yr = (R.normal(35, (n,)) if with_x else None), R.normal(36, (n,))
    for t in R.LERP_T_EXACT + (1.7,):
        y = _np(tops.lerp(_t(xi) if with_x else None, _t(yi), t))
        assert np.array_equal(y, R.lerp(xi, yi, t)), t
    assert np.array_equal(_np(LerpFn.apply(_t(xi) if with_x else None, _t(yi), 0.5)), R.lerp(xi, yi, 0.5))
    for t in R.LERP_T:
        y = _np(tops.lerp(_t(xr) if with_x else None, _t(yr), t))
        _bounded("lerp t%.1f n%d %s" % (t, n, "x" if with_x else "-"), y, R.lerp(xr, yr, t), R.lerp_bound(xr, yr))
    assert np.array_equal(_np(tops.lerp(_t(xr) if with_x else None, _t(yr), 1.7)),
                          _np(tops.lerp(_t(xr) if with_x else None, _t(yr), 1.0)))


# ---------------------------------------------------------------------------------------------- axis zoom, add_adjacent
@pytest.mark.parametrize("case", R.ZOOM_CASES, ids=lambda c: "%s-axis%d-x%s" % ("x".join(map(str, c[0])), c[1], c[2]))
def test_axis_zoom(ops, case):
    shape, axis, factor = case
    v = R.normal(41, shape) + F32(0.25)
    y = _np(ops.axis_zoom_linear(_t(v), axis, factor))
    ref, bound = R.zoom(v, axis, factor)
    _bounded("axis_zoom %s axis%d x%s" % ("x".join(map(str, shape)), axis, factor), y, ref, bound)
    if factor == 1:
        assert np.array_equal(y, v)
    if shape[axis] == 1:
        assert np.array_equal(y, np.repeat(v, 4, axis=axis))


@pytest.mark.parametrize("c", R.ADJ_C)
@pytest.mark.parametrize("s", R.ADJ_S)
def test_add_adjacent_exact(ops, s, c):
    x = R.normal(51, (s,) + R.ADJ_HW + (c,))
    assert np.array_equal(_np(ops.add_adjacent(_t(x))), R.add_adjacent(x))
    for off, cnt in R.adj_windows(s):
        assert np.array_equal(_np(ops.add_adjacent(_t(x), off, cnt)), R.add_adjacent(x, off, cnt)), (off, cnt)
