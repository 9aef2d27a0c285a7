"""The adjoints of the legacy-TF1 resizes (mpg_resize_bilinear_bwd / mpg_resize_bicubic_bwd, include/mpgan.h), restated from
the forward's taps and not from the kernels: numpy, float64 sums of float32 weights times float32 gradients.  Both resizes are
linear maps Y = R_h X R_w^T whose rows hold the taps of one output index, so dX = R_h^T dY R_w: every output sends
weight * dy to the (clamped) source index of each of its taps, along H and then along W.  No GPU imports:
test_resize_bwd_host.py checks this file on the CPU, test_resize_bwd_gpu.py holds the kernels against it.

The taps are those of tests/elem_ref.py and oracle/ops.py: the float32 source coordinate of elem_ref.src_coord with the
bilinear pair (i0, min(i0 + 1, in - 1)) weighted (1 - l, l) -- 1 - l rounded to float32, which is what
oracle.ops.resize_bilinear_tf1 returns for an impulse --, oracle.ops._nearest_index, and oracle.ops.bicubic_taps_tf1."""
import functools

import numpy as np

import elem_ref as E
from oracle import ops as O

F32 = np.float32
# (lo, hi): an output whose floor index is i0 reads the source indices i0 + lo .. i0 + hi before clamping
TAP_SPAN = {0: (0, 1), 2: (-1, 2)}


@functools.lru_cache(maxsize=None)
def axis_taps(out_size, in_size, method):
    """(idx [out, T] int64, wt [out, T] float32) of one axis: T = 2 bilinear, 1 nearest, 4 bicubic"""
    if method == 0:
        i0, l = E.src_coord(out_size, in_size)
        idx = np.stack([i0, np.minimum(i0 + 1, in_size - 1)], axis=1)
        wt = np.stack([F32(1) - l, l], axis=1).astype(F32)
    elif method == 1:
        idx = O._nearest_index(out_size, in_size)[:, None]
        wt = np.ones((out_size, 1), dtype=F32)
    elif method == 2:
        idx, wt = O.bicubic_taps_tf1(out_size, in_size)
    else:
        raise ValueError("resize method %r" % (method,))
    idx.setflags(write=False)
    wt.setflags(write=False)
    return idx, wt


def _adjoint(dy, h, w, method, dtype, absolute):
    n, oh, ow, c = dy.shape
    iy, wy = axis_taps(oh, h, method)
    ix, wx = axis_taps(ow, w, method)
    g = dy.astype(dtype)
    if absolute:
        g, wy, wx = np.abs(g), np.abs(wy), np.abs(wx)
    tmp = np.zeros((n, h, ow, c), dtype=dtype)
    for t in range(iy.shape[1]):
        np.add.at(tmp, (slice(None), iy[:, t]), g * wy[:, t].astype(dtype)[None, :, None, None])
    dx = np.zeros((n, h, w, c), dtype=dtype)
    for t in range(ix.shape[1]):
        np.add.at(dx, (slice(None), slice(None), ix[:, t]), tmp * wx[:, t].astype(dtype)[None, None, :, None])
    return dx


def resize_bwd(dy, h, w, method, dtype=np.float64):
    """dx [n, h, w, c] of y = resize_images(x, [oh, ow], method) for dy [n, oh, ow, c]; a source that no output reads gets 0"""
    return _adjoint(dy, h, w, method, dtype, False)


def max_addends(out_size, in_size, method):
    """the largest number of (output, tap) pairs that one source index of the axis collects"""
    idx, _ = axis_taps(out_size, in_size, method)
    return int(np.bincount(idx.ravel(), minlength=in_size).max())


def resize_bwd_bound(dy, h, w, method):
    """Every addend of a pass is one rounded product, every partial sum one rounded add: m_y roundings on the path along H,
    m_x along W, each acting on at most the sum of the |weight| |dy| behind it.  6 more for the weights themselves, as
    elem_ref.bicubic_bound takes them: two per axis for a float32 weight up to 2 ulp from the table (bilinear: the one
    rounding of 1 - l), and the two stores (tmp and dx)."""
    n, oh, ow, c = dy.shape
    m_y, m_x = max_addends(oh, h, method), max_addends(ow, w, method)
    return E.SLACK * (m_y + m_x + 6) * E.U * _adjoint(dy, h, w, method, np.float64, True) + E.TINY


def window(i, in_size, out_size, method):
    """[a, b]: the outputs of the axis that the kernel of source index i visits, in integer arithmetic.  With the exact
    e = floor(o * in / out), a tap of o can be i only if i - hi <= i0 <= i - lo (clamping only widens this at i = 0 and
    i = in - 1, where the window is cut at 0 and out - 1 anyway); the float32 i0 is within 1 of e, so e lies in
    [i - hi - 1, i - lo + 1], that is (i - hi - 1) * out / in <= o < (i - lo + 2) * out / in."""
    lo, hi = TAP_SPAN[method]
    a = max(0, -((-(i - hi - 1) * out_size) // in_size))
    b = min(out_size - 1, -((-(i - lo + 2) * out_size) // in_size) - 1)
    return a, b


def axis_indices(out_size, in_size, method):
    """the idx of axis_taps alone, vectorised (bicubic_taps_tf1 loops in Python and rebuilds its table on every call): the
    float32 floor of elem_ref.src_coord plus lo .. hi, clamped.  test_resize_bwd_host.py holds it against axis_taps"""
    lo, hi = TAP_SPAN[method]
    i0, _ = E.src_coord(out_size, in_size)
    return np.clip(i0[:, None] + np.arange(lo, hi + 1)[None, :], 0 if method == 2 else None, in_size - 1)


def window_misses(in_size, out_size, method):
    """the (i, o) pairs where output o has a tap on source i and lies outside window(i)"""
    idx = axis_indices(out_size, in_size, method)
    wins = [window(i, in_size, out_size, method) for i in range(in_size)]
    return [(int(i), o) for o in range(out_size) for i in set(idx[o].tolist()) if not wins[i][0] <= o <= wins[i][1]]
