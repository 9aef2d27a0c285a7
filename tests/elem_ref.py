"""Plain references, per-element error bounds and the case tables for the resize, pooling, pixel-norm, minibatch-stddev,
add_act / lerp, axis-zoom and add_adjacent kernels (mpgan_elem.hip, mpgan_train_elem.hip), written from include/mpgan.h and
oracle/ops.py and not from the kernels.  numpy, float64 arithmetic on float32 inputs; what the header takes in float32 (the
resize source coordinate float32(o) * (float32(in) / float32(out)), its floor and fraction, the bicubic table offset
rint(frac * 1024)) is taken in float32 here too.  No GPU imports: test_elem_host.py checks this file on the CPU,
test_elem_gpu.py holds the kernels against it.

Bounds.  Next to every reference that is not exact stands a function that returns the bound ARRAY: the number of float32
roundings on the path, times U = 2^-24, times the magnitude each rounding acts on (taken from the float64 reference), times
SLACK = 2 (contraction to FMA and a 1-ulp rsqrtf are allowed), plus TINY = 2^-126 (a denormal result may be flushed).  The
GPU test asserts |y - ref| <= bound elementwise and prints the worst err / bound of the case."""
import functools
import math

import numpy as np

from oracle import multipass as MP
from oracle import ops as O

F32 = np.float32
U = 2.0 ** -24
SLACK = 2.0
TINY = 2.0 ** -126


def ints(seed, shape, lo=-64, hi=64):
    """integers in [lo, hi] as float32: sums, differences and dyadic fractions of them are exact"""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(F32)


def normal(seed, shape, scale=1.0, shift=0.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale + shift).astype(F32)


def worst(y, ref, bound):
    """max over the elements of |y - ref| / bound"""
    err = np.abs(np.asarray(y, np.float64) - np.asarray(ref, np.float64))
    return float(np.max(err / bound)) if err.size else 0.0


# ---------------------------------------------------------------------------------------------- resize
# h, w -> oh, ow; n = 2, c in {1, 3}; every method runs every geometry
RESIZE_GEOMS = [
    (8, 8, 16, 16),
    (5, 7, 20, 14),
    (6, 6, 9, 15),
    (9, 6, 6, 4),       # down, non-integer
    (8, 8, 4, 2),       # down, dyadic
    (8, 3, 3, 8),
    (7, 5, 7, 5),       # identity
    (1, 1, 5, 3),
    (4, 1, 1, 4),
    (2, 6, 82, 74),     # float32 coordinate below an integer: row 41 takes source row 0, column 37 source column 2
]
RESIZE_N = 2
RESIZE_C = (1, 3)
# dyadic ratios (x2; /2 and /4; identity; x4 and x8): with integer data every intermediate of the bilinear lerps is exact
BILINEAR_EXACT_GEOMS = [(8, 8, 16, 16), (8, 8, 4, 2), (7, 5, 7, 5), (3, 5, 12, 40)]
# bicubic only: output row 344 of 347 over 17 has the float32 fraction 873.5 / 1024, a tie that rint sends to table offset
# 874; the fraction of the UNROUNDED product float32(344) * float32(17 / 347) lies below the tie and gives offset 873
BICUBIC_TIE_GEOM = (17, 1, 347, 1)
BICUBIC_TIE = (17, 347, 344, 874, 873)
F32_EDGE = ((2, 82, 41), (6, 74, 37))       # (in, out, o): float32(o) * (float32(in) / float32(out)) < o * in / out, an integer


def src_coord(out_size, in_size):
    """the float32 source coordinate of mpgan.h: (floor as int64, fraction as float32, both exact)"""
    scale = F32(in_size) / F32(out_size)
    s = np.arange(out_size, dtype=F32) * scale
    lo = np.floor(s)
    return lo.astype(np.int64), (s - lo).astype(F32)


def exact_floor_index(out_size, in_size):
    """what exact rational arithmetic would take: floor(o * in / out)"""
    return np.minimum(np.arange(out_size, dtype=np.int64) * in_size // out_size, in_size - 1)


def resize_nearest(x, oh, ow):
    return O.resize_nearest_tf1(x, oh, ow)


def _bilinear_taps(x, oh, ow):
    y0, fy = src_coord(oh, x.shape[1])
    x0, fx = src_coord(ow, x.shape[2])
    y1 = np.minimum(y0 + 1, x.shape[1] - 1)
    x1 = np.minimum(x0 + 1, x.shape[2] - 1)
    taps = [x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]]
    return taps, fy, fx


def resize_bilinear(x, oh, ow, dtype=np.float64):
    """tl + (tr - tl) lx, bl + (br - bl) lx, top + (bot - top) ly; every operation rounded to `dtype`"""
    taps, fy, fx = _bilinear_taps(x, oh, ow)
    tl, tr, bl, br = [t.astype(dtype) for t in taps]
    lx = fx.astype(dtype)[None, None, :, None]
    ly = fy.astype(dtype)[None, :, None, None]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    return top + (bot - top) * ly


def bilinear_edge_input(kind):
    """2 x 6 sources for the 2x6 -> 82x74 edge on which every lerp has a zero addend or a zero difference, so that an output
    is one rounded product, contracted or not.  "row": row 0 zero, row 1 a value per (sample, channel), constant along w;
    output row 41 is v * 0.99999994 rounded.  "column": columns 0..2 zero, columns 3..5 v, constant along h; output column
    37 is v * 0.99999976 rounded.  A coordinate taken in exact arithmetic gives v itself in both places."""
    v = (np.abs(normal(23, (RESIZE_N, 1, 1, 3))) + F32(0.5)).astype(F32) * np.array([1, -1, 1], dtype=F32)
    x = np.zeros((RESIZE_N, 2, 6, 3), dtype=F32)
    if kind == "row":
        x[:, 1:2, :, :] = v
    else:
        x[:, :, 3:, :] = v
    return x


def bilinear_bound(x, oh, ow):
    """three lerps of two roundings each, acting on at most the largest of the four taps"""
    taps, _, _ = _bilinear_taps(np.abs(x.astype(np.float64)), oh, ow)
    return SLACK * 6 * U * np.maximum(np.maximum(taps[0], taps[1]), np.maximum(taps[2], taps[3])) + TINY


def resize_bicubic(x, oh, ow):
    """oracle.ops.resize_bicubic_tf1 without its final rounding: along W with the table's float32 weights, then along H"""
    iy, wy = O.bicubic_taps_tf1(oh, x.shape[1])
    ix, wx = O.bicubic_taps_tf1(ow, x.shape[2])
    x64 = x.astype(np.float64)
    tmp = np.zeros((x.shape[0], x.shape[1], ow, x.shape[3]))
    for t in range(4):
        tmp += x64[:, :, ix[:, t], :] * wx[:, t].astype(np.float64)[None, None, :, None]
    out = np.zeros((x.shape[0], oh, ow, x.shape[3]))
    for t in range(4):
        out += tmp[:, iy[:, t], :, :] * wy[:, t].astype(np.float64)[None, :, None, None]
    return out


def bicubic_abs_weight_sums(out_size, in_size):
    _, wt = O.bicubic_taps_tf1(out_size, in_size)
    return np.abs(wt.astype(np.float64)).sum(axis=1)


def bicubic_bound(x, oh, ow):
    """16 products, 15 adds and float32 weights up to 2 ulp from the table: 40 U (sum |wy|) (sum |wx|) max |tap|"""
    iy, _ = O.bicubic_taps_tf1(oh, x.shape[1])
    ix, _ = O.bicubic_taps_tf1(ow, x.shape[2])
    ax = np.abs(x.astype(np.float64))
    big = np.zeros((x.shape[0], oh, ow, x.shape[3]))
    for r in range(4):
        for t in range(4):
            big = np.maximum(big, ax[:, iy[:, r]][:, :, ix[:, t]])
    sy = bicubic_abs_weight_sums(oh, x.shape[1])[None, :, None, None]
    sx = bicubic_abs_weight_sums(ow, x.shape[2])[None, None, :, None]
    return SLACK * 40 * U * sy * sx * big + TINY


# nearest-resize backward: (fy, fx) on 3 x 5 sources, n = 2, c in {1, 12}; 2 * 3 * 5 * 12 = 360 elements need two blocks
NEAREST_BWD_FACTORS = [(1, 1), (1, 3), (2, 1), (4, 2), (8, 8)]
NEAREST_BWD_SRC = (2, 3, 5)
NEAREST_BWD_C = (1, 12)


def resize_nearest_bwd(dy, h, w, dtype=np.float64):
    """the adjoint of resize_nearest: every output pixel sends its dy to the source pixel it was read from"""
    n, oh, ow, c = dy.shape
    iy = O._nearest_index(oh, h)
    ix = O._nearest_index(ow, w)
    dx = np.zeros((n, h, w, c), dtype=dtype)
    np.add.at(dx, (slice(None), iy[:, None], ix[None, :]), dy.astype(dtype))
    return dx


# ---------------------------------------------------------------------------------------------- pooling
AVG_POOL_HW = [(2, 2), (7, 9), (8, 5), (6, 6), (3, 2)]
AVG_POOL_N = 2
AVG_POOL_C = (1, 5, 8)


def avg_pool2(x, dtype=np.float64):
    """tf.nn.avg_pool 2 x 2 VALID: a last odd row or column is dropped"""
    n, h, w, c = x.shape
    oh, ow = h // 2, w // 2
    xd = x.astype(dtype)
    acc = np.zeros((n, oh, ow, c), dtype=dtype)
    for dy in range(2):
        for dx in range(2):
            acc += xd[:, dy:dy + 2 * oh:2, dx:dx + 2 * ow:2, :]
    return acc * dtype(0.25)


def avg_pool2_bwd(dy, h, w, dtype=np.float64):
    """the adjoint: a quarter of dy to each of the four pixels of its window, zero in a dropped row or column"""
    n, oh, ow, c = dy.shape
    dx = np.zeros((n, h, w, c), dtype=dtype)
    dx[:, :2 * oh, :2 * ow, :] = dtype(0.25) * np.repeat(np.repeat(dy.astype(dtype), 2, axis=1), 2, axis=2)
    return dx


MAX_POOL_SHAPES = [(2, 9, 11, 5), (1, 15, 17, 3)]
MAX_POOL_KS = [(1, 1), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (5, 3)]
# (15, 15) on 1 x 15 x 17 x 3 only: one window row
MAX_POOL_GEOMS = [(sh, k, s) for sh in MAX_POOL_SHAPES for k, s in MAX_POOL_KS] + [((1, 15, 17, 3), 15, 15)]
MAX_POOL_DATA = ("random", "equal", "negative", "ties")


def max_pool_data(kind, shape):
    if kind == "random":
        return normal(101, shape)
    if kind == "equal":
        return np.full(shape, 0.75, dtype=F32)
    if kind == "negative":
        return (-np.abs(normal(102, shape)) - F32(0.5)).astype(F32)
    if kind == "ties":
        # rows 1..6, columns 2..8 hold one value above everything else: windows inside, across and outside the block
        x = (normal(103, shape) * F32(0.1)).astype(F32)
        x[:, 1:7, 2:9, :] = F32(3.0)
        return x
    raise ValueError(kind)


def _pool_windows(x, k, s):
    n, h, w, c = x.shape
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    return np.stack([x[:, dy:dy + (oh - 1) * s + 1:s, dx:dx + (ow - 1) * s + 1:s, :] for dy in range(k) for dx in range(k)])


def max_pool(x, k, s):
    return O.max_pool(x, k, s)


def max_pool_arg(x, k, s):
    """window position dy * k + dx of the first maximum in scan order (numpy.argmax returns the first)"""
    return np.argmax(_pool_windows(x, k, s), axis=0).astype(np.uint8)


def max_pool_arg_loop(x, k, s):
    """the same as the scan it describes: a later element wins only when it is strictly greater"""
    n, h, w, c = x.shape
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    arg = np.zeros((n, oh, ow, c), dtype=np.uint8)
    for b in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for ch in range(c):
                    best, at = x[b, s * oy, s * ox, ch], 0
                    for dy in range(k):
                        for dx in range(k):
                            v = x[b, s * oy + dy, s * ox + dx, ch]
                            if v > best:
                                best, at = v, dy * k + dx
                    arg[b, oy, ox, ch] = at
    return arg


def max_pool_bwd(dy, arg, h, w, k, s, dtype=np.float64):
    """every output sends dy to its arg position; overlapping windows add"""
    n, oh, ow, c = dy.shape
    b, oy, ox, ch = np.meshgrid(np.arange(n), np.arange(oh), np.arange(ow), np.arange(c), indexing="ij")
    a = arg.astype(np.int64)
    dx = np.zeros((n, h, w, c), dtype=dtype)
    np.add.at(dx, (b, s * oy + a // k, s * ox + a % k, ch), dy.astype(dtype))
    return dx


# ---------------------------------------------------------------------------------------------- pixel norm
PN_C = (1, 2, 3, 5, 31, 32, 33, 64, 65, 100, 128, 200)
PN_NPIX = (1, 37, 1031)
PN_EPS = 1e-8


def pn_lanes(c):
    """lanes that share one pixel: the largest power of two <= min(c, 64) (mpgan.h, mpg_pixel_norm)"""
    lanes = 1
    while lanes * 2 <= min(c, 64):
        lanes *= 2
    return lanes


def pn_sum_roundings(c):
    """roundings of one lane-group sum over c channels: ceil(c / lanes) terms a lane, log2(lanes) shuffle adds, the division
    by c and the added eps"""
    lanes = pn_lanes(c)
    return -(-c // lanes) + int(math.log2(lanes)) + 2


def pn_data(npix, c):
    return normal(7000 + 13 * c + npix, (npix, c), 1.3), normal(9000 + 13 * c + npix, (npix, c))


def _pn_r(x64, eps):
    return 1.0 / np.sqrt(np.mean(x64 * x64, axis=-1, keepdims=True) + np.float64(F32(eps)))


def pixel_norm(x, eps=PN_EPS):
    """x * rsqrt(mean_c x^2 + eps), eps the float32 the C ABI receives"""
    x64 = x.astype(np.float64)
    return x64 * _pn_r(x64, eps)


def pixel_norm_bound(x, eps=PN_EPS):
    """all terms of the sum of squares are positive: relative error E U, E = pn_sum_roundings(c).  The scale carries half of
    it plus 1.5 U for rsqrtf, the product one more rounding"""
    e = pn_sum_roundings(x.shape[-1])
    return SLACK * (e / 2.0 + 2.5) * U * np.abs(pixel_norm(x, eps)) + TINY


def pixel_norm_bwd(dy, x, eps=PN_EPS):
    """dx = r (dy - x k), r = rsqrt(mean_c x^2 + eps), k = r^2 mean_c(dy x)"""
    x64, d64 = x.astype(np.float64), dy.astype(np.float64)
    r = _pn_r(x64, eps)
    k = r * r * np.mean(d64 * x64, axis=-1, keepdims=True)
    return r * (d64 - x64 * k)


def pixel_norm_bwd_bound(dy, x, eps=PN_EPS):
    """r is off by (E/2 + 1.5) U relative.  The terms of the dot product have either sign, so its error is E U sum |dy x|
    and not E U |dot|: with kabs = r^2 mean_c |dy x| >= |k|, k = dot r r / c is off by (E + 2 (E/2 + 1.5) + 3) U kabs.
    dx = r (dy - x k) adds the product, the subtraction (which can cancel) and the multiplication by r:
    |error| <= (2.5 E + 10.5) U r (|dy| + |x| kabs)."""
    e = pn_sum_roundings(x.shape[-1])
    x64, d64 = x.astype(np.float64), dy.astype(np.float64)
    r = _pn_r(x64, eps)
    kabs = r * r * np.mean(np.abs(d64 * x64), axis=-1, keepdims=True)
    return SLACK * (2.5 * e + 10.5) * U * r * (np.abs(d64) + np.abs(x64) * kabs) + TINY


# ---------------------------------------------------------------------------------------------- minibatch stddev
# n, group, h, w, c
MBSTD_CASES = [
    (8, 4, 24, 24, 3),      # hwc 1728, g hw 2304: more than one block per group in both statistic passes, 7 elementwise
    (3, 4, 5, 7, 3),        # group > n
    (4, 1, 8, 8, 16),       # g = 1: the statistic is sqrt(1e-8)
    (4, 4, 4, 4, 33),       # m = 1
    (6, 2, 3, 3, 1),        # c = 1
]
MBSTD_OFFSET = 1000.0       # (8, 4, 24, 24, 3) again with this added to every input


def mbstd_data(case, offset=0.0):
    n, group, h, w, c = case
    x = normal(500 + n + 7 * c, (n, h, w, c)).astype(np.float64)
    m = n // min(group, n)
    # members of group mi are the samples with n % m == mi: another spread per group, so that stat[n % m] cannot be
    # confused with another index
    x *= (1.0 + np.arange(n) % m)[:, None, None, None]
    return (x + offset).astype(F32), normal(600 + n + 7 * c, (n, h, w, c + 1))


def mbstd_stat(x, group):
    """per-group statistic [m] and per-element standard deviations [m, h, w, c] of GAN.minibatch_stddev_layer, float64"""
    n = x.shape[0]
    g = min(group, n)
    v = x.astype(np.float64).reshape((g, n // g) + x.shape[1:])
    v = v - v.mean(axis=0, keepdims=True)
    sd = np.sqrt((v * v).mean(axis=0) + 1e-8)
    return sd.mean(axis=(1, 2, 3)), sd


def _mbstd_sum_roundings(count):
    """roundings of a sum of `count` addends as the statistic kernels form it: blocks = min(ceil(count / 1024), 512) of 256
    threads, each thread ceil(count / (256 blocks)) addends, 8 tree levels, one atomic per block in any order"""
    blocks = min(-(-count // 1024), 512)
    return -(-count // (256 * blocks)) + 8 + blocks


def mbstd_stat_bound(x, group):
    """[m].  (addends per thread + 8 + blocks) U stat for the sum of positive terms, 2 U for 1 / hwc and its product,
    (g + 3) U for the two-pass variance of each term; the mean of g > 1 members is off by at most g U max|x|, which enters
    the variance only squared (the deviations from the true mean sum to zero): (g U max|x|)^2 / (2 sd) on each sd"""
    n, h, w, c = x.shape
    g = min(group, n)
    stat, sd = mbstd_stat(x, group)
    cnt = _mbstd_sum_roundings(h * w * c) + 2 + g + 3
    mean_term = (0.5 * (g * U * float(np.abs(x).max())) ** 2 / sd).mean(axis=(1, 2, 3)) if g > 1 else 0.0
    return SLACK * (cnt * U * stat + mean_term) + TINY


def mbstd(x, group):
    """(y [n, h, w, c + 1] float64, stat [m])"""
    n = x.shape[0]
    stat, _ = mbstd_stat(x, group)
    m = stat.shape[0]
    last = np.broadcast_to(stat[np.arange(n) % m][:, None, None, None], x.shape[:3] + (1,))
    return np.concatenate([x.astype(np.float64), last], axis=3), stat


def mbstd_bwd(x, dy, group):
    """float64 autograd on the torch statement of GAN.py:476-488 (tests/test_kernels_gpu.py, test_minibatch_stddev_gradient)"""
    import torch
    n, h, w, c = x.shape
    g = min(group, n)
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    v = x64.reshape(g, -1, h, w, c)
    v = v - v.mean(dim=0, keepdim=True)
    v = torch.sqrt((v * v).mean(dim=0) + 1e-8).mean(dim=(1, 2, 3), keepdim=True)
    y = torch.cat([x64, v.repeat(g, h, w, 1)], dim=3)
    (dx,) = torch.autograd.grad(y, [x64], torch.tensor(dy, dtype=torch.float64))
    return y.detach().numpy(), dx.numpy()


def mbstd_bwd_bound(x, dy, group):
    """dx = dy[..., :c] + t, t = coef (x - mean), coef = dstat / (hwc g sd), dstat the group's sum of dy[..., c].
    dstat: (addends + 8 + blocks) U sum |dy[..., c]| (terms of either sign); coef: (g + 3) / 2 for sd, 4 for the two
    products and the division; t: the difference and the product; the mean's g U max|x| acts on the difference; the final
    sum rounds once."""
    n, h, w, c = x.shape
    g = min(group, n)
    m = n // g
    _, sd = mbstd_stat(x, group)
    v = x.astype(np.float64).reshape(g, m, h, w, c)
    dev = np.abs(v - v.mean(axis=0, keepdims=True))
    d64 = dy.astype(np.float64)
    last = d64[..., c].reshape(g, m, h * w)
    dstat, dstat_abs = last.sum(axis=(0, 2)), np.abs(last).sum(axis=(0, 2))
    scale = 1.0 / (h * w * c * g * sd)                                     # [m, h, w, c]
    t = np.abs(dstat)[:, None, None, None] * scale * dev                   # [g, m, h, w, c]
    t_sum = _mbstd_sum_roundings(g * h * w) * dstat_abs[:, None, None, None] * scale * dev
    t_mean = np.abs(dstat)[:, None, None, None] * scale * (g * float(np.abs(x).max()) if g > 1 else 0.0)
    _, dx = mbstd_bwd(x, dy, group)
    total = np.abs(dx).reshape(g, m, h, w, c) + t * ((g + 3) / 2.0 + 6.0) + t_sum + t_mean
    return (SLACK * U * total + TINY).reshape(n, h, w, c)


# ---------------------------------------------------------------------------------------------- add_act, lerp
ELEM_N = (1, 255, 256, 257, 70001)
ACTS = (None, "relu", "lrelu", "tanh")
LEAK = 0.2
LERP_T_EXACT = (0.0, 1.0, 0.5)
LERP_T = (0.0, 0.3, 1.0, 1.7)


def special_values(n):
    """normal data with zeros, negative zeros and +-20 mixed in (the first eight elements when n allows it)"""
    a = normal(31, (n,), 2.0)
    sp = np.array([0.0, -0.0, 20.0, -20.0, 0.0, -0.0, 20.0, -20.0], dtype=F32)
    a[:min(n, 8)] = sp[:min(n, 8)]
    return a


def add_act(a, b, act, leak=LEAK):
    """act(a + b) in float64 on the float32 sum (the one add is a float32 add in the kernel and here)"""
    v = a if b is None else (a + b).astype(F32)
    if act is None or act == "relu":
        return O.activation(v, act)
    lk = np.float64(F32(leak))
    v64 = v.astype(np.float64)
    if act == "lrelu":
        return 0.5 * (1.0 + lk) * v64 + 0.5 * (1.0 - lk) * np.abs(v64)
    return np.tanh(v64)


def add_act_bound(a, b, act):
    """lrelu: 1 + leak, 1 - leak, two coefficient products, two products with v and the sum, all on at most |v|: 7 U |v|.
    tanh: a float32 tanhf within 2 ulp = 4 U of the result"""
    ref = np.abs(add_act(a, b, act))
    v = np.abs(a if b is None else (a + b).astype(F32)).astype(np.float64)
    if act == "lrelu":
        return SLACK * 7 * U * v + TINY
    if act == "tanh":
        return SLACK * 4 * U * ref + TINY
    raise ValueError(act)


def lerp(x, y, t, dtype=np.float64):
    """x + (y - x) clip(t, 0, 1) with the float32 t the C ABI receives; x None = zeros"""
    tt = dtype(F32(min(max(float(t), 0.0), 1.0)))
    a = np.zeros(y.shape, dtype=dtype) if x is None else x.astype(dtype)
    return a + (y.astype(dtype) - a) * tt


def lerp_bound(x, y):
    """the difference, the product and the sum, each on at most |x| + |y|"""
    a = 0.0 if x is None else np.abs(x.astype(np.float64))
    return SLACK * 3 * U * (a + np.abs(y.astype(np.float64))) + TINY


# ---------------------------------------------------------------------------------------------- axis zoom
# shape, axis, factor
ZOOM_CASES = [
    ((1, 4, 5, 2), 0, 4), ((3, 1, 5, 2), 1, 4), ((3, 4, 1, 2), 2, 4),            # n = 1: every output plane is the input plane
    ((2, 4, 5, 2), 0, 8), ((3, 2, 5, 2), 1, 8), ((3, 4, 2, 2), 2, 8),            # n = 2
    ((6, 4, 5, 2), 0, 1), ((3, 6, 5, 2), 1, 1), ((3, 4, 6, 2), 2, 1),            # factor 1: bit-exact copy
    ((6, 4, 5, 2), 0, 1.5), ((3, 6, 5, 2), 1, 1.5), ((3, 4, 6, 2), 2, 1.5),      # big = 9
    ((3, 4, 5, 1), 2, 4),                                                        # inner = 1
    ((5, 4, 3, 2), 0, 4), ((1, 5, 3, 2), 1, 4),                                  # outer = 1
]


def zoom(v, axis, factor):
    """(float64 result of scipy.ndimage.zoom(order=1) along one axis, bound 2^-23 max(|a|, |b|)): the kernel works in double
    and rounds once"""
    n = v.shape[axis]
    big = int(round(n * factor))
    o = np.arange(big, dtype=np.float64)
    s = o * (n - 1) / (big - 1) if big > 1 else np.zeros(1)
    i0 = np.minimum(np.floor(s).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    shape = [1] * v.ndim
    shape[axis] = big
    t = (s - i0).reshape(shape)
    a = np.take(v, i0, axis=axis).astype(np.float64)
    b = np.take(v, i1, axis=axis).astype(np.float64)
    return a * (1.0 - t) + b * t, 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) + TINY


# ---------------------------------------------------------------------------------------------- add_adjacent
ADJ_S = (1, 2, 6)
ADJ_C = (1, 4)
ADJ_HW = (4, 5)


def adj_windows(s):
    """(s_off, s_cnt): all slices, the first alone, the last alone, and [2, 5) of 6"""
    wins = [(0, s), (0, 1), (s - 1, 1)] + ([(2, 3)] if s == 6 else [])
    return sorted(set(wins))


def add_adjacent(x, s_off=0, s_cnt=None):
    """out[i] = concat(in[i], in[i-1][..., 0], in[i+1][..., 0]), zeros at the ends of the WHOLE stack; slices [s_off, s_off + s_cnt)"""
    s = x.shape[0]
    s_cnt = s - s_off if s_cnt is None else s_cnt
    if s >= 2:
        full = MP.add_adjacent(x, x.shape[-1])
    else:
        zero = np.zeros_like(x[..., 0:1])
        full = np.concatenate([x, zero, zero], axis=3)
    return full[s_off:s_off + s_cnt]


# ---------------------------------------------------------------------------------------------- shared, read-only inputs
@functools.lru_cache(maxsize=None)
def resize_input(h, w, c, kind):
    x = ints(11 + h + 3 * w + c, (RESIZE_N, h, w, c)) if kind == "int" else normal(17 + h + 3 * w + c, (RESIZE_N, h, w, c))
    x.setflags(write=False)
    return x
