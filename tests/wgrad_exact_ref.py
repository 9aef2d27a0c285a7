"""Data, float64 reference and case list of the bit-exact weight-gradient suite (test_wgrad_exact_gpu.py,
test_wgrad_exact_host.py) for the matrix-core kernels of csrc/mpgan_wgrad_mfma.hip.

The weight gradient contracts over the pixels P = n h w:

    dw[ky, kx, ci, co] = wscale * sum_{b, oy, ox} x[b, oy + ky - (kh-1)//2, ox + kx - (kw-1)//2, ci] * dy[b, oy, ox, co]

with x zero outside the image.  "Lo-exact" data (conv_exact_ref.lo_exact): v = s (1 + l 2^-f), the lo part with the sign
of the hi part, so the fp16 split of include/mpgan.h is hi = s, lo = s l 2^-f.  Every product of the three-product
definition x_hi d_hi + x_lo d_hi + x_hi d_lo is a multiple of 2^-f and the sum of |term| over P is at most
P (1 + 6 2^-f) < 2^(24 - f): every fp32 partial sum, in any order, is exact.  f = 13 with l in 0..3 holds up to P = 2046;
f = 12 and f = 11 with l in {0, 1} up to 4094 and 8190.  dy is the lo-exact tensor times 2^e (e = -20: the gradient range
that needs the power-of-two scale of mpg::pow2_scale), wscale is 0.5: every factor besides the data is a power of two, so
the kernels' `val * unscale` and the fp32 atomics that combine row ranges, splits and column chunks are exact too, and the
result does not depend on their order.  The expectation is the float64 sum of the three products (F16X1: of x_hi d_hi
alone) times wscale 2^e, NOT x * dy, which also holds lo * lo.

The "normal" data kind (Gaussian x, 1e-6-scaled Gaussian dy: arbitrary mantissas) is compared with the float64 autograd
of test_train_gpu.ref_conv_grads at that file's bounds.

Nothing here touches the GPU or the library under test.  Each case names, as `cls`, the fields of the launch plan
(mpg_conv2d_wgrad_plan) it is there for; the host test holds them against the library.
"""
import functools
import zlib

import numpy as np

from conv_exact_ref import lo_exact, split16, sum_abs_bound      # noqa: F401  (re-exported)

WSCALE = 0.5
EXPONENTS = (0, -20)
NORMAL_WSCALE = 0.05
NORMAL_BOUND = {3: 2e-6, 1: 2e-3}          # relative L2, as test_train_gpu.test_conv_wgrad_mfma


def frac_for(p):
    """the f of v = s (1 + l 2^-f) for a contraction over p pixels"""
    for f in (13, 12, 11):
        if sum_abs_bound(p, f) < 2.0 ** (24 - f):
            return f
    raise ValueError("contraction over %d pixels is too long for exact fp32 sums" % p)


class Case(object):
    """one weight gradient.  `cls`: the plan fields the case is there for, held by the host test against launch
    `cls_launch` of the plan at every precision of the case.  `guard`: part of the subset that runs the raw ABI call into a
    NaN-guarded buffer.  `normal`: also run with Gaussian data."""

    def __init__(self, name, n, h, w, cin, cout, kh, kw, precs=(3, 1), cls=None, cls_launch=0, launches=None, guard=False,
                 normal=False):
        self.name, self.n, self.h, self.w, self.cin, self.cout, self.kh, self.kw = name, n, h, w, cin, cout, kh, kw
        self.precs, self.cls, self.cls_launch, self.launches = tuple(precs), dict(cls or {}), cls_launch, launches
        self.guard, self.normal = guard, normal

    @property
    def pixels(self):
        return self.n * self.h * self.w

    @property
    def frac(self):
        return frac_for(self.pixels)

    @property
    def shape(self):
        return (self.n, self.h, self.w, self.cin, self.cout, self.kh, self.kw)

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def wgrad64(x, dy, kh, kw):
    """sum_p x[p + tap] dy[p] in float64, [kh, kw, cin, cout]: one matrix product per tap; TF SAME padding ((k - 1) // 2
    zeros in front of a k-wide filter)"""
    x = np.asarray(x, dtype=np.float64)
    dy = np.asarray(dy, dtype=np.float64)
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    assert dy.shape[:3] == (n, h, w)
    pt, pl = (kh - 1) // 2, (kw - 1) // 2
    xp = np.zeros((n, h + kh - 1, w + kw - 1, cin))
    xp[:, pt:pt + h, pl:pl + w] = x
    d2 = dy.reshape(n * h * w, cout)
    out = np.empty((kh, kw, cin, cout))
    for ky in range(kh):
        for kx in range(kw):
            out[ky, kx] = xp[:, ky:ky + h, kx:kx + w].reshape(n * h * w, cin).T @ d2
    return out


class CaseData(object):
    """lo-exact tensors of a case: x [n, h, w, cin] and d [n, h, w, cout] (float32; dy = d 2^e), their fp16 parts
    (xh, xl), (dh, dl) in float64 and the partial sums hh = x_hi d_hi, corr = x_lo d_hi + x_hi d_lo"""

    def __init__(self, case):
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        f = case.frac
        self.case = case
        self.x, self.xh, self.xl = lo_exact(rng, (case.n, case.h, case.w, case.cin), f)
        self.d, self.dh, self.dl = lo_exact(rng, (case.n, case.h, case.w, case.cout), f)
        self.hh = wgrad64(self.xh, self.dh, case.kh, case.kw)
        self.corr = wgrad64(self.xl, self.dh, case.kh, case.kw) + wgrad64(self.xh, self.dl, case.kh, case.kw)

    def dy(self, e):
        return self.d * np.float32(2.0 ** e)

    def expected64(self, prec, e):
        return WSCALE * 2.0 ** e * (self.hh if prec == 1 else self.hh + self.corr)

    def expected(self, prec, e):
        return self.expected64(prec, e).astype(np.float32)


@functools.lru_cache(maxsize=4)
def case_data(case):
    return CaseData(case)


@functools.lru_cache(maxsize=2)
def normal_data(case):
    """(x, dy) Gaussian float32, dy times 1e-6"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()) + 1)
    x = rng.standard_normal((case.n, case.h, case.w, case.cin)).astype(np.float32)
    dy = (rng.standard_normal((case.n, case.h, case.w, case.cout)) * 1e-6).astype(np.float32)
    return x, dy


# ---------------------------------------------------------------------------------------------------------------------
# diagnosis
# ---------------------------------------------------------------------------------------------------------------------
def mismatch_report(got, want, what=""):
    """'' when the arrays [kh, kw, cin, cout] are equal bit for bit; else where they differ: how many values, the first
    (ky, kx, ci, co), and the taps, ci tiles and cout tiles of 32 that are hit"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad) == 0:
        return ""
    ky, kx, ci, co = (int(v) for v in bad[0])
    taps = sorted({(int(b[0]), int(b[1])) for b in bad})
    cis = sorted({int(b[2]) // 32 for b in bad})
    cos = sorted({int(b[3]) // 32 for b in bad})
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = err.max() / max(np.abs(want.astype(np.float64)).max(), 1e-300)
    return ("%s: %d of %d values differ (max |diff| %.3e, %.3e of max |expected|); first at (ky, kx, ci, co) = (%d, %d, %d, %d): "
            "got %r, expected %r; taps hit: %s%s; ci tiles hit: %s; cout tiles hit: %s"
            % (what, len(bad), got.size, float(err.max()), float(rel), ky, kx, ci, co, float(got[ky, kx, ci, co]),
               float(want[ky, kx, ci, co]), taps[:10], " ..." if len(taps) > 10 else "", cis, cos))


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the smallest shapes that reach each launch class of wgrad_plan
# ---------------------------------------------------------------------------------------------------------------------
def ring(**kw):
    return dict(form="ring", **kw)


def row(**kw):
    return dict(form="row", **kw)


X3, X1 = (3,), (1,)

CASES = [
    # ---- ring form (square 3x3 / 4x4 / 5x5): every instantiation <K, K, COTW, PREC> ---------------------------------------
    Case("ring 3x3 8->20 cotw1", 1, 9, 17, 8, 20, 3, 3, cls=ring(k=3, cotw=1, n_cow=1), guard=True),
    Case("ring 3x3 8->40 cotw2", 1, 9, 41, 8, 40, 3, 3, cls=ring(k=3, cotw=2, n_cow=1), guard=True),          # 3 k-steps, the last 9 pixels
    Case("ring 3x3 8->70 x3 cotw2", 1, 9, 17, 8, 70, 3, 3, X3, cls=ring(k=3, cotw=2, prec=3, n_cow=2), guard=True),
    Case("ring 3x3 8->70 x1 cotw4", 1, 9, 17, 8, 70, 3, 3, X1, cls=ring(k=3, cotw=4, prec=1, n_cow=1), guard=True, normal=True),
    Case("ring 4x4 8->20 cotw1", 1, 9, 17, 8, 20, 4, 4, cls=ring(k=4, cotw=1, n_cow=1), guard=True),
    Case("ring 4x4 8->40 cotw2", 1, 9, 17, 8, 40, 4, 4, cls=ring(k=4, cotw=2, n_cow=1), guard=True),
    Case("ring 5x5 8->40 cotw1", 1, 9, 17, 8, 40, 5, 5, cls=ring(k=5, cotw=1, n_cow=2), guard=True),
    # ---- ring geometry: w < 8, h < KH, 1..3 column chunks with a ragged last one, 1..3 row ranges with a ragged last one
    # that starts at a row which is no multiple of KH + 1, n_outer % 8 != 0 (padding blocks return), channel groups and
    # cout tiles that do not exist, a fifth ci tile, a ragged last cout window
    Case("ring h1 w5 3x3 8->8", 1, 1, 5, 8, 8, 3, 3, cls=ring(k=3, cotw=1, chunks=1, ranges=1, rows_per_range=1, n_outer=1)),
    Case("ring h2 w17 n3 5x5 12->20", 3, 2, 17, 12, 20, 5, 5, cls=ring(k=5, chunks=1, ranges=1, rows_per_range=2, n_outer=3), normal=True),
    Case("ring h2 w5 4x4 12->8", 1, 2, 5, 12, 8, 4, 4, cls=ring(k=4, cotw=1, ranges=1, rows_per_range=2)),
    Case("ring h9 w64 3x3 40->70 x3", 1, 9, 64, 40, 70, 3, 3, X3, cls=ring(k=3, cotw=2, chunks=1, n_ci=2, n_cow=2, ranges=1, rows_per_range=9)),
    Case("ring h9 w64 3x3 40->70 x1", 1, 9, 64, 40, 70, 3, 3, X1, cls=ring(k=3, cotw=4, chunks=1, n_ci=2, n_cow=1, ranges=1, rows_per_range=9)),
    Case("ring h17 w70 5x5 8->136", 1, 17, 70, 8, 136, 5, 5, cls=ring(k=5, chunks=2, n_ci=1, n_cow=5, ranges=2, rows_per_range=9, n_outer=4), normal=True),
    Case("ring h25 w17 n3 3x3 130->130 x3", 3, 25, 17, 130, 130, 3, 3, X3,
         cls=ring(k=3, cotw=2, n_ci=5, n_cow=3, ranges=3, rows_per_range=9, n_outer=9), normal=True),
    Case("ring h25 w17 n3 3x3 130->130 x1", 3, 25, 17, 130, 130, 3, 3, X1,
         cls=ring(k=3, cotw=4, n_ci=5, n_cow=2, ranges=3, rows_per_range=9, n_outer=9)),
    Case("ring h9 w129 4x4 12->40", 1, 9, 129, 12, 40, 4, 4, cls=ring(k=4, cotw=2, chunks=3, ranges=1, n_outer=3)),
    Case("ring h25 w70 5x5 40->8", 1, 25, 70, 40, 8, 5, 5, cls=ring(k=5, chunks=2, n_ci=2, n_cow=1, ranges=3, rows_per_range=9, n_outer=6)),
    Case("ring h65 w70 3x3 8->8", 1, 65, 70, 8, 8, 3, 3, cls=ring(k=3, chunks=2, ranges=8, rows_per_range=9, n_outer=16)),     # f = 11; no padding blocks
    Case("ring h17 w5 n3 4x4 130->136", 3, 17, 5, 130, 136, 4, 4, cls=ring(k=4, cotw=2, n_ci=5, n_cow=3, ranges=2, rows_per_range=9, n_outer=6)),
    # ---- row form: every launch<KW, COTW, PREC>, every wave layout (cit, cog, ks), kw = 3 under kh in {1, 2, 5, 6, 7} (the
    # even heights pad one row before), kw = 4 as (2,4), kw = 5 as (1,5) and (7,5) ------------------------------------------
    Case("row 1x3 8->8", 2, 5, 19, 8, 8, 1, 3, cls=row(k=3, cotw=1, cit=1, cog=1, ks=2, chunk=32), guard=True),
    Case("row 6x3 8->40", 2, 5, 70, 8, 40, 6, 3, cls=row(k=3, cotw=1, cit=1, cog=2, ks=4, chunk=128)),
    Case("row 1x1 8->104", 2, 5, 70, 8, 104, 1, 1, cls=row(k=1, cotw=1, cit=1, cog=4, ks=2, chunk=64), guard=True),
    Case("row 7x3 40->8", 2, 5, 70, 40, 8, 7, 3, cls=row(k=3, cotw=1, cit=2, cog=1, ks=4, chunk=128)),
    Case("row 2x3 40->40", 2, 5, 70, 40, 40, 2, 3, cls=row(k=3, cotw=1, cit=2, cog=2, ks=2, chunk=64), normal=True),
    Case("row 1x1 40->104", 2, 4, 19, 40, 104, 1, 1, cls=row(k=1, cotw=1, cit=2, cog=4, ks=1, chunk=32, nsplit=8)),     # no padding blocks
    Case("row 5x3 72->8", 2, 5, 70, 72, 8, 5, 3, cls=row(k=3, cotw=1, cit=4, cog=1, ks=2, chunk=64)),
    Case("row 1x1 72->40", 2, 5, 70, 72, 40, 1, 1, cls=row(k=1, cotw=1, cit=4, cog=2, ks=1, chunk=64)),
    Case("row 5x3 72->104 cotw2", 2, 5, 19, 72, 104, 5, 3, cls=row(k=3, cotw=2, cit=4, cog=2, ks=1, chunk=32), guard=True, normal=True),
    Case("row 1x1 72->104 cotw2", 2, 5, 70, 72, 104, 1, 1, cls=row(k=1, cotw=2, cit=4, cog=2, ks=1, chunk=64), guard=True, normal=True),
    Case("row 2x4 40->40", 2, 5, 19, 40, 40, 2, 4, cls=row(k=4, cotw=1, cit=2, cog=2), guard=True),
    Case("row 1x5 8->40", 2, 5, 19, 8, 40, 1, 5, cls=row(k=5, cotw=1, cit=1, cog=2), guard=True),
    Case("row 7x5 72->40", 2, 5, 19, 72, 40, 7, 5, cls=row(k=5, cotw=1, cit=4, cog=2, ks=1)),
    # ---- row form, chunk: 32, 64, 128, 256 pixels at 8 -> 8 (all eight waves share the k-steps from 128 on); rows of several
    # chunks whose last one is shorter than one k-step
    Case("row chunk32 w9 1x3 8->8", 2, 5, 9, 8, 8, 1, 3, cls=row(chunk=32, ks=2)),
    Case("row chunk64 w33 3x1 8->8", 2, 5, 33, 8, 8, 3, 1, cls=row(chunk=64, ks=4)),
    Case("row chunk128 w70 1x3 8->8", 2, 5, 70, 8, 8, 1, 3, cls=row(chunk=128, ks=8)),
    Case("row chunk256 w130 2x3 8->8", 2, 3, 130, 8, 8, 2, 3, cls=row(chunk=256, ks=8), normal=True),
    Case("row chunk256 w260 1x3 8->8", 1, 3, 260, 8, 8, 1, 3, cls=row(chunk=256, ks=8)),                        # 256 + 4 pixels
    Case("row chunk64 w130 5x3 72->104", 1, 3, 130, 72, 104, 5, 3, cls=row(k=3, cotw=2, chunk=64, ks=1)),         # 64 + 64 + 2 pixels
    # ---- row form, windows: merged on the grid; unmerged with a ragged last window; cin > 128
    Case("row merged 1x1 8->256", 2, 5, 19, 8, 256, 1, 1, cls=row(windows=2, cout=128, cit=1, cog=4), launches=1, normal=True),
    Case("row merged 2x4 8->128", 2, 5, 19, 8, 128, 2, 4, cls=row(windows=2, cout=64, cit=1, cog=2), launches=1, normal=True),
    Case("row merged 5x3 40->256", 1, 5, 19, 40, 256, 5, 3, cls=row(windows=2, cout=128, cit=2, cog=4), launches=1),
    Case("row ragged window 5x3 8->192", 2, 5, 19, 8, 192, 5, 3, cls=row(windows=1, co0=128, cout=64, cog=2), cls_launch=1, launches=2),
    Case("row ragged window 2x4 8->96", 2, 5, 19, 8, 96, 2, 4, cls=row(windows=1, co0=64, cout=32, cog=1), cls_launch=1, launches=2),
    Case("row cin260 1x1 260->40", 2, 5, 19, 260, 40, 1, 1, cls=row(ci0=256, cin=4, cit=1, cog=2), cls_launch=2, launches=3),
    Case("row cin260 1x1 260->256", 2, 5, 19, 260, 256, 1, 1, cls=row(ci0=128, cin=128, cit=4, cog=2, cotw=2, windows=2), cls_launch=1, launches=3),
    # ---- row form, splits: two image rows per split, one split holding the last row of an image and the first of the next
    # (the vertical taps' halo row is zero there, not the other image's row); nsplit % 8 != 0
    Case("row splits 7x3 n3 h49 w8", 3, 49, 8, 8, 8, 7, 3, cls=row(nsplit=74, rows_per_split=2), normal=True),
    Case("row splits 1x5 n2 h513 w2", 2, 513, 2, 8, 8, 1, 5, cls=row(nsplit=513, rows_per_split=2)),
    Case("row splits 3x1 n3 h115 w4", 3, 115, 4, 8, 40, 3, 1, cls=row(nsplit=173, rows_per_split=2)),
    Case("row nsplit 10 5x1 40->8", 2, 5, 19, 40, 8, 5, 1, cls=row(nsplit=10, rows_per_split=1, blocks=80)),
]

GUARD_CASES = [c for c in CASES if c.guard]
NORMAL_CASES = [c for c in CASES if c.normal]
