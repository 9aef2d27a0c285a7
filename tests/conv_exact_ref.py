"""Data and float64 reference of the bit-exact fused-convolution suite (test_conv_exact_gpu.py, test_conv_exact_host.py).

"Lo-exact" data: v = s (1 + l 2^-f) with a random sign s and a random integer l (0..3 at f = 13; 0..1 at f = 12 once the
contraction K = sum of kh kw cin over the segments exceeds 2046).  The lo part carries the sign of the hi part, so the
split of include/mpgan.h is exact: hi = fp16(v) = s and lo = fp16(v - hi) = s l 2^-f.  Every product of the three-product
definition a_hi w_hi + a_lo w_hi + a_hi w_lo is a multiple of 2^-f, and the sum of |term| over K is at most
K (1 + 6 2^-f) < 2^(24 - f): every partial sum, in any order, is an exact fp32 number, and so is the result.  Hi values
are bf6 (e3m2) code 8 and lo values codes {0, 4, 8, 12} under any block scale that puts the block maximum in [8, 16).
The expectation is the float64 sum of the three products (F16X1: of a_hi w_hi alone), NOT x * w, which also holds
lo * lo.

With hi = +-1 everywhere every block of 32 K values has the same bf6 block scale.  Cases with gexp = 2 give every
second channel group of the activations the factor 2^-2 and the same input channels of the weights the factor 2^+2:
every product, and so the bound and the expectation's structure, stays what it was, but neighbouring blocks (and the
halves of a block that spans two groups) now carry different scales, and a scale applied to the wrong block shows.
Within a mixed block the smaller values are e3m2 codes 2 (hi) and {0, 1, 2, 3} or {0, 2, 4, 6} (lo): still exact.

conv_small_kernel (every cin and cout <= 8) multiplies hi + lo in fp32, so its cases use small integers instead.

Nothing here touches the GPU or the library under test, except launch_class(), a restatement of the host code's K
decomposition that the host test checks against mpg_conv_pack_size.
"""
import functools
import zlib

import numpy as np

MAX_SEG = 4
TW = 32


class Seg(object):
    """one K segment: a kh x kw filter over `cin` channels, starting at channel c_off of a c_total-channel source that
    is stored at 1 / 2^up_log2 of the output resolution"""

    def __init__(self, kh, kw, cin, up_log2=0, pad_hi=0, c_off=0, c_total=None, gexp=0):
        self.kh, self.kw, self.cin, self.up_log2, self.pad_hi, self.c_off = kh, kw, cin, up_log2, pad_hi, c_off
        self.c_total = c_off + cin if c_total is None else c_total
        self.gexp = gexp        # odd channel groups: activations times 2^-gexp, weights times 2^+gexp
        assert not (gexp and c_off)

    def group_scale(self):
        """per input channel: the power of two the activations are divided and the weights multiplied by"""
        return 2.0 ** (self.gexp * ((np.arange(self.cin) // 8) % 2))

    def __repr__(self):
        return "Seg(%dx%dx%d up %d pad_hi %d c_off %d of %d)" % (self.kh, self.kw, self.cin, self.up_log2, self.pad_hi,
                                                                  self.c_off, self.c_total)


class Case(object):
    """one launch shape.  `cls`: the launch class the case is there for, as the fields of launch_class() of segment 0
    (or of segment cls_seg) at precision cls_prec that must hold -- the host test checks them."""

    def __init__(self, name, n, h, w, cout, segs, precs=(1, 2, 3), act=None, g8=False, cls=None, cls_prec=None, cls_seg=0):
        self.name, self.n, self.h, self.w, self.cout, self.segs = name, n, h, w, cout, list(segs)
        self.precs, self.act, self.g8 = tuple(precs), act, g8
        self.cls, self.cls_prec, self.cls_seg = dict(cls or {}), cls_prec, cls_seg
        self.small = cout <= 8 and all(s.cin <= 8 for s in self.segs)     # conv_small_kernel: integer data

    @property
    def k(self):
        return sum(s.kh * s.kw * s.cin for s in self.segs)

    @property
    def frac(self):
        return 13 if self.k <= 2046 else 12

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def split16(v):
    """the split of include/mpgan.h in numpy: hi = fp16(v), lo = fp16(v - hi), both as float64"""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi.astype(np.float64), lo.astype(np.float64)


def lo_exact(rng, shape, frac):
    """(v float32, hi float64, lo float64) with v = hi + lo, hi = +-1, lo = hi * l * 2^-frac"""
    hi = rng.choice([-1.0, 1.0], size=shape)
    lo = hi * rng.integers(0, 4 if frac == 13 else 2, size=shape) * 2.0 ** -frac
    return (hi + lo).astype(np.float32), hi, lo


def small_ints(rng, shape):
    v = rng.integers(-3, 4, size=shape).astype(np.float64)
    return v.astype(np.float32), v, np.zeros(shape)


def sum_abs_bound(k, frac):
    """upper bound of the sum of |term| over a contraction of length k on lo-exact data"""
    return k * (1.0 + 6.0 * 2.0 ** -frac)


def g8_roundtrip(y):
    """what a G8 tensor (hi16 + lo16) keeps of fp32 values"""
    hi, lo = split16(y)
    return (hi + lo).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def pad_before(k, pad_hi):
    """zeros in front of a k-wide filter: TF SAME puts (k - 1) // 2 there, pad_hi = 1 puts k // 2"""
    return k // 2 if pad_hi else (k - 1) // 2


def upsample_nearest(x, up_log2):
    r = 1 << up_log2
    return x if r == 1 else np.repeat(np.repeat(x, r, axis=1), r, axis=2)


def correlate(x, w, pad_hi=0):
    """stride-1 zero-padded correlation in float64: out[n, y, x, o] = sum x[n, y + dy - pt, x + dx - pl, c] w[dy, dx, c, o]"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, h, wd, c = x.shape
    kh, kw, c2, co = w.shape
    assert c == c2
    pt, pl = pad_before(kh, pad_hi), pad_before(kw, pad_hi)
    xp = np.zeros((n, h + kh - 1, wd + kw - 1, c))
    xp[:, pt:pt + h, pl:pl + wd] = x
    out = np.zeros((n, h, wd, co))
    for dy in range(kh):
        for dx in range(kw):
            out += xp[:, dy:dy + h, dx:dx + wd] @ w[dy, dx]
    return out


class CaseData(object):
    """tensors of a case: per segment the source x [n, h >> up, w >> up, c_total] and the filter w [kh, kw, cin, cout]
    (float32), and per segment the float64 partial sums hh = a_hi w_hi and corr = a_lo w_hi + a_hi w_lo"""

    def __init__(self, case):
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        make = (lambda shape: small_ints(rng, shape)) if case.small else (lambda shape: lo_exact(rng, shape, case.frac))
        self.case, self.x, self.w, self.hh, self.corr, self.parts = case, [], [], [], [], []
        for s in case.segs:
            assert case.h % (1 << s.up_log2) == 0 and case.w % (1 << s.up_log2) == 0, (case, s)
            x, xh, xl = make((case.n, case.h >> s.up_log2, case.w >> s.up_log2, s.c_total))
            w, wh, wl = make((s.kh, s.kw, s.cin, case.cout))
            if s.gexp:      # powers of two: exact in every format
                gs = s.group_scale()
                x, xh, xl = (x / gs).astype(np.float32), xh / gs, xl / gs
                gs = gs[:, None]
                w, wh, wl = (w * gs).astype(np.float32), wh * gs, wl * gs
            win = slice(s.c_off, s.c_off + s.cin)
            up = lambda t: upsample_nearest(t[..., win], s.up_log2)
            self.x.append(x)
            self.w.append(w)
            self.parts.append(((xh, xl), (wh, wl)))
            self.hh.append(correlate(up(xh), wh, s.pad_hi))
            if case.small:      # fp32 arithmetic on hi + lo: integers have no lo part
                self.corr.append(np.zeros_like(self.hh[-1]))
            else:
                self.corr.append(correlate(up(xl), wh, s.pad_hi) + correlate(up(xh), wl, s.pad_hi))

    def expected64(self, prec):
        """float64 expectation before the activation: one product at MPG_PREC_F16X1, three at F16F6 / F16X3"""
        e = sum(self.hh)
        return e if prec == 1 and not self.case.small else e + sum(self.corr)

    def expected(self, prec):
        e = self.expected64(prec)
        if self.case.act == "relu":
            e = np.maximum(e, 0.0)
        else:
            assert self.case.act is None, "only exact activations"
        return e.astype(np.float32)


@functools.lru_cache(maxsize=4)
def case_data(case):
    return CaseData(case)


# ---------------------------------------------------------------------------------------------------------------------
# the K decomposition the host code (seg_shape / seg_shape_f6 / lds_plan in csrc/mpgan_conv_mfma.hip) chooses
# ---------------------------------------------------------------------------------------------------------------------
LDS_TWO_WG = 80 * 1024


def pipe(nt, prec):
    """(tile rows, k-steps per stage, waves, stage bytes, ring bytes) of Pipe<NT, PREC> / Pipe6<NT> (csrc/mpgan_conv.h)"""
    if prec == 2:
        return dict(th=16, ks=4, waves=4 if nt == 1 else 8, wstage=8 * nt * 1024, ring=3 * 8 * nt * 1024)
    th = 8 if nt >= 3 else 16
    ks = (1 if nt in (2, 4) else 2) * (1 if prec == 3 else 2)
    wstage = ks * nt * 1024 * (2 if prec == 3 else 1)
    return dict(th=th, ks=ks, waves=4, wstage=wstage, ring=(3 if nt == 3 else 4) * wstage)


def _img_bytes(p, kh, kw, cgc):
    npx = ((p["th"] + kh - 1) * (TW + kw - 1) + 63) & ~63
    ni = (cgc * 2 * (npx // 64) + p["waves"] - 1) // p["waves"]
    return ni * p["waves"] * 1024


def launch_class(kh, kw, cin, cout, prec):
    """kernel family and K decomposition of one segment: dict(kernel, nt, th, cgc, nchunks, sc, stages, tp, pref,
    direct, ring_wraps, wstage).  Launches whose every cin and cout is <= 8 run conv_small_kernel (kernel = "small"),
    which reads an fp32 table behind the MFMA image the decomposition describes.

    A classifier for the case list, never the source of an expectation.  The host test holds it against
    mpg_conv_pack_size, which confirms `stages` times `wstage` only: through them nt, the direct path, tp and, wherever
    the stage count differs between one and two groups per chunk, cgc.  `pref` and `th` are copies of the host code's
    formula and of the Pipe traits and are confirmed by nothing; a retuned Pipe has to be restated here."""
    nt = (cout + 31) // 32
    p = pipe(nt, prec)
    cg = (cin + 7) // 8
    t = kh * kw
    c = dict(kernel="mfma", nt=nt, th=p["th"], cgc=1, nchunks=cg, tp=0, pref=0, direct=0, wstage=p["wstage"])
    if prec == 2:
        c["kernel"] = "f6"
        if t == 1 and cin > 8 and nt <= 2:
            c.update(direct=1, nchunks=1, sc=(cg + 7) // 8)
        else:
            tp = t if t >= 16 else 8 if t <= 8 else 12 if t <= 12 else 16
            pref = 1
            for g in range(1, cg):
                if (g * tp) // 8 - ((g - 1) * tp + 7) // 8 < 2:
                    pref = 0
            c.update(tp=tp, pref=pref, sc=(cg * tp + 7) // 8)
        c["stages"] = c["sc"]
    else:
        if cg >= 2 and t % 2 == 1 and 1024 + 2 * _img_bytes(p, kh, kw, 2) + p["ring"] <= LDS_TWO_WG:
            c["cgc"] = 2
        c["nchunks"] = (cg + c["cgc"] - 1) // c["cgc"]
        c["sc"] = ((t * c["cgc"] + 1) // 2 + p["ks"] - 1) // p["ks"]
        c["stages"] = c["nchunks"] * c["sc"]
    c["ring_wraps"] = c["stages"] // (p["ring"] // p["wstage"])
    if cin <= 8 and cout <= 8:
        c["kernel"] = "small"
    return c


def pack_bytes(kh, kw, cin, cout, prec):
    """what mpg_conv_pack_size answers for a shape that fits the LDS"""
    c = launch_class(kh, kw, cin, cout, prec)
    return c["stages"] * c["wstage"] + (kh * kw * 64 * 4 if c["kernel"] == "small" else 0)


def tile_hw(case, prec):
    """(tile rows, tile columns) of a workgroup of the kernel that runs `case` at `prec`"""
    if case.small:
        return 16, 64
    return pipe((case.cout + 31) // 32, prec)["th"], TW


def blocks(case, prec):
    th, tw = tile_hw(case, prec)
    return case.n * ((case.h + th - 1) // th) * ((case.w + tw - 1) // tw)


# ---------------------------------------------------------------------------------------------------------------------
# diagnosis
# ---------------------------------------------------------------------------------------------------------------------
def mismatch_report(got, want, th, tw=TW, what=""):
    """'' when the arrays [n, h, w, c] are equal bit for bit; else where they differ: how many values, the first
    (n, y, x, c), that position as (tile row, tile column, cout tile of 32), and which tiles / cout tiles are hit"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32)) if got.dtype == np.float32 else np.argwhere(got != want)
    if len(bad) == 0:
        return ""
    n, y, x, c = (int(v) for v in bad[0])
    tiles = sorted({(int(b[1]) // th, int(b[2]) // tw) for b in bad})
    ctiles = sorted({int(b[3]) // 32 for b in bad})
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return ("%s: %d of %d values differ (max |diff| %.3e); first at (n, y, x, c) = (%d, %d, %d, %d): got %r, expected %r, "
            "i.e. tile row %d (row %d of it), tile column %d (column %d of it), cout tile %d (channel %d of it); "
            "tiles hit (row, column): %s%s; cout tiles hit: %s"
            % (what, len(bad), got.size, float(err.max()), n, y, x, c, float(got[n, y, x, c]), float(want[n, y, x, c]),
               y // th, y % th, x // tw, x % tw, c // 32, c % 32, tiles[:8], " ..." if len(tiles) > 8 else "", ctiles))


def rotations(seq):
    seq = list(seq)
    return [seq[i:] + seq[:i] for i in range(len(seq))]


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def S(kh, kw, cin, **kw_):
    return Seg(kh, kw, cin, **kw_)


# the minimal case: 1x1, cin 16, cout 32 on one 16x32 tile: one weight stage, one block.  Decides whether the block-scaled
# bf6 MFMA accumulates lo-exact data exactly (MPG_PREC_F16F6: the direct 1x1 path).
MINIMAL = Case("minimal 1x1x16->32 16x32", 1, 16, 32, 32, [S(1, 1, 16)], cls=dict(kernel="f6", direct=1, stages=1), cls_prec=2)

MFMA = (1, 3)     # conv_mfma_kernel
F6 = (2,)         # conv_mfma_f6_kernel

CASES = [
    MINIMAL,
    # ---- conv_mfma_kernel (F16X1 / F16X3) -------------------------------------------------------------------------
    # two groups per chunk (cgc = 2) needs an odd tap count, >= 16 channels AND two double-buffered images + ring within
    # 80 KiB: with the present Pipe shapes that holds only for three / four cout tiles (8-row tiles) and 1xN filters
    Case("mfma cgc2 1x1x16->65", 2, 9, 33, 65, [S(1, 1, 16)], MFMA, cls=dict(kernel="mfma", cgc=2, nchunks=1, nt=3)),    # one chunk
    Case("mfma cgc2 1x3x24->97", 2, 9, 33, 97, [S(1, 3, 24)], MFMA, cls=dict(kernel="mfma", cgc=2, nchunks=2, nt=4)),    # last chunk half empty
    Case("mfma cgc2 1x7x40->96", 1, 19, 40, 96, [S(1, 7, 40)], MFMA, g8=True, cls=dict(kernel="mfma", cgc=2, nchunks=3, nt=3)),
    Case("mfma cgc2 3x1x24->128", 1, 9, 33, 128, [S(3, 1, 24)], MFMA, cls=dict(kernel="mfma", cgc=2, nt=4)),
    # odd tap counts that fall back to one group per chunk because two two-group images exceed LDS_TWO_WG
    Case("mfma cgc1(lds) 3x3x16->40", 1, 19, 40, 40, [S(3, 3, 16)], MFMA, cls=dict(kernel="mfma", cgc=1, nchunks=2)),
    Case("mfma cgc1(lds) 3x3x24->40", 2, 19, 40, 40, [S(3, 3, 24)], MFMA, act="relu", cls=dict(kernel="mfma", cgc=1, nchunks=3)),   # 8 blocks: remap
    Case("mfma cgc1(lds) 5x5x40->40", 1, 9, 33, 40, [S(5, 5, 40)], MFMA, cls=dict(kernel="mfma", cgc=1, nchunks=5)),
    Case("mfma cgc1(lds) 7x7x16->97", 1, 9, 33, 97, [S(7, 7, 16)], MFMA, cls=dict(kernel="mfma", cgc=1, nchunks=2, nt=4)),
    # one group per chunk because the tap count is even
    Case("mfma cgc1(even) 4x4x16->40", 1, 19, 40, 40, [S(4, 4, 16)], MFMA, cls=dict(kernel="mfma", cgc=1, nchunks=2)),
    Case("mfma cgc1(even) 2x2x24->65", 1, 9, 33, 65, [S(2, 2, 24)], MFMA, cls=dict(kernel="mfma", cgc=1, nchunks=3, nt=3)),
    # one stage in the whole launch: fewer stages than the ring is deep
    Case("mfma one stage 1x1x8->16", 1, 3, 5, 16, [S(1, 1, 8)], MFMA, cls=dict(kernel="mfma", stages=1, ring_wraps=0)),    # image smaller than a tile
    Case("mfma two stages 1x1x16->32", 1, 19, 40, 32, [S(1, 1, 16)], MFMA, cls=dict(kernel="mfma", cgc=1, stages=2, ring_wraps=0)),   # one per chunk
    # many ring wraps
    Case("mfma ring 7x7x40->40", 1, 19, 40, 40, [S(7, 7, 40)], MFMA, g8=True, cls=dict(kernel="mfma", cgc=1, nchunks=5, stages=125), cls_prec=3),
    # K above 2046: l in 0..1, f = 12
    Case("mfma f12 5x5x128->32", 1, 9, 33, 32, [S(5, 5, 128)], (1, 2, 3), cls=dict(nchunks=16)),
    # all four cout tilings with full and barely started last tiles; h ragged against the tile height (16 rows for
    # one / two cout tiles, 8 for three / four); batch 2: 8 blocks at 19x40 (block-id remap) for nt <= 2, 12 for nt >= 3
] + [
    Case("cout %d 3x3x24" % co, 2, 19, 40, co, [S(3, 3, 24)], (1, 2, 3), g8=(co in (9, 33, 97)),
         cls=dict(nt=(co + 31) // 32, th=16 if co <= 64 else 8), cls_prec=3)
    for co in (9, 32, 33, 64, 65, 96, 97, 128)
] + [
    # ---- conv_mfma_f6_kernel (F16F6) ------------------------------------------------------------------------------
    # tp = 8: one group (pref 1) and several (pref 0)
    Case("f6 tp8 2x2x8->16", 1, 19, 40, 16, [S(2, 2, 8)], F6, cls=dict(kernel="f6", tp=8, pref=1, nchunks=1)),
    Case("f6 tp8 2x2x24->40", 2, 19, 40, 40, [S(2, 2, 24)], F6, cls=dict(kernel="f6", tp=8, pref=0, nchunks=3)),            # 8 blocks: remap
    Case("f6 tp8 1x5x24->40", 1, 9, 33, 40, [S(1, 5, 24)], F6, cls=dict(kernel="f6", tp=8, pref=0)),
    Case("f6 tp8 1x1x8->16", 1, 9, 33, 16, [S(1, 1, 8)], F6, cls=dict(kernel="f6", tp=8, direct=0, nchunks=1)),             # 1x1, one group: not direct
    Case("f6 tp8 1x1x40->65", 1, 19, 40, 65, [S(1, 1, 40)], F6, cls=dict(kernel="f6", tp=8, direct=0, pref=0, nt=3)),       # 1x1, cout > 64: not direct
    # tp = 12
    Case("f6 tp12 3x3x8->16", 1, 9, 33, 16, [S(3, 3, 8)], F6, cls=dict(kernel="f6", tp=12, pref=1, nchunks=1)),
    Case("f6 tp12 3x3x24->40", 1, 19, 40, 40, [S(3, 3, 24)], F6, g8=True, cls=dict(kernel="f6", tp=12, pref=0, nchunks=3)),
    Case("f6 tp12 2x5x24->128", 1, 9, 33, 128, [S(2, 5, 24)], F6, cls=dict(kernel="f6", tp=12, pref=0, nt=4)),
    # tp = 16
    Case("f6 tp16 3x5x8->16", 1, 3, 5, 16, [S(3, 5, 8)], F6, cls=dict(kernel="f6", tp=16, pref=1, nchunks=1)),              # image smaller than a tile
    Case("f6 tp16 3x5x24->40", 1, 19, 40, 40, [S(3, 5, 24)], F6, cls=dict(kernel="f6", tp=16, pref=1, nchunks=3)),
    Case("f6 tp16 2x7x24->65", 1, 9, 33, 65, [S(2, 7, 24)], F6, act="relu", cls=dict(kernel="f6", tp=16, pref=1, nt=3)),
    # tp = T
    Case("f6 tpT 4x4x8->16", 1, 9, 33, 16, [S(4, 4, 8)], F6, cls=dict(kernel="f6", tp=16, pref=1, nchunks=1)),
    Case("f6 tpT 4x4x24->40", 1, 19, 40, 40, [S(4, 4, 24)], F6, cls=dict(kernel="f6", tp=16, pref=1, nchunks=3)),
    Case("f6 tpT 5x5x40->40", 1, 19, 40, 40, [S(5, 5, 40)], F6, g8=True, cls=dict(kernel="f6", tp=25, pref=1, nchunks=5)),
    Case("f6 tpT 7x7x24->96", 1, 9, 33, 96, [S(7, 7, 24)], F6, cls=dict(kernel="f6", tp=49, pref=1, nt=3)),
    # the direct 1x1 path: 2, 8, 9, 17 and 25 channel groups, a last group that is not full
    Case("f6 direct 1x1x16->16", 1, 9, 33, 16, [S(1, 1, 16)], F6, cls=dict(kernel="f6", direct=1, stages=1)),
    Case("f6 direct 1x1x64->40", 1, 19, 40, 40, [S(1, 1, 64)], F6, cls=dict(kernel="f6", direct=1, stages=1, nt=2)),
    Case("f6 direct 1x1x68->64", 2, 19, 40, 64, [S(1, 1, 68)], F6, g8=True, cls=dict(kernel="f6", direct=1, stages=2, nt=2)),   # 9 groups, 4 channels in the last
    Case("f6 direct 1x1x132->33", 1, 9, 33, 33, [S(1, 1, 132)], F6, cls=dict(kernel="f6", direct=1, stages=3)),               # 17 groups
    Case("f6 direct 1x1x200->16", 1, 9, 33, 16, [S(1, 1, 200)], F6, cls=dict(kernel="f6", direct=1, stages=4)),               # 25 groups: the ring wraps
    # seg_flip: one cout tile, two segments, blocks 256.. walk the segments backwards.  65 images of 32x64 = 260
    # blocks (no remap); 66 images = 264 blocks, a multiple of 8 (remap)
    # block scales that differ between neighbouring blocks (gexp): a tap stream whose blocks span two groups (tp 12, tp T),
    # the direct path, whose blocks hold four groups, and conv_mfma_kernel for the fp16 planes
    Case("scales 3x3x24->40", 1, 19, 40, 40, [S(3, 3, 24, gexp=2)], (1, 2, 3), cls=dict(kernel="f6", tp=12), cls_prec=2),
    Case("scales 5x5x40->65", 1, 9, 33, 65, [S(5, 5, 40, gexp=2)], (1, 2, 3), cls=dict(kernel="f6", tp=25), cls_prec=2),
    Case("scales 1x1x68->40", 1, 19, 40, 40, [S(1, 1, 68, gexp=2)], (1, 2, 3), g8=True, cls=dict(kernel="f6", direct=1), cls_prec=2),
    Case("f6 seg_flip 260 blocks", 65, 32, 64, 16, [S(5, 5, 16), S(1, 1, 16)], F6, cls=dict(kernel="f6", nt=1)),
    Case("f6 seg_flip 264 blocks", 66, 32, 64, 16, [S(5, 5, 16), S(1, 1, 16)], F6, act="relu", cls=dict(kernel="f6", nt=1)),
] + [
    # ---- non-square filters on all three families: lo-exact 24 -> 40, integers 3 -> 5 on conv_small_kernel --------
    Case("nonsquare %dx%dx24->40" % k, 1, 19, 40, 40, [S(k[0], k[1], 24)], (1, 2, 3)) for k in ((1, 7), (7, 1), (3, 5), (2, 3), (1, 3))
] + [
    Case("nonsquare small %dx%dx3->5" % k, 1, 19, 70, 5, [S(k[0], k[1], 3)], (3,), cls=dict(kernel="small"))
    for k in ((1, 7), (7, 1), (3, 5), (2, 3), (1, 3))
] + [
    # ---- pad_hi = 1 for even filters on all three families --------------------------------------------------------
    Case("pad_hi %dx%dx24->40" % k, 1, 19, 40, 40, [S(k[0], k[1], 24, pad_hi=1)], (1, 2, 3)) for k in ((2, 2), (4, 4), (6, 6), (2, 3))
] + [
    Case("pad_hi small %dx%dx3->5" % k, 1, 19, 70, 5, [S(k[0], k[1], 3, pad_hi=1)], (3,), cls=dict(kernel="small"))
    for k in ((2, 2), (4, 4), (6, 6), (2, 3))
]

# ---- segments: three and four per launch, different filters, up_log2 0 / 1 / 4, channel windows of wider G8 tensors,
# pad_hi 0 and 1 mixed.  Checked at every precision and in every rotation (partial sums are exact: same bits).
SEG_CASES = [
    Case("3 segments 5x5 + 1x1 + 3x3", 2, 32, 64, 40,
         [S(5, 5, 24, c_off=8, c_total=40), S(1, 1, 16, up_log2=1), S(3, 3, 16, up_log2=4, c_off=16, c_total=40)], (1, 2, 3), g8=True),
    Case("4 segments 5x5 + 1x1 + 3x3 + 1x7", 1, 16, 48, 65,
         [S(5, 5, 16), S(1, 1, 24, up_log2=4, c_off=8, c_total=32), S(3, 3, 8, up_log2=1), S(1, 7, 24, c_off=16, c_total=48)], (1, 2, 3)),
    Case("4 segments pad_hi mix", 1, 16, 32, 16,
         [S(4, 4, 16, pad_hi=1), S(2, 2, 16), S(1, 1, 16, up_log2=4), S(2, 3, 8, pad_hi=1, up_log2=1)], (1, 2, 3), act="relu"),
    Case("3 segments small", 1, 16, 80, 5, [S(3, 3, 3), S(1, 1, 8, up_log2=4), S(2, 2, 2, pad_hi=1, up_log2=1)], (3,), g8=True, cls=dict(kernel="small")),
]

# pad_hi changes nothing for odd filters
PAD_HI_ODD = [
    Case("pad_hi odd 3x3x24->40", 1, 19, 40, 40, [S(3, 3, 24, pad_hi=1)], (1, 2, 3)),
    Case("pad_hi odd 1x5x24->40", 1, 9, 33, 40, [S(1, 5, 24, pad_hi=1)], (1, 2, 3)),
    Case("pad_hi odd small 5x5x3->5", 1, 19, 70, 5, [S(5, 5, 3, pad_hi=1)], (3,), cls=dict(kernel="small")),
]

# in_amax: the data times 2^-30 and 2^+10, converted with the power-of-two scale of max |x|
AMAX_CASES = [
    Case("in_amax 3x3x24->40", 1, 19, 40, 40, [S(3, 3, 24)], (1, 2, 3)),
    Case("in_amax 1x1x40->16 + 4x4x16", 1, 9, 33, 16, [S(1, 1, 40), S(4, 4, 16, pad_hi=1)], (1, 2, 3)),
    Case("in_amax small 3x3x3->5", 1, 19, 70, 5, [S(3, 3, 3)], (3,), cls=dict(kernel="small")),
]
AMAX_EXPONENTS = (-30, 10)

# post_add into a channel window of a 12-channel fp32 tensor at offset 3 (small outputs take the MFMA kernels then)
POST_ADD_CASES = [
    Case("post_add 3x3x24->8", 1, 19, 40, 8, [S(3, 3, 24)], (1, 2, 3)),
    Case("post_add 3x3x24->5", 2, 9, 33, 5, [S(3, 3, 24)], (1, 2, 3), g8=True),
]
POST_ADD_STRIDE, POST_ADD_COFF = 12, 3

ALL_CASES = CASES + SEG_CASES + PAD_HI_ODD + AMAX_CASES + POST_ADD_CASES
