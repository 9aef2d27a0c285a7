"""Data, case lists and float64 reference of the bit-exact suite of the small-channel convolutions
(test_conv_small_exact_gpu.py, test_conv_small_exact_host.py): conv_small_kernel and conv_small_pair_kernel of
csrc/mpgan_conv_small.hip.

Both kernels form hi + lo in fp32 and then run one chain of fmaf, so a result is exact when every partial sum is an fp32
number.  Two kinds of data give that with NON-ZERO lo planes:

  x-fine   activations lo_exact(f = 13): hi = +-1, lo = hi l 2^-13 with l in 0..3; filters ternary {-1, 0, 1}
  w-fine   activations ternary; filters lo_exact(f = 13), packed with wscale = 2^-4, a cout_scale of powers of two in
           [1/4, 4] and as a channel window of a wider HWIO filter (all of it undone exactly by the packer): an fp32
           table that was rounded to fp16, or scaled or addressed wrongly, shows

Biases are multiples of 1/4.  Every product is then a multiple of 2^-13, and where the sum of |term| of an output stays
below 2^11 every partial sum of it, in any order, is a multiple of 2^-13 below 2^11: 24 bits, an fp32 number.  That
bound is a condition on the data that the host test evaluates per output; it is no tolerance.  The expectation is the
float64 sum of the full products (hi + lo) * w, plus bias, then relu or nothing (one side is always coarse: there is no
lo * lo to leave out).

A launch that ends in relu gets a bias that puts each channel's mean one to two standard deviations above zero, so that
the clamp acts and more than half of the outputs still carry the lo parts: the host test proves that every case would
fail if the fine side lost its lo part.

Nothing here touches the GPU or the library under test.  chan_bound(), form(), weight_read(), pair_bounds() and
pair_lds_bytes() restate the dispatch of mpgan_conv_small.hip; they label the cases and never give an expectation.
"""
import functools
import zlib

import numpy as np

from conv_exact_ref import correlate, g8_roundtrip, lo_exact, mismatch_report, rotations, split16, upsample_nearest  # noqa: F401

FRAC = 13
BOUND = 2.0 ** 11          # in units of 1: 24 bits at 2^-13
TH, TW = 16, 64            # output tile of a workgroup of both kernels
N, H, W = 2, 19, 70        # two ragged tiles each way, 8 blocks per image, a batch offset above zero
LDS_MAX = 160 * 1024
SM_RPT = 4
BOUNDS = (1, 2, 4, 8)


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch of mpgan_conv_small.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
def chan_bound(c):
    """channels rounded up to 1, 2, 4, 8"""
    return 1 if c <= 1 else 2 if c <= 2 else 4 if c <= 4 else 8


def form(cs, cob, kh, kw):
    """which form of the column sums small_filter<CS, COUTB> takes: fixed forms exist only when CS * COUTB < 64"""
    if cs * cob < 64 and (kh, kw) == (5, 5):
        return "5x5"
    if cs * cob < 64 and (kh, kw) == (1, 1):
        return "1x1"
    return "run"


def weight_read(cs, cob):
    """shape of the LDS weight reads of small_column at NW = CS * COUTB weights per tap"""
    nw = cs * cob
    return {1: "scalar", 2: "float2"}.get(nw, "float4 block" if nw <= 16 else "float4 per channel")


def kx_unrolled(cs, cob, kh, kw):
    return form(cs, cob, kh, kw) != "run" and cs * cob <= 16


def stage_label(cs, cob, kh, kw):
    return (cs, cob, form(cs, cob, kh, kw), weight_read(cs, cob), kx_unrolled(cs, cob, kh, kw))


def pair_bounds(cin, cmid, cout):
    """the instantiation conv_small_pair_kernel<CINB, CMIDB, COUTB> mpg_conv2d_small_pair picks"""
    return (1 if cin == 1 else 4 if cin <= 4 else 8, 2 if cmid <= 2 else 8, 1 if cout == 1 else 8)


def _up4(n):
    return (n + 3) & ~3


def pair_lds_bytes(cin, cmid, cout, ka, kb, ks=None):
    """dynamic LDS of a pair launch: input tile, middle tile and three tables, each rounded up to 16 bytes"""
    ci, cm, co = pair_bounds(cin, cmid, cout)
    mw, mh = TW + kb[1] - 1, TH + kb[0] - 1
    mgroups = (mh + SM_RPT - 1) // SM_RPT
    xw, xh = mw + ka[1] - 1, mgroups * SM_RPT + ka[0] - 1
    x_px, mid_px = xw * xh, mw * (mgroups * SM_RPT + kb[0] - 1)
    floats = (_up4(x_px * ci) + _up4(mid_px * cm) + _up4(ka[0] * ka[1] * ci * cm) + _up4(kb[0] * kb[1] * cm * co)
              + _up4(ks[0] * ks[1] * ci * co if ks is not None else 0))
    return 4 * floats


def last_pass_pixels(kh, kw):
    """pixels of a single launch's halo tile that its last pass of 256 threads holds"""
    npx = (TW + kw - 1) * (TH + kh - 1)
    return npx - 256 * ((npx - 1) // 256)


def pair_tile_pixels(ka, kb):
    """(pixels of the input tile of a pair launch, moved in passes of 256 threads; those of them that stage A uses: the
    tile is rounded up to whole groups of SM_RPT middle rows, and the rows past the middle tile are read, never used)"""
    mw, mh = TW + kb[1] - 1, TH + kb[0] - 1
    xw = mw + ka[1] - 1
    return xw * ((mh + SM_RPT - 1) // SM_RPT * SM_RPT + ka[0] - 1), xw * (mh + ka[0] - 1)


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def ternary(rng, shape, share=1.0):
    """(v float32, hi, lo): -1, 0, 1 with `share` of non-zeros; no lo part"""
    v = rng.choice([-1.0, 0.0, 1.0], size=shape, p=[share / 2, 1.0 - share, share / 2])
    return v.astype(np.float32), v, np.zeros(shape)


def grid_bits(a):
    """the smallest g >= 0 with a 2^g integral everywhere (14 where there is none up to 13)"""
    a = np.asarray(a, dtype=np.float64)
    for g in range(FRAC + 1):
        if np.array_equal(a * 2.0 ** g, np.round(a * 2.0 ** g)):
            return g
    return FRAC + 1


def quarter_bias(rng, cout, pre=None, whole=False):
    """multiples of 1/4 (whole numbers with `whole`): small and of either sign, or -- given the sums `pre` of a launch that
    ends in relu -- what puts each channel's mean one to two of its standard deviations above zero"""
    if pre is None:
        b = rng.integers(-8, 9, size=cout) / 4.0
    else:
        mean, std = pre.mean(axis=(0, 1, 2)), np.maximum(pre.std(axis=(0, 1, 2)), 1.0)
        b = np.round((rng.uniform(1.0, 2.0, size=cout) * std - mean) * 4.0) / 4.0
    return np.round(b) if whole else b


class Packing(object):
    """how an effective filter w [kh, kw, cin, cout] reaches mpg_conv_pack_weights: raw = the HWIO tensor handed over,
    of which channels c_off .. c_off + cin are packed, times wscale, times cout_scale per output channel"""

    def __init__(self, rng, w, fine):
        self.c_off, self.wscale, self.cout_scale, self.raw = 0, 1.0, None, np.ascontiguousarray(w, dtype=np.float32)
        if fine:
            kh, kw, cin, cout = w.shape
            self.c_off = int(rng.integers(1, 4))
            total = self.c_off + cin + int(rng.integers(1, 3))
            self.wscale = 2.0 ** -4
            self.cout_scale = (2.0 ** rng.integers(-2, 3, size=cout)).astype(np.float32)
            raw = lo_exact(rng, (kh, kw, total, cout), FRAC)[0].astype(np.float64)      # foreign channels: the same kind
            raw[:, :, self.c_off:self.c_off + cin] = w
            self.raw = (raw * 2.0 ** 4 / self.cout_scale).astype(np.float32)

    def effective(self, cin):
        """what the packer is to make of raw, in float64"""
        w = self.raw[:, :, self.c_off:self.c_off + cin].astype(np.float64) * self.wscale
        return w if self.cout_scale is None else w * self.cout_scale.astype(np.float64)


def _make(rng, shape, fine, share=1.0):
    return lo_exact(rng, shape, FRAC) if fine else ternary(rng, shape, share)


def _source(x, s, goff=0):
    """the segment's channel window of its source tensor (goff: of the window goff channels further), upsampled"""
    win = x[..., s.c_off + goff:s.c_off + goff + s.cin]
    if s.up_x_only:
        return np.repeat(win, 1 << s.up_log2, axis=2)
    return upsample_nearest(win, s.up_log2)


def _act(e, act):
    assert act in (None, "relu"), "only the exact activations"
    return np.maximum(e, 0.0) if act == "relu" else e


# ---------------------------------------------------------------------------------------------------------------------
# single launch
# ---------------------------------------------------------------------------------------------------------------------
class Seg(object):
    """one segment: kh x kw over `cin` channels from channel c_off of the c_total-channel source `src` (segments that
    name the same source share one tensor), stored at 1 / 2^up_log2 of the output (up_x_only: of its columns)"""

    def __init__(self, kh, kw, cin, up_log2=0, up_x_only=0, pad_hi=0, c_off=0, c_total=None, src=None):
        self.kh, self.kw, self.cin, self.up_log2, self.up_x_only, self.pad_hi, self.c_off = kh, kw, cin, up_log2, up_x_only, pad_hi, c_off
        self.c_total = c_off + cin if c_total is None else c_total
        self.src = src
        self.window = bool(c_off or self.c_total != cin)

    def __repr__(self):
        return "Seg(%dx%dx%d up %d%s pad_hi %d c_off %d of %d)" % (self.kh, self.kw, self.cin, self.up_log2, "x" if self.up_x_only else "",
                                                                    self.pad_hi, self.c_off, self.c_total)


class Case(object):
    """one launch of conv_small_kernel.  kind: "x" (x-fine) or "w" (w-fine); tags: what the case is in the list for"""

    def __init__(self, name, cout, segs, kind="x", act=None, n=N, h=H, w=W, prec=3, bias=True, tags=()):
        assert cout <= 8 and all(s.cin <= 8 for s in segs) and kind in ("x", "w")
        self.name, self.cout, self.segs, self.kind, self.act = name, cout, list(segs), kind, act
        self.n, self.h, self.w, self.prec, self.bias, self.tags = n, h, w, prec, bias, tuple(tags)

    @property
    def cob(self):
        return chan_bound(self.cout)

    @property
    def cinb(self):
        return chan_bound(max(s.cin for s in self.segs))

    def labels(self):
        """(COUT, CINB, [(CS, COUT, form, weight-read class, kx unrolled) per segment]) the launch runs"""
        return self.cob, self.cinb, [stage_label(chan_bound(s.cin), self.cob, s.kh, s.kw) for s in self.segs]

    def __repr__(self):
        return self.name


class CaseData(object):
    def __init__(self, case):
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        self.case, self.src, self.names, self.w, self.pack = case, {}, [], [], []
        for i, s in enumerate(case.segs):
            assert case.w % (1 << s.up_log2) == 0 and (s.up_x_only or case.h % (1 << s.up_log2) == 0), (case, s)
            name = s.src if s.src is not None else "seg%d" % i
            shape = (case.n, case.h >> (0 if s.up_x_only else s.up_log2), case.w >> s.up_log2, s.c_total)
            if name not in self.src:
                self.src[name] = _make(rng, shape, case.kind == "x", 2.0 / 3.0)
            assert self.src[name][0].shape == shape, (case, s)
            self.names.append(name)
            w = _make(rng, (s.kh, s.kw, s.cin, case.cout), case.kind == "w")
            self.w.append(w)
            self.pack.append(Packing(rng, w[0], case.kind == "w"))
        self.bias = None
        if case.bias:
            self.bias = quarter_bias(rng, case.cout, self.sums() if case.act == "relu" else None)

    def sums(self, hi_only=False, goff=None, absolute=False):
        """float64 sum over the segments.  hi_only: the fine side without its lo part; goff: segment -> shift of its
        channel window (a wrong group); absolute: of |x| and |w|, the bound on every partial sum"""
        e = 0.0
        for i, (s, name, (_, wh, wl)) in enumerate(zip(self.case.segs, self.names, self.w)):
            _, xh, xl = self.src[name]
            x, w = xh + xl, wh + wl
            if hi_only:
                x, w = (xh, w) if self.case.kind == "x" else (x, wh)
            if absolute:
                x, w = np.abs(x), np.abs(w)
            e = e + correlate(_source(x, s, goff(i) if goff else 0), w, s.pad_hi)
        return e

    def bias64(self):
        return 0.0 if self.bias is None else self.bias

    def abs_sum(self):
        return self.sums(absolute=True) + np.abs(self.bias64())

    def expected64(self, **kw):
        return _act(self.sums(**kw) + self.bias64(), self.case.act)

    def expected(self):
        return self.expected64().astype(np.float32)

    def wrong_group(self, i):
        """a neighbouring channel group of segment i's window"""
        s = self.case.segs[i]
        return 8 if s.c_off + 8 + s.cin <= s.c_total else -8


@functools.lru_cache(maxsize=4)
def case_data(case):
    return CaseData(case)


# counts that reach each bound: ragged and full
RAGGED_CIN = {1: 1, 2: 2, 4: 3, 8: 7}
RAGGED_COUT = {1: 1, 2: 2, 4: 3, 8: 5}


def _forms():
    """every (COUT, CINB) instantiation at 5x5 and 1x1 (x-fine) and at run-time 3x3 (w-fine); across the three the
    bounds 4 and 8 are reached by a ragged and by a full channel count on both sides"""
    out = []
    for cob in BOUNDS:
        for cib in BOUNDS:
            rc, ro = RAGGED_CIN[cib], RAGGED_COUT[cob]
            for k, cin, cout, kind, act, prec in ((5, rc, cob, "x", "relu", 2), (1, cib, ro, "x", None, 3), (3, rc, ro, "w", None, 3),):
                out.append(Case("forms %dx%dx%d->%d" % (k, k, cin, cout), cout, [Seg(k, k, cin)], kind, act, prec=prec, tags=("forms",)))
            if cib >= 4 and cob >= 4:       # the full count of both bounds in one launch
                out.append(Case("forms 3x3x%d->%d" % (cib, cob), cob, [Seg(3, 3, cib)], "w", "relu", prec=2, tags=("forms",)))
    return out


FORM_CASES = _forms()

# run-time sizes that stress the tile passes (7x7: 4 pixels in the last one) and the row buffer, at float4-per-channel
# weight reads (NW 32 or 64)
SIZE_CASES = [
    Case("size 7x7x7->8", 8, [Seg(7, 7, 7)], "x", "relu", prec=2, tags=("size",)),
    Case("size 7x7x8->5", 5, [Seg(7, 7, 8)], "w", None, tags=("size",)),
    Case("size 1x7x8->3", 3, [Seg(1, 7, 8)], "x", None, tags=("size",)),
    Case("size 7x1x4->8", 8, [Seg(7, 1, 4)], "w", "relu", tags=("size",)),
    Case("size 2x2x8->4", 4, [Seg(2, 2, 8)], "x", None, tags=("size",)),
    Case("size 2x2x7->8 pad_hi", 8, [Seg(2, 2, 7, pad_hi=1)], "w", None, prec=2, tags=("size",)),
    Case("size 4x4x3->8", 8, [Seg(4, 4, 3)], "x", "relu", tags=("size",)),
    Case("size 4x4x8->8 pad_hi", 8, [Seg(4, 4, 8, pad_hi=1)], "x", None, tags=("size",)),
]

# segments narrower than the launch's bound (CS < CINB); every rotation must give the same bits
SEG_CASES = [
    Case("segments 5x5x2 + 1x1x8 -> 1", 1, [Seg(5, 5, 2), Seg(1, 1, 8)], "x", "relu", prec=2, tags=("segments",)),
    Case("segments 3x3x1 + 5x5x4 up1 + 1x1x2 up4 + 1x7x8 -> 3", 3,
         [Seg(3, 3, 1), Seg(5, 5, 4, up_log2=1), Seg(1, 1, 2, up_log2=4), Seg(1, 7, 8)], "x", None, h=32, w=80, tags=("segments",)),
]

# upsampled sources with fine data
UP_CASES = [
    Case("up 1 3x3x3->5", 5, [Seg(3, 3, 3, up_log2=1)], "x", None, h=20, w=72, tags=("up",)),
    Case("up 2 5x5x8->2", 2, [Seg(5, 5, 8, up_log2=2)], "x", "relu", h=20, w=72, prec=2, tags=("up",)),
    Case("up 4 3x3x2->8", 8, [Seg(3, 3, 2, up_log2=4)], "x", None, h=32, w=80, tags=("up",)),
    Case("up 2 columns 5x5x1->8", 8, [Seg(5, 5, 1, up_log2=2, up_x_only=1)], "x", "relu", w=72, tags=("up",)),
    Case("up 2 columns 1x1x8->1 + 3x3x2", 1, [Seg(1, 1, 8, up_log2=2, up_x_only=1), Seg(3, 3, 2)], "x", None, w=72, tags=("up",)),
]

# channel windows of a 24-channel G8 tensor whose every other channel holds data of the same kind
WINDOW_CASES = [
    Case("window 3x3x%d at 8 of 24 -> %d" % (cin, cout), cout, [Seg(3, 3, cin, c_off=8, c_total=24)], "x", act, tags=("window",))
    for cin, cout, act in ((1, 8, None), (3, 4, "relu"), (8, 2, None))
] + [
    Case("windows 5x5x8 at 0 + 1x1x3 at 16 of 24 -> 5", 5,
         [Seg(5, 5, 8, c_off=0, c_total=24, src="t"), Seg(1, 1, 3, c_off=16, c_total=24, src="t")], "x", "relu", prec=2, tags=("window",)),
]

# in_amax: the activations times 2^e, converted with the power-of-two scale of max |x|; no bias (it is added behind the
# scale, and 2^-30 times a sum plus a quarter is no fp32 number)
AMAX_CASES = [
    Case("in_amax 3x3x3->5", 5, [Seg(3, 3, 3)], "x", None, bias=False, tags=("amax",)),
    Case("in_amax 5x5x2 + 1x1x8 -> 4", 4, [Seg(5, 5, 2), Seg(1, 1, 8)], "x", None, bias=False, prec=2, tags=("amax",)),
]
AMAX_EXPONENTS = (-30, 10)

PLAIN_CASES = FORM_CASES + SIZE_CASES + UP_CASES + WINDOW_CASES       # one launch each
SINGLE_CASES = PLAIN_CASES + SEG_CASES + AMAX_CASES


# ---------------------------------------------------------------------------------------------------------------------
# pair: act_b(conv_b(relu(conv_a(up(x)) + bias_a)) + conv_s(up(x)) + bias_b)
# ---------------------------------------------------------------------------------------------------------------------
class Pair(object):
    """one launch of conv_small_pair_kernel.  kind: "x" (x-fine, every filter ternary), "wa" (x ternary, filter A and
    the shortcut fine, filter B ternary) or "wb" (x and filter A ternary, bias A whole numbers: a whole-number middle;
    filter B and the shortcut fine).  shares: non-zero share of filter A and filter B."""

    def __init__(self, name, chans, ka, kb, ks, kind="x", act_b="relu", shares=(1.0, 1.0), up_log2=0, up_x_only=0, c_off=0,
                 c_total=None, n=N, h=H, w=W, prec=2, fits=True, tags=()):
        self.name, (self.cin, self.cmid, self.cout), self.ka, self.kb, self.ks = name, chans, ka, kb, ks
        self.kind, self.act_a, self.act_b, self.shares = kind, "relu", act_b, shares
        self.seg = Seg(ka[0], ka[1], self.cin, up_log2=up_log2, up_x_only=up_x_only, c_off=c_off, c_total=c_total)
        self.n, self.h, self.w, self.prec, self.fits, self.tags = n, h, w, prec, fits, tuple(tags)

    @property
    def inst(self):
        return pair_bounds(self.cin, self.cmid, self.cout)

    def labels(self):
        """the instantiation and the (CS, COUT, form, weight-read class, kx unrolled) of stage A, stage B, shortcut"""
        ci, cm, co = self.inst
        st = [stage_label(ci, cm, *self.ka), stage_label(cm, co, *self.kb)]
        return self.inst, st + ([stage_label(ci, co, *self.ks)] if self.ks is not None else [])

    def lds_bytes(self):
        return pair_lds_bytes(self.cin, self.cmid, self.cout, self.ka, self.kb, self.ks)

    def __repr__(self):
        return self.name


class PairData(object):
    def __init__(self, case):
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        s, k = case.seg, case.kind
        self.case = case
        shape = (case.n, case.h >> (0 if s.up_x_only else s.up_log2), case.w >> s.up_log2, s.c_total)
        self.x = _make(rng, shape, k == "x", 2.0 / 3.0)
        self.wa = _make(rng, case.ka + (case.cin, case.cmid), k == "wa", case.shares[0])
        self.wb = _make(rng, case.kb + (case.cmid, case.cout), k == "wb", case.shares[1])
        self.ws = _make(rng, case.ks + (case.cin, case.cout), k != "x") if case.ks is not None else None
        self.pack_a, self.pack_b = Packing(rng, self.wa[0], k == "wa"), Packing(rng, self.wb[0], k == "wb")
        self.pack_s = Packing(rng, self.ws[0], k != "x") if self.ws is not None else None
        self.bias_a = quarter_bias(rng, case.cmid, whole=(k == "wb"))
        self.bias_b = None
        self.bias_b = quarter_bias(rng, case.cout, self.pre_b() if case.act_b == "relu" else None)

    def _w(self, t, fine_name, hi_only):
        return t[1] if hi_only and self.case.kind == fine_name else t[1] + t[2]

    def _x(self, hi_only, goff, absolute=False):
        x = self.x[1] if hi_only and self.case.kind == "x" else self.x[1] + self.x[2]
        return _source(np.abs(x) if absolute else x, self.case.seg, goff)

    def mid(self, hi_only=False, goff=0):
        """the float64 middle tensor; zero outside the image, as filter B's SAME padding sees it"""
        return np.maximum(correlate(self._x(hi_only, goff), self._w(self.wa, "wa", hi_only)) + self.bias_a, 0.0)

    def pre_b(self, hi_only=False, goff=0):
        e = correlate(self.mid(hi_only, goff), self._w(self.wb, "wb", hi_only))
        if self.ws is not None:
            e = e + correlate(self._x(hi_only, goff), self.ws[1] if hi_only and self.case.kind != "x" else self.ws[1] + self.ws[2])
        return e + (0.0 if self.bias_b is None else self.bias_b)

    def abs_sum_a(self):
        return correlate(self._x(False, 0, True), np.abs(self.wa[1] + self.wa[2])) + np.abs(self.bias_a)

    def abs_sum_b(self):
        e = correlate(np.abs(self.mid()), np.abs(self.wb[1] + self.wb[2])) + np.abs(self.bias_b)
        if self.ws is not None:
            e = e + correlate(self._x(False, 0, True), np.abs(self.ws[1] + self.ws[2]))
        return e

    def expected64(self, **kw):
        return _act(self.pre_b(**kw), self.case.act_b)

    def expected(self):
        return self.expected64().astype(np.float32)

    def wrong_group(self):
        s = self.case.seg
        return 8 if s.c_off + 8 + s.cin <= s.c_total else -8


@functools.lru_cache(maxsize=4)
def pair_data(case):
    return PairData(case)


K1, K3, K5, K7 = (1, 1), (3, 3), (5, 5), (7, 7)
PAIR_INSTANCES = [(ci, cm, co) for ci in (1, 4, 8) for cm in (2, 8) for co in (1, 8)]


def _production():
    """(a) all 12 instantiations at 5x5 / 5x5 with a 1x1 shortcut, x-fine, with channel counts that reach each bound"""
    out = []
    for i, (ci, cm, co) in enumerate(PAIR_INSTANCES):
        cin = {1: 1, 4: (3, 4)[i % 2], 8: (7, 8)[(i // 2) % 2]}[ci]
        cmid = {2: 2, 8: (3, 8)[(i // 4 + i) % 2]}[cm]
        cout = {1: 1, 8: (5, 8)[(i // 2 + i // 4) % 2]}[co]
        shares = (1.0 if ci * cm < 64 else 0.5, 1.0 if cm == 2 else 0.5)
        out.append(Pair("pair %d->%d->%d 5x5/5x5/1x1" % (cin, cmid, cout), (cin, cmid, cout), K5, K5, K1, "x", ("relu", None)[i % 2],
                        shares, tags=("production",)))
    return out


PAIR_CASES = _production() + [
    # (b) run-time forms, all three cin bounds; a shortcut larger than filter A sits at a non-zero offset of the input tile
    Pair("pair 4->8->1 3x3/7x7/3x3", (4, 8, 1), K3, K7, K3, "x", "relu", (1.0, 0.5), tags=("runtime",)),
    Pair("pair 1->2->8 7x7/3x3/none", (1, 2, 8), K7, K3, None, "x", None, tags=("runtime",)),
    Pair("pair 7->2->8 1x1/5x5/5x5", (7, 2, 8), K1, K5, K5, "x", "relu", tags=("runtime",)),
    Pair("pair 3->2->5 7x7/3x3/none", (3, 2, 5), K7, K3, None, "x", "relu", tags=("runtime",)),
    Pair("pair 1->8->1 3x3/7x7/3x3", (1, 8, 1), K3, K7, K3, "x", None, (1.0, 0.5), tags=("runtime",)),
    # (c) w-fine
    Pair("pair 1->2->8 filter A fine", (1, 2, 8), K5, K5, K1, "wa", "relu", prec=3, tags=("w-fine",)),
    Pair("pair 8->2->1 filter B fine", (8, 2, 1), K5, K5, K1, "wb", None, prec=3, tags=("w-fine",)),
    # (d) upsampling and windows
    Pair("pair 1->2->8 up 2", (1, 2, 8), K5, K5, K1, "x", "relu", up_log2=2, h=20, w=72, tags=("up",)),
    Pair("pair 4->2->8 up 2 columns", (4, 2, 8), K5, K5, K1, "x", None, up_log2=2, up_x_only=1, w=72, tags=("up",)),
    Pair("pair 1->8->1 window at 8 of 24", (1, 8, 1), K5, K5, K1, "x", "relu", c_off=8, c_total=24, tags=("window",)),
    Pair("pair 8->2->1 window at 8 of 24", (8, 2, 1), K5, K5, K1, "x", None, c_off=8, c_total=24, tags=("window",)),
    # the ninth pass of the input tile (pixels 2048 ..) holds pixels that stage A uses only where both filters have 7 rows:
    # 24 of them at 7x5 / 7x7, 80 at 7x7 / 7x7, in tile rows 27 and 26 .. 27, which lie inside an image of 27 rows
    Pair("pair 3->2->1 7x5/7x7/3x3", (3, 2, 1), (7, 5), K7, K3, "x", None, h=27, tags=("passes",)),
    Pair("pair 1->2->8 7x7/7x7/none", (1, 2, 8), K7, K7, None, "x", "relu", h=27, tags=("passes",)),
    # (e) the LDS budget: 7x5 / 5x7 with a 3x3 shortcut fits at 8 -> 8 -> 8
    Pair("pair 8->8->8 7x5/5x7/3x3", (8, 8, 8), (7, 5), (5, 7), K3, "x", "relu", (0.5, 0.25), tags=("lds",)),
]

# ... and 7x7 / 7x7 does not: refused, nothing written
PAIR_TOO_LARGE = Pair("pair 8->8->8 7x7/7x7/3x3", (8, 8, 8), K7, K7, K3, "x", "relu", (0.5, 0.25), fits=False, tags=("lds",))
PAIR_TOO_LARGE_BYTES = 167552
