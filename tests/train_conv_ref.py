"""Cases, data, integer references and the restated launch arithmetic of the exact tests of mpgan_train_conv.hip
(mpg_conv2d_wgrad, mpg_conv2d_dgrad, mpg_fc_forward) and of mpg_conv2d_direct (test_train_conv_gpu.py; what is claimed
here is proven on the CPU by test_train_conv_host.py).

References: tf.nn.conv2d SAME on NHWC / HWIO with independent kh, kw, sh, sw, its two gradients and the matrix product
of the fully connected layer, in int64 numpy, as plain loops over output pixels and taps from the definition

    y[b, oy, ox, o] = sum_{ky, kx, c} x[b, oy sh + ky - pt, ox sw + kx - pl, c] w[ky, kx, c, o]

over the taps that fall inside the image (pt, pl: oracle.ops.same_pad).

Data, as the "exact" kind of conv_triad_ref: x, dy integers in [-3, 3], w integers in [-2, 2], bias integers in [-3, 3],
wscale = 2^-1, cout_scale powers of two, activations none / relu / lrelu with leak 2^-2.  Every product is an integer,
every fp32 partial sum of a contraction whose sum of |terms| stays below 2^23 is exact in any order (fp32 holds every
integer up to 2^24), and the scale, cout_scale, the bias and the three activations only produce multiples of 2^-6 far
below 2^24 of them.  That covers the fp32 atomics of wgrad_kernel and fc_splitk_kernel and every FMA chain, so the GPU
assertion is np.array_equal, without a tolerance.

Nothing here touches the GPU or the library under test.
"""
import collections
import functools
import zlib

import numpy as np

from oracle.ops import same_pad

WSCALE = 0.5
XMAX, WMAX, BMAX = 3, 2, 3
LEAK = 0.25
ACTS = (None, "relu", "lrelu")
COUT_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
EXACT_LIMIT = 2 ** 23


# ---------------------------------------------------------------------------------------------------------------------
# the launch arithmetic of mpgan_train_conv.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
WG_TK, WG_TARGET_BLOCKS, WG_MIN_PIX, WG_MAX_SPLIT = 8, 2048, 128, 65535       # wgrad_kernel: TK; launch_wgrad
FC_GROUP, FC_SPLIT_K, FC_SPLIT_BLOCKS, FC_TARGET_BLOCKS, FC_MIN_TERMS, FC_CHUNK = 64, 16384, 512, 1024, 2048, 256   # mpg_fc_forward
FILTER_MAX = 16                                                                # MPG_GEOM_CHECK


MICRO_THRESHOLDS = (16, 32, 64)                                                # micro()


def micro(c):
    """mpgan_train_conv.hip: micro() -- channels a thread holds of a (16 * micro) wide tile"""
    t2, t4, t8 = MICRO_THRESHOLDS
    return 8 if c > t8 else 4 if c > t4 else 2 if c > t2 else 1


def wgrad_launch(n, h, w, cin, cout, kh, kw, sh, sw):
    """mpgan_train_conv.hip: mpg_conv2d_wgrad + launch_wgrad -> (mi, ni, ci_tiles, co_tiles, split, pps): the
    wgrad_kernel<mi, ni> instantiation, the grid's channel tiles and the pixel split (pps pixels a slice)"""
    mi, ni = micro(cin), micro(cout)
    tm, tn = 16 * mi, 16 * ni
    ci_tiles, co_tiles = -(-cin // tm), -(-cout // tn)
    tiles = kh * kw * ci_tiles * co_tiles
    pix = n * -(-h // sh) * -(-w // sw)
    split = -(-WG_TARGET_BLOCKS // tiles)
    split = min(split, (pix + WG_MIN_PIX - 1) // WG_MIN_PIX)
    split = min(max(split, 1), WG_MAX_SPLIT)
    pps = -(-pix // split)
    pps = (pps + WG_TK - 1) // WG_TK * WG_TK
    split = -(-pix // pps)
    return mi, ni, ci_tiles, co_tiles, split, pps


def fc_plan(rows, k, cout):
    """mpgan_train_conv.hip: mpg_fc_forward -> ("one",) for fc_fwd_kernel, ("split", splits, kchunk) for
    fc_splitk_kernel + fc_finish_kernel"""
    ogroups = -(-cout // FC_GROUP)
    if k >= FC_SPLIT_K and rows * ogroups < FC_SPLIT_BLOCKS:
        splits = min(FC_TARGET_BLOCKS // (rows * ogroups), k // FC_MIN_TERMS)
        if splits > 1:
            kchunk = -(-(-(-k // splits)) // FC_CHUNK) * FC_CHUNK
            return "split", -(-k // kchunk), kchunk
    return ("one",)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class ConvCase(collections.namedtuple("ConvCase", "n h w cin cout kh kw sh sw why")):
    __slots__ = ()

    @property
    def geom(self):
        return tuple(self[:9])

    @property
    def out_hw(self):
        return -(-self.h // self.sh), -(-self.w // self.sw)

    @property
    def pixels(self):
        oh, ow = self.out_hw
        return self.n * oh * ow

    def __repr__(self):
        return "%dx%d_s%dx%d_%dto%d_n%d_%dx%d-%s" % (self.kh, self.kw, self.sh, self.sw, self.cin, self.cout, self.n, self.h,
                                                    self.w, self.why)


# the two channel counts of each micro() class: the smallest / the threshold, and for 8 one tile / two ragged tiles
MICRO_CLASSES = {1: (5, 16), 2: (17, 32), 4: (33, 64), 8: (65, 130)}


def _micro_cases():
    """all 16 wgrad_kernel<MI, NI> at (1, 5, 6, cin, cout, 3, 3, 1, 1); over the table both values of every class stand on
    both axes (cin takes value j % 2 of its class, cout value i % 2)"""
    out = []
    for i, mi in enumerate((1, 2, 4, 8)):
        for j, ni in enumerate((1, 2, 4, 8)):
            out.append(ConvCase(1, 5, 6, MICRO_CLASSES[mi][j % 2], MICRO_CLASSES[ni][i % 2], 3, 3, 1, 1, "wgrad_kernel_%d_%d" % (mi, ni)))
    return out


CONV_CASES = _micro_cases() + [
    ConvCase(1, 15, 20, 4, 4, 3, 3, 1, 1, "P300-3_splits_of_104-last_92"),
    ConvCase(1, 33, 31, 1, 1, 1, 1, 1, 1, "P1023-8_splits-last_127-one_tile"),
    ConvCase(2, 13, 17, 17, 33, 3, 5, 1, 2, "kh_ne_kw-sh_ne_sw-two_splits"),
    ConvCase(1, 2, 3, 8, 8, 3, 3, 1, 1, "P6_below_TK"),
    ConvCase(1, 1, 1, 40, 3, 3, 3, 1, 1, "P1-only_the_centre_tap"),
    ConvCase(2, 9, 7, 6, 12, 4, 4, 2, 2, "even_filter-stride2-odd_image"),
    ConvCase(2, 5, 8, 33, 16, 2, 2, 3, 3, "stride_above_filter-16_of_40_untouched"),
    ConvCase(2, 11, 5, 8, 130, 2, 7, 3, 1, "stride_above_filter-15_of_55_untouched"),
    ConvCase(1, 6, 6, 65, 65, 1, 1, 2, 2, "1x1_stride2"),
    ConvCase(2, 4, 9, 16, 17, 16, 1, 1, 1, "filter_limit_16"),
]

FcCase = collections.namedtuple("FcCase", "rows k cout why")

FC_CASES = [
    FcCase(1, 1, 1, "smallest"),
    FcCase(2, 3, 2, "k_below_the_4_lanes"),
    FcCase(1, 255, 1, "no1-k_below_BLK"),
    FcCase(1, 257, 129, "three_groups-last_has_one_output"),
    FcCase(2, 16383, 64, "one_pass-just_below_the_split"),
    FcCase(1, 16384, 65, "8_splits-second_group_has_one_output"),
    FcCase(3, 16387, 5, "8_chunks_of_2304-last_259"),
    FcCase(511, 16384, 1, "split_in_two"),
    FcCase(512, 16384, 1, "not_split-512_blocks"),
    FcCase(16, 262144, 1, "64_splits"),
]


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def _rng(case):
    return np.random.default_rng(zlib.crc32(repr(tuple(case[:-1])).encode()))


def _ints(rng, m, shape):
    a = rng.integers(-m, m + 1, size=shape, dtype=np.int64)
    while not a.any():              # a one-element filter drawn as 0 would make the case vacuous
        a = rng.integers(-m, m + 1, size=shape, dtype=np.int64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def conv_data(case):
    """int64 arrays x [n,h,w,cin], w [kh,kw,cin,cout], dy [n,oh,ow,cout], bias [cout]; float32 cout_scale [cout]"""
    rng = _rng(case)
    oh, ow = case.out_hw
    d = dict(x=_ints(rng, XMAX, (case.n, case.h, case.w, case.cin)), w=_ints(rng, WMAX, (case.kh, case.kw, case.cin, case.cout)),
             dy=_ints(rng, XMAX, (case.n, oh, ow, case.cout)), bias=_ints(rng, BMAX, (case.cout,)))
    cs = np.asarray(COUT_SCALES, np.float32)[rng.integers(0, len(COUT_SCALES), size=case.cout)]
    cs.setflags(write=False)
    d["cout_scale"] = cs
    return d


@functools.lru_cache(maxsize=None)
def fc_data(case):
    """int64 arrays x [rows,k], w [k,cout], bias [cout]"""
    rng = _rng(case)
    return dict(x=_ints(rng, XMAX, (case.rows, case.k)), w=_ints(rng, WMAX, (case.k, case.cout)), bias=_ints(rng, BMAX, (case.cout,)))


# ---------------------------------------------------------------------------------------------------------------------
# integer references
# ---------------------------------------------------------------------------------------------------------------------
def _taps(h, w, kh, kw, sh, sw):
    """(oy, ox, ky, kx, iy, ix) of every tap of every output pixel that reads inside the image"""
    oh, pt, _ = same_pad(h, kh, sh)
    ow, pl, _ = same_pad(w, kw, sw)
    for oy in range(oh):
        for ox in range(ow):
            for ky in range(kh):
                iy = oy * sh + ky - pt
                if not 0 <= iy < h:
                    continue
                for kx in range(kw):
                    ix = ox * sw + kx - pl
                    if 0 <= ix < w:
                        yield oy, ox, ky, kx, iy, ix


def _i64(a):
    a = np.asarray(a)
    assert a.dtype == np.int64, a.dtype
    return a


def fwd(x, wt, sh, sw):
    x, wt = _i64(x), _i64(wt)
    n, h, w, _ = x.shape
    kh, kw, _, cout = wt.shape
    y = np.zeros((n, -(-h // sh), -(-w // sw), cout), np.int64)
    for oy, ox, ky, kx, iy, ix in _taps(h, w, kh, kw, sh, sw):
        y[:, oy, ox, :] += x[:, iy, ix, :] @ wt[ky, kx]
    return y


def wgrad(x, dy, kh, kw, sh, sw):
    """-> (dw [kh,kw,cin,cout], the same sum over |x| |dy|: the sum of |terms| of each element's contraction)"""
    x, dy = _i64(x), _i64(dy)
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    assert dy.shape == (n, -(-h // sh), -(-w // sw), cout), dy.shape
    dw = np.zeros((kh, kw, cin, cout), np.int64)
    mag = np.zeros_like(dw)
    ax, ady = np.abs(x), np.abs(dy)
    for oy, ox, ky, kx, iy, ix in _taps(h, w, kh, kw, sh, sw):
        dw[ky, kx] += x[:, iy, ix, :].T @ dy[:, oy, ox, :]
        mag[ky, kx] += ax[:, iy, ix, :].T @ ady[:, oy, ox, :]
    return dw, mag


def dgrad(dy, wt, h, w, sh, sw):
    dy, wt = _i64(dy), _i64(wt)
    kh, kw, cin, cout = wt.shape
    n = dy.shape[0]
    assert dy.shape == (n, -(-h // sh), -(-w // sw), cout), dy.shape
    dx = np.zeros((n, h, w, cin), np.int64)
    for oy, ox, ky, kx, iy, ix in _taps(h, w, kh, kw, sh, sw):
        dx[:, iy, ix, :] += dy[:, oy, ox, :] @ wt[ky, kx].T
    return dx


def fc(x, w):
    return _i64(x) @ _i64(w)


def touched(h, w, kh, kw, sh, sw):
    """bool [h, w]: the input pixels some tap of some output pixel reads; bool [kh, kw]: the taps that ever read inside"""
    pix, tap = np.zeros((h, w), bool), np.zeros((kh, kw), bool)
    for _, _, ky, kx, iy, ix in _taps(h, w, kh, kw, sh, sw):
        pix[iy, ix] = True
        tap[ky, kx] = True
    return pix, tap


@functools.lru_cache(maxsize=None)
def conv_reference(case):
    """dict of read-only int64 arrays y, dw, dw_terms, dx and the sums of |terms| y_terms, dx_terms, once per case"""
    d = conv_data(case)
    dw, mag = wgrad(d["x"], d["dy"], case.kh, case.kw, case.sh, case.sw)
    r = dict(y=fwd(d["x"], d["w"], case.sh, case.sw), dw=dw, dw_terms=mag, dx=dgrad(d["dy"], d["w"], case.h, case.w, case.sh, case.sw),
             y_terms=fwd(np.abs(d["x"]), np.abs(d["w"]), case.sh, case.sw),
             dx_terms=dgrad(np.abs(d["dy"]), np.abs(d["w"]), case.h, case.w, case.sh, case.sw))
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def fc_reference(case):
    d = fc_data(case)
    r = dict(y=fc(d["x"], d["w"]), y_terms=fc(np.abs(d["x"]), np.abs(d["w"])))
    for v in r.values():
        v.setflags(write=False)
    return r


def epilogue(acc, wscale=WSCALE, cout_scale=None, bias=None, act=None, leak=LEAK):
    """what the kernels make of an integer contraction: act(acc * wscale [* cout_scale] [+ bias]) as float32.  Computed in
    float64, where every step is exact on this data, and cast without rounding (asserted)"""
    v = np.asarray(acc, np.float64) * wscale
    if cout_scale is not None:
        v = v * np.asarray(cout_scale, np.float64)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
    assert act in ACTS, act
    if act == "relu":
        v = np.maximum(v, 0.0)
    elif act == "lrelu":
        v = np.where(v >= 0.0, v, leak * v)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out + np.float32(0.0)          # -0.0 -> 0.0


def scaled_ints(a, wscale=WSCALE):
    """the integers a float32 kernel output stands for, a / wscale, as int64 (asserts that they are integers)"""
    v = np.asarray(a, np.float64) / wscale
    r = np.rint(v)
    assert np.array_equal(r, v), "not a multiple of %g" % wscale
    return r.astype(np.int64)


def mismatch_report(got, want, what=""):
    """'' when the float32 arrays are equal value for value (no NaN allowed); else where and by how much they differ"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if got.dtype != np.float32 or want.dtype != np.float32:
        return "%s: dtypes %s / %s, expected float32" % (what, got.dtype, want.dtype)
    bad = np.argwhere(~(got == want))
    if len(bad) == 0:
        return ""
    idx = tuple(int(v) for v in bad[0])
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return ("%s: %d of %d values differ (max |diff| %.3e); first at %s: got %r, expected %r"
            % (what, len(bad), got.size, float(np.nanmax(err)), idx, float(got[idx]), float(want[idx])))
