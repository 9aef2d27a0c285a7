"""numpy model, data and case tables of the direct tests of the G8 tensor functions (csrc/mpgan_g8.hip, mpg_absmax and
mpg::pow2_scale) -- test_g8_gpu.py; what is claimed here is proven on the CPU by test_g8_host.py.

A G8 tensor (include/mpgan.h) is [N][G = ceil(C/8)][2 planes: hi, lo][H][W][8 x fp16] with value = hi + lo.  Every
producer stores the canonical split of the fp32 value v it holds:

    hi = fp16(v)                      IEEE round to nearest even, gradual underflow
    lo = fp16(fp32(v) - fp32(hi))     the fp32 difference is exact

and +0 in both planes for the channels beyond C.  pack() is that definition on the uint16 image, byte for byte what
the library must store; unpack() is the reading direction, float32(hi) + float32(lo) as one fp32 add, on any planes.
numpy's float32 -> float16 conversion is round to nearest even with subnormals, its float32 arithmetic is IEEE with
subnormals: nothing here is taken from the library under test.

pow2_scale() is the scale law of mpg::pow2_scale as include/mpgan.h states it, kernel_for() a restatement of the
dispatch in mpg_f32_to_g8_scaled: each case names the kernel it is meant to reach and the host test holds the case
against the restatement.

The data makers have fixed seeds and return float32 vectors; mixed() interleaves all classes so that every case, whatever
its shape, sees all of them.

Nothing here touches the GPU or the library under test.
"""
import collections
import functools
import zlib

import numpy as np

F32 = np.float32
F16_MAX = 65504.0


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def split(v):
    """(hi, lo) float16 arrays of the canonical split of float32(v)"""
    v = np.asarray(v, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(F32)).astype(np.float16)
    return hi, lo


def groups(c):
    return (c + 7) // 8


def pack(x, c_off=0, cin=None, scale=1.0):
    """the uint16 image [N][G][2][H][W][8] of float32(x[..., c_off:c_off + cin] * scale); padding channels +0"""
    x = np.asarray(x, dtype=F32)
    n, h, w, c = x.shape
    cin = c - c_off if cin is None else cin
    assert 0 <= c_off and cin >= 1 and c_off + cin <= c
    with np.errstate(over="ignore", invalid="ignore"):
        v = x[..., c_off:c_off + cin] * F32(scale)         # one fp32 multiply, as the kernels do
    assert v.dtype == F32
    hi, lo = split(v)
    g = groups(cin)
    img = np.zeros((n, g, 2, h, w, 8), np.uint16)
    for plane, part in enumerate((hi, lo)):
        full = np.zeros((n, h, w, g * 8), np.uint16)
        full[..., :cin] = part.view(np.uint16)
        img[:, :, plane] = full.reshape(n, h, w, g, 8).transpose(0, 3, 1, 2, 4)
    return img


def unpack(img, c):
    """fp32 NHWC [N,H,W,c] of a uint16 G8 image: float32(hi) + float32(lo), one fp32 add; works on any planes"""
    img = np.asarray(img, dtype=np.uint16)
    n, g, two, h, w, eight = img.shape
    assert two == 2 and eight == 8 and g == groups(c)
    planes = img.view(np.float16).astype(F32)                           # exact
    with np.errstate(over="ignore", invalid="ignore"):
        s = planes[:, :, 0] + planes[:, :, 1]                           # [N][G][H][W][8]
    assert s.dtype == F32
    return np.ascontiguousarray(s.transpose(0, 2, 3, 1, 4).reshape(n, h, w, g * 8)[..., :c])


def pow2_scale(amax):
    """the scale law of include/mpgan.h as a float32: 1 for amax <= 0, NaN and amax >= 3.0e38; else 2^min(9 - e, 126) with
    amax = m 2^e, m in [0.5, 1).  The scale and its reciprocal are normal fp32 numbers."""
    a = F32(amax)
    if not (a > 0) or not (a < F32(3.0e38)):
        return F32(1.0)
    _, e = np.frexp(np.float64(a))              # float64 frexp: exact for every fp32 number, subnormals included
    return F32(2.0 ** min(9 - int(e), 126))


def pow2_scale_uncapped(amax):
    """the law before the cap, in float32 arithmetic: what the host test shows to be inf from 2^-119 down"""
    a = F32(amax)
    if not (a > 0) or not (a < F32(3.0e38)):
        return F32(1.0)
    _, e = np.frexp(np.float64(a))
    with np.errstate(over="ignore"):
        return np.ldexp(F32(1.0), 9 - int(e)).astype(F32)


def absmax(x):
    """max |x_i| over the elements that are not NaN, as a float32; +0 when there is none"""
    a = np.abs(np.asarray(x, dtype=F32).ravel())
    a = a[~np.isnan(a)]
    return F32(a.max()) if a.size else F32(0.0)


# the amax scalars of the scale-law table (the issue's list)
AMAX_TABLE = [
    ("0", F32(0.0)), ("-1", F32(-1.0)), ("2^8", F32(2.0 ** 8)), ("below 2^9", np.nextafter(F32(2.0 ** 9), F32(0.0))),
    ("2^9", F32(2.0 ** 9)), ("1", F32(1.0)), ("3e-5", F32(3e-5)), ("2^-30", F32(2.0 ** -30)), ("2^-100", F32(2.0 ** -100)),
    ("2^-118", F32(2.0 ** -118)), ("2^-119", F32(2.0 ** -119)), ("2^-120", F32(2.0 ** -120)), ("1e-37", F32(1e-37)),
    ("2^-126", F32(2.0 ** -126)), ("2^-140", F32(2.0 ** -140)), ("2.9e38", F32(2.9e38)), ("3.0e38", F32(3.0e38)),
    ("inf", F32(np.inf)), ("NaN", F32(np.nan)),
]


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def normal(size, seed="normal"):
    return _rng(seed).standard_normal(size).astype(F32)


def logmag(size, seed="logmag"):
    """random signs, magnitudes log-uniform in 2^-30 .. 2^15: hi in the fp16 subnormal range (below 2^-14) and flushed to
    zero (below 2^-25), lo subnormal and flushed for the larger ones"""
    rng = _rng(seed)
    return (rng.choice([-1.0, 1.0], size) * 2.0 ** rng.uniform(-30.0, 15.0, size)).astype(F32)


def ties(size, seed="ties"):
    """exact midpoints of two neighbouring fp16 numbers, hi +- half an ulp: a random finite fp16 pattern p (normal and
    subnormal, either sign, even and odd last bit) and the mean of p and its successor in magnitude, an fp32 number.
    Round to nearest even sends it to the even one of the two."""
    rng = _rng(seed)
    p = rng.integers(0, 0x7800, size).astype(np.uint16)           # magnitude patterns below 2^15: the successor is finite
    p[:4] = [0, 1, 0x03FF, 0x0400]                                  # 0|min subnormal, 1|2, last subnormal|first normal
    sign = (rng.integers(0, 2, size).astype(np.uint16) << 15).astype(np.uint16)
    a = (p | sign).view(np.float16).astype(np.float64)
    b = ((p + 1).astype(np.uint16) | sign).view(np.float16).astype(np.float64)
    v = ((a + b) / 2).astype(F32)
    assert np.array_equal(v.astype(np.float64), (a + b) / 2)       # 12 significant bits: exact in fp32
    return v


def edges():
    """the ends of the contract and of the formats: +-65504, 65519.9 (the largest fp32 values that still round to 65504
    are just below 65520), +-0, fp32 subnormals, the fp16 subnormal boundary, 2^-24 (smallest fp16) and the tie 2^-25"""
    tiny = np.array([1, 2, 0x00400000, 0x007FFFFF, 0x80000001, 0x807FFFFF], np.uint32).view(F32)      # fp32 subnormals
    return np.concatenate([
        np.array([F16_MAX, -F16_MAX, 65519.9, -65519.9, 0.0, -0.0, 1e-40, -1e-45], F32), tiny,
        np.array([2.0 ** -14, -2.0 ** -14, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26,
                  1.0, -1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -23, 2048.0 + 1.0, 0.1, -1e-3, 3e-5], F32)])


CLASSES = ("normal", "logmag", "ties", "edges")


def class_vector(kind, size, seed):
    if kind == "edges":
        return np.resize(edges(), size)
    return {"normal": normal, "logmag": logmag, "ties": ties}[kind](size, "%s %s" % (kind, seed))


def mixed(shape, seed="mixed"):
    """float32 tensor of `shape`: a quarter of its elements from each class, in a seeded random order, so that no class
    lines up with a channel, a group or a plane of any case"""
    size = int(np.prod(shape))
    k = len(CLASSES)
    per = (size + k - 1) // k
    out = np.concatenate([class_vector(kind, per, seed) for kind in CLASSES])
    return out[_rng("order %s" % seed).permutation(per * k)[:size]].reshape(shape)


def fp16_patterns(shape, seed):
    """uint16 array of random FINITE fp16 bit patterns, both signs, with subnormals and +-0 among them"""
    rng = _rng(seed)
    p = rng.integers(0, 0x7C00, shape).astype(np.uint16)
    flat = p.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 8))] = rng.integers(0, 0x0400, max(1, flat.size // 8)).astype(np.uint16)
    flat[rng.integers(0, flat.size, max(1, flat.size // 16))] = 0
    return p | (rng.integers(0, 2, shape).astype(np.uint16) << 15).astype(np.uint16)


NAN16 = np.array([0x7E00, 0xFE00, 0x7C01, 0xFFFF], np.uint16)         # quiet and signalling NaN patterns, both signs


def poison_padding(img, c):
    """a copy of the G8 image with NaN patterns in the lanes of the last group beyond c, in both planes"""
    img = img.copy()
    if c % 8:
        pad = img[:, -1, :, :, :, c % 8:]
        img[:, -1, :, :, :, c % 8:] = np.resize(NAN16, pad.shape)
    return img


# ---------------------------------------------------------------------------------------------------------------------
# mpg_f32_to_g8 / mpg_f32_to_g8_scaled: the dispatch and the cases
# ---------------------------------------------------------------------------------------------------------------------
PREDICATES = ("cin >= 32", "c % 4 == 0", "c_off % 4 == 0", "x 16-byte aligned", "n <= 65535")


def predicates(n, c, c_off, cin, misalign):
    """the five conditions of the tiled conversion, in the order of PREDICATES; misalign: bytes the base pointer is off a
    16-byte boundary"""
    return (cin >= 32, c % 4 == 0, c_off % 4 == 0, misalign % 16 == 0, n <= 65535)


def kernel_for(n, c, c_off, cin, misalign):
    return "tiled" if all(predicates(n, c, c_off, cin, misalign)) else "pixel"


class ToG8Case(collections.namedtuple("ToG8Case", "name n h w c c_off cin misalign kernel fails")):
    """one conversion: x [n, h, w, c] at `misalign` bytes off a 16-byte boundary, window [c_off, c_off + cin); `kernel`:
    the kernel the case is there for; `fails`: the one predicate it fails (None for the tiled and the narrow cases)"""
    __slots__ = ()

    def __repr__(self):
        return self.name

    @property
    def shape(self):
        return (self.n, self.h, self.w, self.c)


def _tc(n, h, w, c, c_off, cin, kernel="tiled", misalign=0, fails=None, note=""):
    name = "%s %dx%dx%dx%d [%d:+%d]%s%s" % (kernel, n, h, w, c, c_off, cin, " +%dB" % misalign if misalign else "", " " + note if note else "")
    return ToG8Case(name, n, h, w, c, c_off, cin, misalign, kernel, fails)


TILED_SHAPES = [(1, 1, 1, 32, 0, 32), (2, 3, 11, 36, 4, 32), (1, 1, 31, 36, 0, 33), (1, 1, 31, 36, 0, 34), (1, 1, 31, 36, 0, 35),
                (1, 5, 7, 132, 0, 129), (1, 2, 5, 264, 4, 260), (1, 1, 40, 64, 32, 32)]

TO_G8_CASES = [_tc(*s) for s in TILED_SHAPES] + [
    # the per-pixel kernel through each predicate of the dispatch, failed alone
    _tc(2, 3, 5, 32, 0, 31, "pixel", fails=PREDICATES[0]),
    _tc(2, 3, 5, 33, 0, 32, "pixel", fails=PREDICATES[1]),
    _tc(2, 3, 5, 36, 2, 32, "pixel", fails=PREDICATES[2]),
    _tc(2, 3, 5, 32, 0, 32, "pixel", misalign=4, fails=PREDICATES[3]),
    _tc(65536, 1, 1, 32, 0, 32, "pixel", fails=PREDICATES[4]),
    # narrow windows
    _tc(2, 3, 5, 19, 2, 17, "pixel", note="narrow"),
] + [_tc(2, 3, 5, 12, 1, cin, "pixel", note="narrow") for cin in (1, 3, 8, 9)] + [
    # more than one block of the per-pixel kernel (256 threads, one per pixel and group)
    _tc(1, 9, 31, 9, 0, 9, "pixel", note="two blocks"),
]


@functools.lru_cache(maxsize=2)
def to_g8_data(case):
    """the case's tensor: all four data classes in every channel group"""
    return mixed(case.shape, case.name)


def scaled_data(base, scale):
    """the tensor a scaled conversion is given: base / scale (a power of two; values that fall below the fp32 normal range
    lose bits or vanish, which is part of the data; values beyond the fp32 range, at the scales below 1, stop at its end),
    so that x * scale stays within the contract |v| <= 65504"""
    fmax = np.finfo(F32).max
    with np.errstate(under="ignore", over="ignore"):
        x = np.clip(np.asarray(base, dtype=np.float64) / np.float64(scale), -fmax, fmax).astype(F32)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the other tables
# ---------------------------------------------------------------------------------------------------------------------
FROM_G8_CHANNELS = (1, 7, 8, 13, 40)
FROM_G8_NHW = (2, 3, 5)

ABSMAX_SIZES = (0, 1, 3, 4, 5, 1023, 4099)
ABSMAX_BIG = 17 << 20            # the grid-stride loop under the 4096-block cap (16 elements per thread, 256 threads)


def absmax_positions(n, misalign):
    """{name: (index, value)} of the places the maximum is put for a tensor of n floats: first and last element, the
    float4 bulk and the scalar tail of the aligned path (with a base 4 bytes off every element is scalar work), once as a
    negative value"""
    if n == 0:
        return {}
    pos = {"first": (0, 7.5), "last": (n - 1, 7.5), "negative": (n // 2, -7.5)}
    n4 = (n // 4) * 4 if misalign == 0 else 0
    if n4 >= 8:
        pos["bulk"] = (n4 // 2 + 1, 7.5)
    if n4 and n > n4:
        pos["tail"] = (n4, 7.5)
    return pos


PN_CHANNELS = (1, 7, 8, 33, 36, 256, 257, 264, 505, 512)
PN_HW = ((1, 1), (7, 9), (5, 13))
PN_N = 2
PN_EPS = 1e-8


def pn_kernel(c):
    """waves per block of the pixel_norm_g8_kernel instantiation the host code picks: 4 up to 32 groups, else 8"""
    return 4 if groups(c) <= 32 else 8


def pn_input(c, h, w):
    """general data: Gaussian channels times a log-normal factor per pixel"""
    rng = _rng("pixel norm %d %d %d" % (c, h, w))
    return (rng.standard_normal((PN_N, h, w, c)) * np.exp(rng.standard_normal((PN_N, h, w, 1)))).astype(F32)


def pixel_norm64(x, eps=PN_EPS):
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt(np.mean(x * x, axis=3, keepdims=True) + eps)


# ---------------------------------------------------------------------------------------------------------------------
# the scale law at its consumers: all-positive lo-exact data
# ---------------------------------------------------------------------------------------------------------------------
def lo_exact_pos(rng, shape, frac=13):
    """(v float32, hi float64, lo float64): hi = +1, lo = l 2^-frac with l in 0..3, as conv_exact_ref.lo_exact without
    the signs: no sum of products cancels"""
    hi = np.ones(shape)
    lo = rng.integers(0, 4, size=shape) * 2.0 ** -frac
    return (hi + lo).astype(F32), hi, lo


def is_normal_f32(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return bool(np.all((a >= 2.0 ** -126) & (a < 2.0 ** 128)))


CONSUMER_E = -122               # activations times 2^-122: max |x| < 2^-119, where the uncapped scale is inf
WG_EX, WG_ED = -55, -60         # x and dy of the weight gradient: the two scales multiply to 2^131
WG_WSCALE = 0.5

ConvConsumer = collections.namedtuple("ConvConsumer", "name n h w cin cout k prec x wt expected64")
WgConsumer = collections.namedtuple("WgConsumer", "name n h w cin cout k prec x d expected64")


@functools.lru_cache(maxsize=None)
def conv_consumer(kind):
    """the two convolutions of the consumer test at unit scale.  "fused": 3x3x24->40 at MPG_PREC_F16X3, activations and
    weights lo-exact and positive; the expectation is the float64 sum of the three products a_hi w_hi + a_lo w_hi +
    a_hi w_lo (every term a multiple of 2^-13, 216 (1 + 6 2^-13) < 2^11: every fp32 partial sum is exact).  "small":
    3x3x3->5 on conv_small_kernel, which multiplies hi + lo by an fp32 weight in fp32: with lo-exact weights the products
    would carry lo lo terms of 2^-26 beside sums of 27 and no fp32 sum of them is exact, so its weights are the integers
    1..3 (as in conv_exact_ref) while its activations stay lo-exact and positive: the terms are multiples of 2^-13 with a
    sum below 2^7, exact in fp32 in any order and under fmaf.  The expectation is the float64 sum of (a_hi + a_lo) w."""
    from conv_exact_ref import correlate
    rng = _rng("consumer " + kind)
    if kind == "fused":
        n, h, w, cin, cout, prec = 1, 9, 33, 24, 40, 3
        x, xh, xl = lo_exact_pos(rng, (n, h, w, cin))
        wt, wh, wl = lo_exact_pos(rng, (3, 3, cin, cout))
        e = correlate(xh, wh) + correlate(xl, wh) + correlate(xh, wl)
    else:
        n, h, w, cin, cout, prec = 1, 9, 70, 3, 5, 3
        x, xh, xl = lo_exact_pos(rng, (n, h, w, cin))
        wt = rng.integers(1, 4, size=(3, 3, cin, cout)).astype(F32)
        e = correlate(xh + xl, wt)
    return ConvConsumer(kind, n, h, w, cin, cout, 3, prec, x, wt, e)


@functools.lru_cache(maxsize=None)
def wgrad_consumer():
    """3x3, 16 -> 32, MPG_PREC_F16X3 over 153 pixels, x and dy lo-exact and positive (wgrad_exact_ref: 153 (1 + 6 2^-13) <
    2^11); the expectation at unit scale, WG_WSCALE times the float64 sum of the three products"""
    from wgrad_exact_ref import wgrad64
    rng = _rng("consumer wgrad")
    n, h, w, cin, cout = 1, 9, 17, 16, 32
    x, xh, xl = lo_exact_pos(rng, (n, h, w, cin))
    d, dh, dl = lo_exact_pos(rng, (n, h, w, cout))
    e = WG_WSCALE * (wgrad64(xh, dh, 3, 3) + wgrad64(xl, dh, 3, 3) + wgrad64(xh, dl, 3, 3))
    return WgConsumer("wgrad", n, h, w, cin, cout, 3, 3, x, d, e)
