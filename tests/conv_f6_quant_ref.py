"""Numpy model of the bf6 (e3m2) quantisers of MPG_PREC_F16F6, and the data of test_conv_f6_quant_host.py /
test_conv_f6_quant_gpu.py.

The bit-exact suites on conv_exact_ref's lo-exact data pin addressing, barriers and which scale byte goes with which block;
on that data the bf6 quantisation is the identity.  Here the values have arbitrary exponents and mantissas, and the model
restates the arithmetic the source comments of csrc/mpgan_conv_pack.hip and csrc/mpgan_conv_f6.hip promise:

  K order   a segment's K axis is a stream of tap slots, slot = group * tp + tap (direct 1x1 path: slot = channel group);
            a stage is 8 slots, a BLOCK the 32 values (stage st, half hh): slots 8 st + 2 j + hh, j = 0..3, times 8
            channels.  The same partition for activations (per output pixel) and weights (per output channel).
  weights   v = w * wscale (* cout_scale) in fp32, hi = fp16(v), lo = v - hi.  Per block the scale exponents
            ilogb(max |v|) - 3 and ilogb(max |lo|) - 3, clamped to [-126, 120], 0 for an all-zero block; plane 0 holds the
            e3m2 codes of v / scale (of v, not of hi), plane 1 those of lo / scale_lo.
  activ.    e = biased fp16 exponent of the largest |a_hi| of the block; hi codes of a_hi 2^(18 - e), lo codes of
            a_lo 2^(30 - e); E8M0 bytes e + 109 and e + 97.  Padding slots (taps beyond the filter, groups beyond the
            segment) have zero weights, but the kernel reads real pixels for them, which enter the block maximum: tap (0, 0)
            of the group they pad in the image loop, the last group of the segment in the direct loop.
  result    y = sum a_hi w_hi + sum q(a_lo) q(w) + sum q(a_hi) q(w_lo), accumulated in fp32; a_lo w_lo is dropped.
  e3m2      sign, 3 exponent bits (bias 3), 2 mantissa bits, subnormals M 2^-4, no infinities; round to nearest even,
            saturating at 28 (OCP MX).

e3m2_quantise() works on the table of the 32 representable magnitudes and their midpoints, not on the packer's
ilogb / rint arithmetic.  decode_pack_image() is the only place that knows the byte layout of the weight image.
ALTERNATIVES are the slightly wrong quantisers the tests must be able to tell from the right one.

Hardware departures from the MX definition that the GPU tests found: none (see DESIGN.md, F16F6 precision).
"""
import functools
import zlib

import numpy as np

import conv_exact_ref as R

# ---------------------------------------------------------------------------------------------------------------------
# e3m2
# ---------------------------------------------------------------------------------------------------------------------
GRID = np.array([m / 16.0 for m in range(4)] + [(1.0 + m / 4.0) * 2.0 ** (ex - 3) for ex in range(1, 8) for m in range(4)])
MID = (GRID[:-1] + GRID[1:]) / 2.0      # MID[i] lies between codes i and i + 1
assert len(GRID) == 32 and GRID[31] == 28.0 and (np.diff(GRID) > 0).all()


def e3m2_decode(code):
    code = np.asarray(code).astype(np.int64)
    return np.where(code & 32, -1.0, 1.0) * GRID[code & 31]


def e3m2_quantise(v, rounding="rne", flush=False):
    """(quantised value, 6-bit code) of float64 v: the nearest representable magnitude, ties to the even code, everything
    from the midpoint above 28 upwards to 28.  rounding "trunc" / "away" and flush (subnormal codes become zero) are the
    alternative quantisers."""
    v = np.asarray(v, dtype=np.float64)
    ax = np.abs(v)
    below = np.searchsorted(MID, ax, side="left")      # a tie stays at the lower code
    above = np.searchsorted(MID, ax, side="right")     # a tie goes to the upper code
    if rounding == "rne":
        idx = np.where(below % 2 == 0, below, above)
    elif rounding == "away":
        idx = above
    else:
        assert rounding == "trunc"
        idx = np.searchsorted(GRID, ax, side="right") - 1
    idx = np.minimum(idx, 31)
    if flush:
        idx = np.where(idx < 4, 0, idx)
    code = (idx | (np.signbit(v).astype(np.int64) << 5)).astype(np.uint8)
    return np.copysign(GRID[idx], v), code


# ---------------------------------------------------------------------------------------------------------------------
# alternative quantisers: keyword sets of weight_model / activation_model
# ---------------------------------------------------------------------------------------------------------------------
EXACT = dict(a_round="rne", a_flush=False, a_max="abs", a_shift=0, a_lo_own=False, a_swap=False,
             w_round="rne", w_flush=False, w_shift=0, w_hi_from16=False, w_scale_from16=False, w_swap=False)
ALTERNATIVES = {
    "a truncation": dict(a_round="trunc"),
    "a ties away": dict(a_round="away"),
    "a subnormal codes flushed": dict(a_flush=True),
    "a hi scale from positive values": dict(a_max="pos"),
    "a hi scale from low halves": dict(a_max="low"),
    "a scale one binade up": dict(a_shift=1),
    "a scale one binade down": dict(a_shift=-1),
    "a lo scale from the lo maximum": dict(a_lo_own=True),
    "a halves exchanged": dict(a_swap=True),
    "w truncation": dict(w_round="trunc"),
    "w ties away": dict(w_round="away"),
    "w subnormal codes flushed": dict(w_flush=True),
    "w scale one binade up": dict(w_shift=1),
    "w scale one binade down": dict(w_shift=-1),
    "w hi codes from fp16(v)": dict(w_hi_from16=True),
    "w scale from max |fp16(v)|": dict(w_scale_from16=True),
    "w halves exchanged": dict(w_swap=True),
}


def variant(alt=None):
    q = dict(EXACT)
    if alt is not None:
        q.update(ALTERNATIVES[alt])
    return q


# ---------------------------------------------------------------------------------------------------------------------
# K order and block partition
# ---------------------------------------------------------------------------------------------------------------------
class KBlocks(object):
    """blocks b = 2 st + hh of a segment kh x kw x cin -> cout at precision 2.  Per (block, j = 0..3): slot, group and tap
    the weights come from and `real` (the slot holds a tap of the filter in a group of the segment); a_grp / a_tap: what
    the kernel reads for the activations (padding slots read real pixels).  Per (block, i = 0..31): kidx = tap * cin +
    channel of the K index the element holds, or -1."""


@functools.lru_cache(maxsize=None)
def k_blocks(kh, kw, cin, cout):
    c = R.launch_class(kh, kw, cin, cout, 2)
    assert c["kernel"] == "f6", (kh, kw, cin, cout)
    kb = KBlocks()
    kb.kh, kb.kw, kb.cin, kb.cout = kh, kw, cin, cout
    kb.taps, kb.groups, kb.stages, kb.direct, kb.tp, kb.nt = kh * kw, (cin + 7) // 8, c["stages"], c["direct"], c["tp"], c["nt"]
    kb.nblk = 2 * kb.stages
    b = np.arange(kb.nblk)
    kb.slot = (8 * (b // 2) + (b % 2))[:, None] + 2 * np.arange(4)[None, :]
    if kb.direct:
        kb.grp, kb.tap = kb.slot.copy(), np.zeros_like(kb.slot)
    else:
        kb.grp, kb.tap = kb.slot // kb.tp, kb.slot % kb.tp
    kb.real = (kb.grp < kb.groups) & (kb.tap < kb.taps)
    kb.a_grp = np.minimum(kb.grp, kb.groups - 1)
    kb.a_tap = np.where(kb.real, kb.tap, 0)
    chn = np.repeat(kb.grp, 8, axis=1) * 8 + np.tile(np.arange(8), 4)[None, :]
    ok = np.repeat(kb.real, 8, axis=1) & (chn < cin)
    kb.kidx = np.where(ok, np.repeat(kb.tap, 8, axis=1) * cin + chn, -1)
    kb.k_padded = kb.nblk * 32
    return kb


def _partner(a):
    """per-block quantity [..., nblk] with the two halves of every stage exchanged"""
    s = a.shape
    return a.reshape(s[:-1] + (s[-1] // 2, 2))[..., ::-1].reshape(s)


def _ilogb(m):
    return np.frexp(m)[1].astype(np.int64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
class Model(dict):
    __getattr__ = dict.__getitem__


def weight_model(w, wscale=1.0, cout_scale=None, c_off=0, cin=None, alt=None):
    """w [kh, kw, cin_total, cout] float32 -> per (row of the NT * 32 padded output channels, block): hi16 (fp16 values),
    eh / el (scale exponents), code_hi / code_lo, and hi / q_hi / q_lo (float64: fp16 value, dequantised planes)"""
    q = variant(alt)
    w = np.asarray(w)
    assert w.dtype == np.float32
    kh, kw, cin_total, cout = w.shape
    cin = cin_total - c_off if cin is None else cin
    kb = k_blocks(kh, kw, cin, cout)
    v = w[:, :, c_off:c_off + cin, :] * np.float32(wscale)
    if cout_scale is not None:
        v = v * np.asarray(cout_scale, dtype=np.float32)
    assert v.dtype == np.float32
    flat = np.concatenate([v.reshape(kb.taps * cin, cout), np.zeros((1, cout), np.float32)])
    vb = np.zeros((kb.nt * 32, kb.nblk, 32), np.float32)
    vb[:cout] = flat[kb.kidx].transpose(2, 0, 1)
    hi16 = vb.astype(np.float16)
    hi = hi16.astype(np.float64)
    lo = (vb - hi16.astype(np.float32)).astype(np.float64)        # exact in fp32
    v64 = vb.astype(np.float64)

    def scale_exp(t):
        m = np.abs(t).max(axis=-1)
        e = np.where(m > 0, _ilogb(np.where(m > 0, m, 1.0)) - 3 + q["w_shift"], 0)
        e = np.clip(e, -126, 120)
        return _partner(e) if q["w_swap"] else e

    eh = scale_exp(hi if q["w_scale_from16"] else v64)
    el = scale_exp(lo)
    src = hi if q["w_hi_from16"] else v64
    qh, ch = e3m2_quantise(src * 2.0 ** -eh[..., None], q["w_round"], q["w_flush"])
    ql, cl = e3m2_quantise(lo * 2.0 ** -el[..., None], q["w_round"], q["w_flush"])
    return Model(kb=kb, cout=cout, hi16=hi16, hi=hi, v=v64, lo=lo, eh=eh, el=el, code_hi=ch, code_lo=cl,
                 q_hi=qh * 2.0 ** eh[..., None], q_lo=ql * 2.0 ** el[..., None])


def decode_pack_image(image, kh, kw, cin, cout):
    """the byte image of mpg_conv_pack_weights(prec = 2) -> hi16, eh, el, code_hi, code_lo as in weight_model, plus
    `scale_bytes` [plane, row, block, 4] (the scale word as stored in each plane) and `spare` (bytes 12-15 of half 1).
    Layout per stage: [4 k-steps][NT][64 lanes][8 fp16] | w_hi6 [NT][2 halves][64 lanes][16 B] | w_lo6 the same; lane
    (row r, half hh) = output channel nt * 32 + r, block (stage, hh); a plane keeps the lane's 32 codes, value i at bits
    6 i .. 6 i + 5 of the 24 bytes (16 of half 0, the first 8 of half 1); bytes 8-11 of half 1 are the scale word."""
    kb = k_blocks(kh, kw, cin, cout)
    nt, ns = kb.nt, kb.stages
    image = np.asarray(image, dtype=np.uint8)
    assert image.size == ns * 8 * nt * 1024, (image.size, ns, nt)
    st = image.reshape(ns, 8 * nt * 1024)
    f16 = st[:, :4 * nt * 1024].copy().view(np.float16).reshape(ns, 4, nt, 2, 32, 8)       # [st, j, nt, hh, r, e]
    hi16 = f16.transpose(2, 4, 0, 3, 1, 5).reshape(nt * 32, ns * 2, 32)
    pl = st[:, 4 * nt * 1024:].reshape(ns, 2, nt, 2, 2, 32, 16)                           # [st, plane, nt, half, hh, r, byte]
    pl = pl.transpose(1, 2, 5, 0, 4, 3, 6).reshape(2, nt * 32, ns * 2, 32)                # [plane, row, block, half * 16 + byte]
    bits = np.unpackbits(np.ascontiguousarray(pl[..., :24]), axis=-1, bitorder="little")
    codes = (bits.reshape(bits.shape[:-1] + (32, 6)) * (1 << np.arange(6))).sum(axis=-1).astype(np.uint8)
    sb = pl[..., 24:28]
    return Model(kb=kb, hi16=hi16, code_hi=codes[0], code_lo=codes[1], scale_bytes=sb, spare=pl[..., 28:32],
                 eh=sb[0, ..., 0].astype(np.int64) - 127, el=sb[0, ..., 1].astype(np.int64) - 127)


# ---------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------
def activation_model(hi, lo, kb, pad_hi=0, g_off=0, alt=None):
    """fp16 planes hi, lo [n, groups, h, w, 8] (as stored; stride 1, no upsampling) -> per (n, y, x, block): e, and per
    element a_hi, q_hi, q_lo (float64) and code_hi / code_lo"""
    q = variant(alt)
    hi, lo = np.asarray(hi), np.asarray(lo)
    assert hi.dtype == np.float16 and lo.dtype == np.float16 and hi.shape == lo.shape
    n, _, h, w, _ = hi.shape
    pt, pl = R.pad_before(kb.kh, pad_hi), R.pad_before(kb.kw, pad_hi)

    def gather(p):
        pp = np.zeros((n, kb.groups, h + kb.kh - 1, w + kb.kw - 1, 8), np.float16)
        pp[:, :, pt:pt + h, pl:pl + w] = p[:, g_off:g_off + kb.groups]
        out = np.zeros((n, h, w, kb.nblk, 32), np.float16)
        for b in range(kb.nblk):
            for j in range(4):
                dy, dx = divmod(int(kb.a_tap[b, j]), kb.kw)
                out[:, :, :, b, 8 * j:8 * j + 8] = pp[:, int(kb.a_grp[b, j]), dy:dy + h, dx:dx + w]
        return out

    ah16, al16 = gather(hi), gather(lo)

    def biased_exp(t16, which):
        mag = (t16.view(np.uint16) & 0x7fff).astype(np.int64)
        if which == "pos":
            mag = np.where(t16.view(np.uint16) & 0x8000, 0, mag)
        elif which == "low":
            mag = mag[..., 0::2]
        return mag.max(axis=-1) >> 10

    e = biased_exp(ah16, q["a_max"]) + q["a_shift"]
    e_lo = biased_exp(al16, "abs") + 12 if q["a_lo_own"] else e
    if q["a_swap"]:
        e, e_lo = _partner(e), _partner(e_lo)
    a_hi, a_lo = ah16.astype(np.float64), al16.astype(np.float64)
    qh, ch = e3m2_quantise(a_hi * 2.0 ** (18 - e)[..., None], q["a_round"], q["a_flush"])
    ql, cl = e3m2_quantise(a_lo * 2.0 ** (30 - e_lo)[..., None], q["a_round"], q["a_flush"])
    return Model(kb=kb, e=e, a_hi16=ah16, a_lo16=al16, a_hi=a_hi, a_lo=a_lo, code_hi=ch, code_lo=cl,
                 q_hi=qh * 2.0 ** (e - 18)[..., None], q_lo=ql * 2.0 ** (e_lo - 30)[..., None])


def expected64(am, wm):
    """(sum a_hi w_hi, sum q(a_lo) q(w), sum q(a_hi) q(w_lo)) [n, h, w, cout] in float64, for one segment"""
    kb = am.kb
    valid = (kb.kidx >= 0).reshape(-1)
    sh = am.a_hi.shape[:3]

    def dot(a, b):
        a2 = a.reshape(-1, kb.nblk * 32)[:, valid]
        b2 = b[:wm.cout].reshape(wm.cout, kb.nblk * 32)[:, valid]
        return (a2 @ b2.T).reshape(sh + (wm.cout,))

    return dot(am.a_hi, wm.hi), dot(am.q_lo, wm.q_hi), dot(am.q_hi, wm.q_lo)


def sum_abs_terms(am, wm):
    """sum over K of |term| of the three sums, [n, h, w, cout]"""
    a = Model(am, a_hi=np.abs(am.a_hi), q_lo=np.abs(am.q_lo), q_hi=np.abs(am.q_hi))
    b = Model(wm, hi=np.abs(wm.hi), q_hi=np.abs(wm.q_hi), q_lo=np.abs(wm.q_lo))
    return sum(expected64(a, b))


def to_f32(e64):
    """float32 of an expectation; + 0.0: the accumulators start at +0, so a zero result is +0"""
    return (np.asarray(e64, dtype=np.float64) + 0.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# data: values with ~20 significant bits, built as fp16 hi + lo with |lo| <= half an ulp of hi
# ---------------------------------------------------------------------------------------------------------------------
TIE_CODES = MID[MID < 16.0]                # midpoints between neighbouring codes, every binade, 0 <-> 1/16 included
A_STYLES = ("general", "negative", "maxneg", "zeros", "ties", "top29", "top30", "bottom0", "bottom1", "general")


def _general(rng, shape, ex, fmax=10, sign=None, lo_bits=8):
    """hi = s m 2^(ex - f) with an 11-bit m in [1, 2) and a per-element f in 0..fmax; lo = r 2^-lo_bits half ulps of hi,
    |r| < 2^lo_bits"""
    m = (1024 + rng.integers(0, 1024, size=shape)) / 1024.0
    f = rng.integers(0, fmax + 1, size=shape)
    s = rng.choice([-1.0, 1.0], size=shape) if sign is None else sign
    hi = s * m * 2.0 ** (ex - f)
    r = rng.integers(-(1 << lo_bits) + 1, 1 << lo_bits, size=shape)
    lo = r * 2.0 ** (ex - f - 11 - lo_bits)
    return hi, lo


def _ties(rng, shape, ex):
    """values on the midpoints between e3m2 codes under the scale 2^(ex - 3) (hi) and 2^(ex - 15) (lo); a quarter of the
    elements are integers 8..15 times the scale, so that (nearly) every block has its maximum in that binade"""
    hc = rng.choice(TIE_CODES, size=shape)
    setter = rng.random(size=shape) < 0.25
    hc = np.where(setter, rng.integers(8, 16, size=shape), hc)
    k = np.floor(np.log2(hc))
    lc = rng.choice(TIE_CODES, size=shape)
    lc = np.where(lc < 2.0 ** (k + 1), lc, np.where(k >= -2, 1.125 * 2.0 ** k, 1.0 / 32))       # within half an ulp of hi
    hi = rng.choice([-1.0, 1.0], size=shape) * hc * 2.0 ** (ex - 3)
    lo = rng.choice([-1.0, 1.0], size=shape) * lc * 2.0 ** (ex - 15)
    return hi, lo


def _act_style(rng, style, shape):
    if style == "general":
        return _general(rng, shape, int(rng.integers(-4, 11)))
    if style == "negative":
        return _general(rng, shape, int(rng.integers(-4, 11)), sign=-1.0)
    if style == "maxneg":       # positive values at least two binades below the negative ones
        ex = int(rng.integers(-4, 11))
        hp, lp = _general(rng, shape, ex - 2, fmax=8, sign=1.0)
        hn, ln = _general(rng, shape, ex, fmax=1, sign=-1.0)
        neg = rng.random(size=shape) < 0.3
        return np.where(neg, hn, hp), np.where(neg, ln, lp)
    if style == "zeros":
        return np.zeros(shape), np.zeros(shape)
    if style == "ties":
        return _ties(rng, shape, int(rng.integers(-4, 11)))
    if style in ("top29", "top30"):
        return _general(rng, shape, 14 if style == "top29" else 15)
    # fp16 subnormal hi (exponent field 0), or a few values of the first normal binade among them (field 1); lo is 0
    m = rng.integers(-1023, 1024, size=shape)
    if style == "bottom1":
        m = np.where(rng.random(size=shape) < 0.2, rng.choice([-1, 1], size=shape) * rng.integers(1024, 2048, size=shape), m)
    return m * 2.0 ** -24, np.zeros(shape)


def _to16(hi, lo):
    h16, l16 = hi.astype(np.float16), lo.astype(np.float16)
    assert np.array_equal(h16.astype(np.float64), hi)          # hi is an fp16 number by construction; lo may be rounded
    return h16, l16


def make_activations(rng, n, cin, h, w, per_pixel):
    """fp16 planes hi, lo [n, groups, h, w, 8]; one style per 4 x 8 pixel region (per pixel when a block holds one pixel,
    the direct 1x1 path), the styles taken in turn; channels beyond cin are zero"""
    cg = (cin + 7) // 8
    hi = np.zeros((n, cg, h, w, 8))
    lo = np.zeros((n, cg, h, w, 8))
    rh, rw = (1, 1) if per_pixel else (4, 8)
    k = int(rng.integers(0, len(A_STYLES)))
    for b in range(n):
        for y0 in range(0, h, rh):
            for x0 in range(0, w, rw):
                sl = (b, slice(None), slice(y0, y0 + rh), slice(x0, x0 + rw))
                hi[sl], lo[sl] = _act_style(rng, A_STYLES[k % len(A_STYLES)], hi[sl].shape)
                k += 1
    dead = (np.arange(cg)[:, None] * 8 + np.arange(8)[None, :] >= cin)[None, :, None, None, :]
    return _to16(np.where(dead, 0.0, hi), np.where(dead, 0.0, lo))


W_STYLES = ("general", "negative", "maxneg", "zeros", "ties_hi", "ties_lo", "topbin", "huge", "general", "tiny")


def _weight_style(rng, style, shape):
    """v float64 (an fp32 number) for blocks [..., 32]"""
    if style in ("general", "negative"):
        hi, lo = _general(rng, shape, int(rng.integers(-10, 7)), fmax=10, sign=-1.0 if style == "negative" else None)
        return hi + lo
    if style == "maxneg":
        ex = int(rng.integers(-8, 7))
        hp, lp = _general(rng, shape, ex - 2, fmax=6, sign=1.0)
        hn, ln = _general(rng, shape, ex, fmax=1, sign=-1.0)
        neg = rng.random(size=shape) < 0.3
        return np.where(neg, hn + ln, hp + lp)
    if style == "zeros":
        return np.zeros(shape)
    if style == "ties_hi":      # v on the midpoints of plane 0; lo = 0
        hi, _ = _ties(rng, shape, int(rng.integers(-8, 7)))
        return hi
    if style == "ties_lo":      # hi in one binade, lo on the midpoints of plane 1 (scale 2^-15 of the binade)
        ex = int(rng.integers(-6, 7))
        hi, _ = _general(rng, shape, ex, fmax=0)
        lc = rng.choice(TIE_CODES, size=shape)
        lc = np.where(rng.random(size=shape) < 0.25, rng.integers(8, 16, size=shape), lc)
        return hi + rng.choice([-1.0, 1.0], size=shape) * lc * 2.0 ** (ex - 15)
    if style == "topbin":       # block maximum in [15.5, 16) * scale, some of them so close to 16 that fp16(v) is 16 * scale
        ex = int(rng.integers(-8, 7))
        hi, lo = _general(rng, shape, ex, fmax=8)
        top = (15.5 + rng.integers(0, 2048, size=shape) / 4096.0) * 2.0 ** (ex - 3)
        top = np.where(rng.random(size=shape) < 0.5, (16.0 - rng.integers(1, 16, size=shape) / 4096.0) * 2.0 ** (ex - 3), top)
        pick = rng.random(size=shape) < 0.1
        pick[..., int(rng.integers(0, 32))] = True
        return np.where(pick, rng.choice([-1.0, 1.0], size=shape) * top, hi + lo)
    if style == "huge":         # up to 6e4
        m = (1024 + rng.integers(0, 850, size=shape)) / 1024.0
        f = rng.integers(0, 9, size=shape)
        return rng.choice([-1.0, 1.0], size=shape) * m * 2.0 ** (15 - f) + rng.integers(-255, 256, size=shape) * 2.0 ** (15 - f - 19)
    assert style == "tiny"      # the exponent clamp: ilogb - 3 < -126
    m = (1024 + rng.integers(0, 1024, size=shape)) / 1024.0
    return rng.choice([-1.0, 1.0], size=shape) * m * 2.0 ** rng.choice([-125.0, -124.0], size=shape)


def make_weights(rng, kh, kw, cin_total, cout, c_off=0, cin=None, tiny=True):
    """w [kh, kw, cin_total, cout] float32 whose window [c_off, c_off + cin) has one style per (output channel, block), the
    styles taken in turn; channels outside the window hold general values.  tiny = False leaves out the magnitudes near
    2^-125, whose products with an activation's lo part lie below the fp32 normal range."""
    cin = cin_total - c_off if cin is None else cin
    kb = k_blocks(kh, kw, cin, cout)
    styles = W_STYLES if tiny else W_STYLES[:-1]
    hi, lo = _general(rng, (kb.taps, cin_total, cout), 0, fmax=8)
    w = hi + lo
    vb = np.zeros((cout, kb.nblk, 32))
    k = int(rng.integers(0, len(styles)))
    for co in range(cout):
        for b in range(kb.nblk):
            vb[co, b] = _weight_style(rng, styles[k % len(styles)], (32,))
            # (one more at the end of a row whose length is a multiple of the style count: a block does not get the same
            # style in every output channel)
            k += 1 + (b == kb.nblk - 1 and kb.nblk % len(styles) == 0)
    ok = kb.kidx >= 0
    tap, chn = kb.kidx[ok] // cin, kb.kidx[ok] % cin
    w[tap, c_off + chn, :] = vb[:, ok].T
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w)
    return w32.reshape(kh, kw, cin_total, cout)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
SIZES = ((16, 32), (17, 33))


class QCase(object):
    def __init__(self, cout, segs, n=1):
        self.cout, self.segs, self.n = cout, tuple(segs), n
        self.name = " + ".join("%dx%dx%d" % s for s in segs) + "->%d" % cout
        self.k_seg = [kh * kw * cin for kh, kw, cin in segs]
        self.k = sum(self.k_seg)

    def __repr__(self):
        return self.name

    def kb(self, s):
        return k_blocks(*self.segs[s], self.cout)

    def seed(self, *more):
        return zlib.crc32(repr((self.name,) + more).encode())

    def locate(self, k):
        """global K index -> (segment, dy, dx, channel)"""
        for s, (kh, kw, cin) in enumerate(self.segs):
            if k < self.k_seg[s]:
                return s, k // cin // kw, k // cin % kw, k % cin
            k -= self.k_seg[s]
        raise IndexError(k)


# (a) pack image: (kh, kw, cin_total, c_off, cin, cout, wscale, cout_scale?)
PACK_SHAPES = [
    (3, 3, 40, 8, 24, 40, 1.0, False),        # tp 12, blocks across groups, ragged cout tile
    (5, 5, 16, 8, 8, 128, 1.0, False),
    (2, 2, 32, 8, 24, 16, 1.0, False),        # tp 8
    (1, 1, 80, 8, 68, 40, 1.0, False),        # direct, 9 groups, 4 channels in the last
    (4, 4, 32, 16, 16, 65, 1.0, False),
    (3, 3, 40, 8, 24, 40, 0.3, True),         # fp32 products with wscale and a cout_scale
    (3, 3, 32, 5, 20, 40, 1.0, False),        # a channel tail in the image form, a window at an odd offset
]


def pack_case(shape):
    kh, kw, cin_total, c_off, cin, cout, wscale, cs = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    w = make_weights(rng, kh, kw, cin_total, cout, c_off, cin)
    scale = (0.5 + rng.random(cout)).astype(np.float32) if cs else None
    return w, scale


# (b) activation codes through one-hot weights: every conversion site and cout tiling
B_CASES = [
    QCase(16, [(3, 3, 8)]),             # image loop, nt 1 (the 128-register kernel)
    QCase(40, [(3, 3, 24)]),            # nt 2, pref 0
    QCase(96, [(5, 5, 16)]),            # nt 3
    QCase(128, [(2, 2, 24)]),           # nt 4, tp 8
    QCase(40, [(1, 1, 64)]),            # direct loop, two tile rows at a time
    QCase(64, [(1, 1, 68)]),            # 9 groups, 4 channels in the last
    QCase(16, [(1, 1, 200)]),           # direct loop of the one-cout-tile kernel
    QCase(16, [(5, 5, 16), (1, 1, 16)]),
    QCase(16, [(3, 3, 20)]),            # a channel tail in the image loop (the issue's shapes have one in the direct loop only)
]
# (c) weight codes through impulse activations: one direct and one image shape per cout tiling
C_CASES = [B_CASES[0], B_CASES[6], B_CASES[1], B_CASES[4], B_CASES[2], B_CASES[3], B_CASES[8]]
# (d) dense general data
D_CASES = [QCase(40, [(3, 3, 24)]), QCase(128, [(5, 5, 16)])]


@functools.lru_cache(maxsize=None)
def b_activations(case, size):
    """per segment the fp16 planes (hi, lo) of the general activations of (b) and (d)"""
    rng = np.random.default_rng(case.seed("act", size))
    return tuple(make_activations(rng, case.n, cin, size[0], size[1], per_pixel=bool(case.kb(s).direct))
                 for s, (kh, kw, cin) in enumerate(case.segs))


@functools.lru_cache(maxsize=6)
def b_act_model(case, size, alt=None):
    return tuple(activation_model(hi, lo, case.kb(s), alt=alt) for s, (hi, lo) in enumerate(b_activations(case, size)))


def b_launches(case):
    return (case.k + case.cout - 1) // case.cout


def b_weights(case, launch, second):
    """one-hot weights of launch `launch`: output channel co holds s 2^j (second: times 1 + 2^-12) at K index
    (launch * cout + co) % K; per segment w [kh, kw, cin, cout] float32"""
    rng = np.random.default_rng(case.seed("onehot", launch))
    j = rng.integers(-12, 13, size=case.cout)
    s = rng.choice([-1.0, 1.0], size=case.cout)
    ws = [np.zeros((kh, kw, cin, case.cout), np.float32) for kh, kw, cin in case.segs]
    for co in range(case.cout):
        seg, dy, dx, c = case.locate((launch * case.cout + co) % case.k)
        ws[seg][dy, dx, c, co] = s[co] * 2.0 ** j[co] * ((1 + 2.0 ** -12) if second else 1.0)
    return ws


def terms(ams, wms):
    """the (up to three per segment) float64 sums of a launch, as a list of arrays [n, h, w, cout]"""
    return [t for am, wm in zip(ams, wms) for t in expected64(am, wm)]


def b_terms(case, size, launch, second, alt=None):
    ws = b_weights(case, launch, second)
    return terms(b_act_model(case, size, alt), [weight_model(w, alt=alt) for w in ws])


# (c)
@functools.lru_cache(maxsize=None)
def c_weights(case):
    rng = np.random.default_rng(case.seed("weights"))
    return tuple(make_weights(rng, kh, kw, cin, case.cout, tiny=False) for kh, kw, cin in case.segs)


@functools.lru_cache(maxsize=64)
def c_weight_model(case, alt=None):
    return tuple(weight_model(w, alt=alt) for w in c_weights(case))


def c_launches(case, size):
    """impulses sit on a grid a filter apart; a launch holds one impulse per grid point, each in its own channel"""
    kh, kw, cin = case.segs[0]
    per = len(range(kh // 2, size[0], kh)) * len(range(kw // 2, size[1], kw))
    return (cin + per - 1) // per


def c_activations(case, size, launch, second):
    """fp16 planes (hi, lo) [n, groups, h, w, 8] of launch `launch`: zero but for impulses of 1.0 (second: 1 + 2^-12, i.e.
    lo = 2^-12), the i-th grid point in channel (launch * points + i) % cin"""
    assert len(case.segs) == 1
    kh, kw, cin = case.segs[0]
    hi = np.zeros((case.n, (cin + 7) // 8, size[0], size[1], 8), np.float16)
    lo = np.zeros_like(hi)
    i = launch * len(range(kh // 2, size[0], kh)) * len(range(kw // 2, size[1], kw))
    for y in range(kh // 2, size[0], kh):
        for x in range(kw // 2, size[1], kw):
            c = i % cin
            hi[:, c // 8, y, x, c % 8] = 1.0
            lo[:, c // 8, y, x, c % 8] = 2.0 ** -12 if second else 0.0
            i += 1
    return hi, lo


def c_terms(case, size, launch, second, alt=None):
    hi, lo = c_activations(case, size, launch, second)
    return terms([activation_model(hi, lo, case.kb(0), alt=alt)], c_weight_model(case, alt))


# (d)
@functools.lru_cache(maxsize=None)
def d_weights(case):
    rng = np.random.default_rng(case.seed("dense weights"))
    return tuple(make_weights(rng, kh, kw, cin, case.cout, tiny=False) for kh, kw, cin in case.segs)


D_SIZE = (17, 33)


def d_expected(case, alt=None):
    """(float64 expectation, derived bound) of the dense case.  |fl(sum) - sum| <= ((1 + u)^(m - 1) - 1) sum |terms| for m
    terms added in fp32 in any order and grouping, each addition rounded or chopped (u = 2^-23); the kernel adds, per
    output, 3 K_padded products into one accumulator (the fp16 products are exact, the bf6 ones exact multiples of their
    block scales), and (1 + u)^(3 K_padded) - 1 <= (3 K_padded + 1) u for 3 K_padded u < 2^-9."""
    ams = b_act_model(case, D_SIZE, alt)
    wms = [weight_model(w, alt=alt) for w in d_weights(case)]
    e = sum(terms(ams, wms))
    kp = sum(am.kb.k_padded for am in ams)
    bound = (3 * kp + 1) * 2.0 ** -23 * sum(sum_abs_terms(am, wm) for am, wm in zip(ams, wms))
    return e, bound


# ---------------------------------------------------------------------------------------------------------------------
# which alternatives each test must be able to see (enforced by test_conv_f6_quant_host.py)
# ---------------------------------------------------------------------------------------------------------------------
A_ALTS = tuple(a for a in ALTERNATIVES if a.startswith("a "))
W_ALTS = tuple(a for a in ALTERNATIVES if a.startswith("w "))
