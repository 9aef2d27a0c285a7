"""What g8_ref.py claims, proven without a GPU: the canonical split and the range over which its 2^-22 holds (the range
include/mpgan.h states), that every data class is in the arrays the GPU test converts, the scale-law table, that the
to_g8 cases reach the kernels they name, and that the expectations of the consumer cases are normal fp32 numbers which
the uncapped scale law cannot deliver."""
import os
import re

import numpy as np
import pytest

import g8_ref as R

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mpgan.h")


def _err(v):
    """|v - (hi + lo)| in float64 of the canonical split"""
    hi, lo = R.split(v)
    return np.abs(np.asarray(v, dtype=np.float64) - (hi.astype(np.float64) + lo.astype(np.float64)))


# ---- the split ----------------------------------------------------------------------------------------------------------
def test_split_is_the_definition():
    """hi is the nearest fp16 (ties to the even one, gradual underflow), the fp32 difference v - hi is exact, and unpack
    returns hi + lo without a rounding of its own"""
    for kind in R.CLASSES:
        v = R.class_vector(kind, 4096, "host")
        hi, lo = R.split(v)
        v64, hi64 = v.astype(np.float64), hi.astype(np.float64)
        # nearest: no fp16 neighbour of hi is closer to v
        bits = hi.view(np.uint16)
        mag = bits & 0x7FFF
        assert (mag < 0x7C00).all()
        up = ((mag + 1).astype(np.uint16) | (bits & 0x8000)).view(np.float16).astype(np.float64)      # inf behind 65504
        dn = ((np.maximum(mag.astype(np.int32) - 1, 0)).astype(np.uint16) | (bits & 0x8000)).view(np.float16).astype(np.float64)
        dn = np.where(mag == 0, -up, dn)                                                               # across zero
        d = np.abs(v64 - hi64)
        assert np.all(d <= np.abs(v64 - up)) and np.all(d <= np.abs(v64 - dn)), kind
        tie = (d > 0) & ((d == np.abs(v64 - up)) | (d == np.abs(v64 - dn)))
        assert np.all(bits[tie] & 1 == 0), "%s: a tie went to the odd neighbour" % kind
        if kind == "ties":
            assert tie.all()
        # the fp32 difference is exact
        r32 = v - hi.astype(F32)
        assert np.array_equal(r32.astype(np.float64), v64 - hi64), kind
        assert np.array_equal(lo.view(np.uint16), r32.astype(np.float16).view(np.uint16))
        # pack / unpack agree with it and add nothing
        img = R.pack(v.reshape(1, 16, 16, 16))
        assert np.array_equal(R.unpack(img, 16).astype(np.float64).ravel(), hi64 + lo.astype(np.float64)), kind


def test_split_accuracy_and_its_range():
    """|v - (hi + lo)| <= 2^-22 |v| holds for 2^-3 <= |v| <= 65504 (65519.9, which still rounds to 65504, included) and
    not below: lo is then an fp16 subnormal (spacing 2^-24) and the bound is the absolute 2^-25.  The classes that are
    built to split exactly do."""
    sweep = np.concatenate([R.class_vector(k, 1 << 16, "accuracy") for k in R.CLASSES]
                           + [(s * 2.0 ** np.random.default_rng(7).uniform(-4.0, 16.0, 1 << 16)).astype(F32) for s in (1.0, -1.0)])
    sweep = sweep[np.abs(sweep) < 65520.0]
    err, a = _err(sweep), np.abs(sweep.astype(np.float64))
    upper = a >= 2.0 ** -3
    assert upper.sum() > 1 << 16 and (~upper).sum() > 1 << 16
    assert np.all(err[upper] <= 2.0 ** -22 * a[upper])
    assert np.all(err <= np.maximum(2.0 ** -25, 2.0 ** -22 * a))
    rel = np.max(err[upper] / a[upper])
    print("split: max relative error over [2^-3, 65504] %.4g = 2^%.2f; max absolute error below 2^-3 %.4g = 2^%.2f"
          % (rel, np.log2(rel), err[~upper].max(), np.log2(err[~upper].max())))
    # just below 2^-3 the relative bound fails: lo = 2^-25 and 3 2^-25 are ties between fp16 subnormals
    for v in (2.0 ** -4 + 2.0 ** -25, 2.0 ** -3 - 2.0 ** -14 + 3 * 2.0 ** -25):
        assert float(F32(v)) == v and v < 2.0 ** -3
        assert _err(F32(v)) == 2.0 ** -25 and 2.0 ** -25 > 2.0 ** -22 * v
    # ties (from 2^-13 on: below, half an fp16 ulp is itself under the smallest fp16) and the ends of the contract split exactly
    t = R.class_vector("ties", 1 << 14, "accuracy")
    assert not _err(t[np.abs(t) >= 2.0 ** -13]).any() and (_err(t[np.abs(t) < 2.0 ** -14]) == 2.0 ** -25).all()
    assert not _err(np.array([R.F16_MAX, -R.F16_MAX, 0.0, -0.0, 2.0 ** -24, 1.0 + 2.0 ** -11, 2049.0], F32)).any()
    # what the header says
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"<= 2\^-22 \|v\| for 2\^-3 <= \|v\| <= 65504", text) and "exact to 2^-22" not in text
    assert "2^-25" in text and "min(9 - e, 126)" in text and "not NaN" in text


def test_edges_of_the_formats():
    hi, lo = R.split(np.array([65519.9, 65520.0, -0.0, 2.0 ** -25, 1.5 * 2.0 ** -25, 1e-40, np.inf, np.nan], F32))
    assert hi[0] == 65504 and hi[1] == np.inf and lo[1] == -np.inf                  # beyond the contract: hi + lo is NaN
    assert hi.view(np.uint16)[2] == 0x8000 and lo.view(np.uint16)[2] == 0          # -0: hi keeps the sign, lo is +0
    assert hi[3] == 0 and lo[3] == 0                                                # 2^-25: the tie goes to zero, twice
    assert hi[4] == 2.0 ** -24 and lo[4] == 0                                       # (the fp32 rest, -2^-26, is below the tie)
    assert hi[5] == 0 and lo[5] == 0
    assert np.isinf(hi[6]) and np.isnan(lo[6]) and np.isnan(hi[7]) and np.isnan(lo[7])


# ---- the data -----------------------------------------------------------------------------------------------------------
def _census(v):
    """counts of what the conversion has to get right in the float32 vector v"""
    v = np.asarray(v, dtype=F32).ravel()
    hi, lo = R.split(v)
    hi64 = hi.astype(np.float64)
    bits = hi.view(np.uint16)
    mag = bits & 0x7FFF
    other = np.where(np.abs(hi64) >= np.abs(v.astype(np.float64)), np.maximum(mag.astype(np.int32) - 1, 0), mag + 1).astype(np.uint16)
    other = (other | (bits & 0x8000)).view(np.float16).astype(np.float64)
    d = np.abs(v.astype(np.float64) - hi64)
    tie = (d > 0) & (d == np.abs(v.astype(np.float64) - other))
    rest = v - hi.astype(F32)
    grew = np.abs(hi64) > np.abs(v.astype(np.float64))          # the odd neighbour was the smaller one: rounded away from zero
    return dict(ties=int(tie.sum()), ties_up=int((tie & grew).sum()), ties_down=int((tie & ~grew).sum()),
                subnormal_hi=int(((mag > 0) & (mag < 0x0400)).sum()), flushed_hi=int(((mag == 0) & (v != 0)).sum()),
                subnormal_lo=int(((lo.view(np.uint16) & 0x7FFF > 0) & (lo.view(np.uint16) & 0x7FFF < 0x0400)).sum()),
                flushed_lo=int(((rest != 0) & (lo == 0)).sum()), neg_zero=int((v.view(np.uint32) == 0x80000000).sum()),
                fp32_subnormal=int(((np.abs(v) > 0) & (np.abs(v) < 2.0 ** -126)).sum()), top=int((np.abs(v) >= R.F16_MAX).sum()))


def test_every_class_is_in_the_arrays():
    """by count, in the channel window the conversion reads: ties of both parities of the surviving neighbour, subnormal and
    flushed hi, subnormal and flushed lo, -0, fp32 subnormals and the top of the range"""
    total = {}
    for case in R.TO_G8_CASES:
        if case.n > 64:
            continue          # the 65536-image tensor has everything many times over; the count would take seconds
        x = R.to_g8_data(case)[..., case.c_off:case.c_off + case.cin]
        cen = _census(x)
        for k, v in cen.items():
            total[k] = total.get(k, 0) + v
        if x.size >= 256:
            assert all(v >= 1 for v in cen.values()), (case, cen)
        else:
            assert cen["ties"] >= 1, (case, cen)
    print("census over the to_g8 cases:", total)
    assert all(v >= 16 for v in total.values()), total
    # the scaled runs keep the classes: a power of two moves ties to ties
    cen = _census(R.scaled_data(R.mixed((4096,), "scaled"), 2.0 ** 24) * F32(2.0 ** 24))
    assert cen["ties"] >= 256 and cen["neg_zero"] >= 1 and cen["subnormal_hi"] >= 16, cen
    # the planes of the g8 -> fp32 test: finite patterns, subnormals and both zeros
    p = R.fp16_patterns((2, 2, 2, 3, 5, 8), "host")
    mag = p & 0x7FFF
    assert (mag < 0x7C00).all() and ((mag > 0) & (mag < 0x0400)).sum() >= 8 and (p == 0).sum() >= 1 and (p == 0x8000).sum() >= 1
    img = R.poison_padding(np.zeros((2, 2, 2, 3, 5, 8), np.uint16), 13)
    assert np.isnan(img.view(np.float16)[:, -1, :, :, :, 5:]).all() and not img[:, -1, :, :, :, :5].any() and not img[:, 0].any()
    assert not np.isnan(R.unpack(img, 13)).any()


# ---- the scale law --------------------------------------------------------------------------------------------------------
# log2 of the scale, written down by hand: amax = m 2^e, m in [0.5, 1) -> min(9 - e, 126); None: the scale is 1 by rule
SCALE_LOG2 = {"0": None, "-1": None, "2^8": 0, "below 2^9": 0, "2^9": -1, "1": 8, "3e-5": 24, "2^-30": 38, "2^-100": 108,
              "2^-118": 126, "2^-119": 126, "2^-120": 126, "1e-37": 126, "2^-126": 126, "2^-140": 126, "2.9e38": -119,
              "3.0e38": None, "inf": None, "NaN": None}


def test_pow2_scale_table():
    assert [k for k, _ in R.AMAX_TABLE] == list(SCALE_LOG2)
    for name, amax in R.AMAX_TABLE:
        s = R.pow2_scale(amax)
        k = SCALE_LOG2[name]
        assert s.dtype == F32 and float(s) == (1.0 if k is None else 2.0 ** k), (name, s)
        assert R.is_normal_f32(s) and R.is_normal_f32(1.0 / np.float64(s)), name
        old = R.pow2_scale_uncapped(amax)
        if k is None:
            assert old == 1.0
            continue
        bites = 0 < float(amax) < 2.0 ** -118
        assert bites == (float(s) != float(old)), name
        scaled = float(amax) * float(s)
        if bites:
            assert 0 < scaled < 2.0 ** 8, name
        else:
            assert 2.0 ** 8 <= scaled < 2.0 ** 9, (name, scaled)
        # the uncapped law: inf below 2^-119, a subnormal reciprocal at 2^-119
        assert np.isinf(old) == (float(amax) < 2.0 ** -119), name
    assert 1.0 / float(R.pow2_scale_uncapped(F32(2.0 ** -119))) == 2.0 ** -127
    with np.errstate(invalid="ignore"):
        assert np.isnan(F32(0.0) * R.pow2_scale_uncapped(F32(1e-37)))               # what poisoned a training step


def test_absmax_reference():
    assert R.absmax([]) == 0 and R.absmax([np.nan, np.nan]) == 0 and R.absmax([-0.0, 0.0]).view(np.uint32) == 0
    assert R.absmax([1.0, np.nan, -3.0]) == 3 and np.isinf(R.absmax([1.0, -np.inf, np.nan]))
    for n in R.ABSMAX_SIZES:
        for mis in (0, 4):
            pos = R.absmax_positions(n, mis)
            assert all(0 <= i < n for i, _ in pos.values())
            if n >= 1:
                assert {"first", "last", "negative"} <= set(pos)
    assert {"bulk", "tail"} <= set(R.absmax_positions(4099, 0)) and {"bulk", "tail"} <= set(R.absmax_positions(1023, 0))
    assert not {"bulk", "tail"} & set(R.absmax_positions(4099, 4))
    assert "tail" in R.absmax_positions(5, 0)
    assert (R.ABSMAX_BIG + 256 * 16 - 1) // (256 * 16) > 4096                    # the grid cap is reached


# ---- the cases ------------------------------------------------------------------------------------------------------------
def test_to_g8_cases_reach_their_kernels():
    for case in R.TO_G8_CASES:
        assert R.kernel_for(case.n, case.c, case.c_off, case.cin, case.misalign) == case.kernel, case
        assert case.c_off + case.cin <= case.c
    # every predicate of the dispatch is failed alone by one case
    for i, name in enumerate(R.PREDICATES):
        hits = [c for c in R.TO_G8_CASES if c.fails == name]
        assert len(hits) == 1, name
        p = R.predicates(hits[0].n, hits[0].c, hits[0].c_off, hits[0].cin, hits[0].misalign)
        assert [j for j, ok in enumerate(p) if not ok] == [i], (name, p)
    tiled = [(c.n, c.h, c.w, c.c, c.c_off, c.cin) for c in R.TO_G8_CASES if c.kernel == "tiled"]
    assert tiled == R.TILED_SHAPES
    # what the tiled shapes are there for: one pixel; a second pixel block of one pixel; quad tails of 1, 2, 3 channels;
    # a second channel tile of one channel; three channel tiles at an offset; a window in the middle of the row
    assert (2, 3, 11, 36, 4, 32) in tiled and 3 * 11 == 32 + 1 and 129 == 128 + 1 and 260 > 2 * 128
    assert {c.cin for c in R.TO_G8_CASES if "narrow" in c.name} == {17, 1, 3, 8, 9}
    # the other tables
    n, h, w = R.FROM_G8_NHW
    assert all((n * h * w * c) % 256 for c in R.FROM_G8_CHANNELS)
    assert {R.pn_kernel(c) for c in R.PN_CHANNELS} == {4, 8} and R.pn_kernel(256) == 4 and R.pn_kernel(257) == 8
    assert sorted(h * w for h, w in R.PN_HW) == [1, 63, 65]


def test_the_data_tells_planes_and_channels_apart():
    """a conversion that swaps the two planes, or two channels of a group, gives another image on every case's data (for
    mpg_g8_to_f32 the planes commute, hi + lo, so only the channels can be told apart there)"""
    for case in R.TO_G8_CASES:
        if case.n > 64:
            continue
        img = R.pack(R.to_g8_data(case), case.c_off, case.cin)
        assert not np.array_equal(img[:, :, ::-1], img), case
        for a, b in ((0, 1), (3, 4), (6, 7)):
            sw = img.copy()
            sw[..., [a, b]] = img[..., [b, a]]
            assert (a >= case.cin and b >= case.cin) or not np.array_equal(sw, img), (case, a, b)
        if R.groups(case.cin) > 1:
            assert not np.array_equal(img[:, ::-1], img), case
    n, h, w = R.FROM_G8_NHW
    for c in R.FROM_G8_CHANNELS:
        img = R.poison_padding(R.fp16_patterns((n, R.groups(c), 2, h, w, 8), "from_g8 %d" % c), c)
        want = R.unpack(img, c)
        assert np.isfinite(want).all()
        for a, b in ((0, 1), (3, 4), (6, 7)):
            if b < c:
                sw = img.copy()
                sw[..., [a, b]] = img[..., [b, a]]
                assert not np.array_equal(R.unpack(sw, c).view(np.uint32), want.view(np.uint32)), (c, a, b)
        # reading a padding lane shows: it holds a NaN
        assert c % 8 == 0 or np.isnan(R.unpack(img, R.groups(c) * 8)[..., c:]).all()


def test_consumer_expectations_are_normal_fp32_numbers():
    """the fused and the small convolution at 2^-122 and the weight gradient at 2^-55 x 2^-60: every expectation is a normal
    fp32 number, exactly (no exemption list), the data splits as intended under the capped scale, and the uncapped law gives
    inf for each of them"""
    for kind in ("fused", "small"):
        c = R.conv_consumer(kind)
        assert (c.expected64 > 0).all()
        want = c.expected64 * 2.0 ** R.CONSUMER_E
        assert R.is_normal_f32(want) and np.array_equal(want.astype(F32).astype(np.float64), want), kind
        x = c.x * F32(2.0 ** R.CONSUMER_E)
        assert np.array_equal(x.astype(np.float64), c.x.astype(np.float64) * 2.0 ** R.CONSUMER_E)
        amax = R.absmax(x)
        assert np.isinf(R.pow2_scale_uncapped(amax)) and R.pow2_scale(amax) == 2.0 ** 126
        assert not _err(x * R.pow2_scale(amax)).any()                          # hi = 16, lo = l 2^-9
        hi, lo = R.split(x * R.pow2_scale(amax))
        assert (hi == 16).all() and lo.any()
        # fp32 sums of the scaled terms are exact: the sum of |term| stays below 2^24 quanta
        quantum = 2.0 ** -13
        assert c.expected64.max() / quantum < 2.0 ** 24 and np.array_equal(np.round(c.expected64 / quantum), c.expected64 / quantum)
    g = R.wgrad_consumer()
    want = g.expected64 * 2.0 ** (R.WG_EX + R.WG_ED)
    assert (g.expected64 > 0).all() and R.is_normal_f32(want) and np.array_equal(want.astype(F32).astype(np.float64), want)
    sx, sd = R.pow2_scale(R.absmax(g.x * F32(2.0 ** R.WG_EX))), R.pow2_scale(R.absmax(g.d * F32(2.0 ** R.WG_ED)))
    assert (float(sx), float(sd)) == (2.0 ** 63, 2.0 ** 68)
    with np.errstate(over="ignore"):
        assert np.isinf(sx * sd) and F32(R.WG_WSCALE) / (sx * sd) == 0             # the single factor: every gradient 0
    assert g.expected64.max() / (R.WG_WSCALE * 2.0 ** -13) < 2.0 ** 24
