"""The data of the bit-exact fused-convolution suite (conv_exact_ref.py) has the properties test_conv_exact_gpu.py
relies on, for every case of its list: the fp16 split is the intended one, the sum of |term| stays below 2^(24 - f) so
that every fp32 partial sum is exact, the float64 expectation survives float32 (and, where the case reads the G8 output,
the hi16 + lo16 planes), and the launch class each case names is the one the host code chooses -- the restatement of
seg_shape / seg_shape_f6 in conv_exact_ref.launch_class() is held against mpg_conv_pack_size.  No GPU."""
import numpy as np
import pytest

import conv_exact_ref as R
from oracle import ops as O


@pytest.mark.parametrize("case", R.ALL_CASES, ids=repr)
def test_case_data_is_exact(case):
    assert 1 <= len(case.segs) <= R.MAX_SEG
    d = R.case_data(case)
    for s, x, w, ((xh, xl), (wh, wl)) in zip(case.segs, d.x, d.w, d.parts):
        gs = s.group_scale()
        for v, hi, lo, unit in ((x, xh, xl, 1.0 / gs if s.gexp else 1.0), (w, wh, wl, gs[:, None] if s.gexp else 1.0)):
            assert v.dtype == np.float32
            h2, l2 = R.split16(v)
            assert np.array_equal(h2, hi) and np.array_equal(l2, lo), (case, s)
            assert np.array_equal(v.astype(np.float64), hi + lo)
            if case.small:
                assert not lo.any() and np.abs(hi).max() <= 3
            else:
                assert np.array_equal(np.abs(hi), np.ones_like(hi) * unit) and (lo * hi >= 0).all()      # lo has the sign of hi
                assert np.isin(np.abs(lo) / unit * 2.0 ** case.frac, [0, 1, 2, 3] if case.frac == 13 else [0, 1]).all()
    if case.small:
        assert case.k * 9 < 2 ** 24
    else:
        assert R.sum_abs_bound(case.k, case.frac) < 2.0 ** (24 - case.frac), (case.k, case.frac)
    for prec in case.precs:
        e64 = d.expected64(prec)
        assert np.array_equal(e64.astype(np.float32).astype(np.float64), e64), (case, prec)
        assert np.array_equal(e64 * 2.0 ** case.frac, np.round(e64 * 2.0 ** case.frac))
        if case.g8:     # the G8 planes keep every bit of the result
            assert np.array_equal(R.g8_roundtrip(d.expected(prec)), d.expected(prec)), (case, prec)
    if not case.small:
        # lo * lo is not part of the definition: the full product is another number
        full = sum(R.correlate(R.upsample_nearest((xh + xl)[..., s.c_off:s.c_off + s.cin], s.up_log2), wh + wl, s.pad_hi)
                   for s, ((xh, xl), (wh, wl)) in zip(case.segs, d.parts))
        assert not np.array_equal(full, d.expected64(3))
        assert np.abs(full - d.expected64(3)).max() <= case.k * 9 * 4.0 ** -case.frac


@pytest.mark.parametrize("case", R.AMAX_CASES, ids=repr)
@pytest.mark.parametrize("e", R.AMAX_EXPONENTS)
def test_scaled_data_splits_exactly(case, e):
    """x 2^e is an exact fp32 tensor whose power-of-two scale into [2^8, 2^9) gives the same split, 2^8 times larger"""
    d = R.case_data(case)
    for x, ((xh, xl), _) in zip(d.x, d.parts):
        xs = x * np.float32(2.0 ** e)
        assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) * 2.0 ** e)
        m, ex = np.frexp(np.abs(xs).max())
        scaled = xs * np.float32(2.0 ** (9 - int(ex)))
        assert 256 <= np.abs(scaled).max() < 512
        k = 2.0 ** (9 - int(ex) + e)
        hi, lo = R.split16(scaled)
        assert np.array_equal(hi, xh * k) and np.array_equal(lo, xl * k)
    for prec in case.precs:
        want = d.expected64(prec) * 2.0 ** e
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)


def test_reference_correlation():
    """correlate() is a plain zero-padded correlation: TF SAME padding without pad_hi (the oracle's conv2d_same), one more
    zero in front of an even filter with it, nothing changed for an odd one"""
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, size=(2, 7, 9, 3)).astype(np.float64)       # integers: exact in the oracle's float32 too
    for kh, kw in ((3, 3), (4, 4), (2, 3), (1, 7), (6, 6), (5, 1)):
        w = rng.integers(-3, 4, size=(kh, kw, 3, 4)).astype(np.float64)
        a = R.correlate(x, w)
        assert np.array_equal(a, O.conv2d_same(x, w))
        b = R.correlate(x, w, pad_hi=1)
        dy, dx = 1 - kh % 2, 1 - kw % 2        # pad_hi shifts the window of an even axis by one pixel
        assert np.array_equal(b[:, dy:, dx:], a[:, :7 - dy, :9 - dx])
        if dy == 0 and dx == 0:
            assert np.array_equal(a, b)
    # definition at one corner, written out: output (0, 0) of a 2x2 filter with pad_hi sees only x[0, 0] under tap (1, 1)
    w = rng.integers(-3, 4, size=(2, 2, 3, 4)).astype(np.float64)
    assert np.array_equal(R.correlate(x, w, pad_hi=1)[0, 0, 0], x[0, 0, 0] @ w[1, 1])
    assert np.array_equal(R.correlate(x, w)[0, 6, 8], x[0, 6, 8] @ w[0, 0])
    assert np.array_equal(R.upsample_nearest(x, 1)[:, 5, 7], x[:, 2, 3])


def test_launch_class_matches_the_library(mpg):
    """the restated K decomposition gives the packed size the library reports, for every segment shape and precision of
    the case list, and every case is in the class its comment names"""
    from mpgan_amd import _lib
    lib = _lib.load()
    for case in R.ALL_CASES:
        for prec in case.precs:
            for s in case.segs:
                got = lib.mpg_conv_pack_size(s.kh, s.kw, s.cin, case.cout, prec)
                assert got > 0 and got == R.pack_bytes(s.kh, s.kw, s.cin, case.cout, prec), (case, s, prec, got)
            if case.cls_prec in (None, prec):
                s = case.segs[case.cls_seg]
                c = R.launch_class(s.kh, s.kw, s.cin, case.cout, prec)
                if case.small:
                    c["kernel"] = "small"
                assert {k: c[k] for k in case.cls} == case.cls, (case, prec, c)
    # shapes whose size distinguishes the decompositions: two groups per chunk, one group by the LDS limit, every tap
    # padding, the direct path and its neighbours
    for (kh, kw, cin, cout) in ((1, 1, 32, 96), (1, 3, 48, 128), (3, 3, 32, 96), (5, 5, 128, 128), (7, 7, 24, 40), (1, 1, 64, 64),
                                (1, 1, 64, 65), (3, 3, 32, 96), (3, 5, 24, 16), (2, 2, 24, 16), (1, 1, 136, 33)):
        for prec in (1, 2, 3):
            assert lib.mpg_conv_pack_size(kh, kw, cin, cout, prec) == R.pack_bytes(kh, kw, cin, cout, prec), (kh, kw, cin, cout, prec)


def test_case_list_covers_the_launch_classes():
    names = [c.name for c in R.ALL_CASES]
    assert len(set(names)) == len(names)
    assert {s.up_log2 for c in R.SEG_CASES for s in c.segs} >= {0, 1, 4}
    assert {s.c_off for c in R.SEG_CASES for s in c.segs} >= {0, 8, 16}
    assert {s.pad_hi for c in R.SEG_CASES for s in c.segs} == {0, 1}
    assert {len(c.segs) for c in R.SEG_CASES} >= {3, 4}
    assert any(s.gexp for c in R.CASES for s in c.segs)
    seen = set()
    for case in R.CASES + R.SEG_CASES:
        for prec in case.precs:
            parity = "grid%%8=%d" % min(R.blocks(case, prec) % 8, 1)
            for s in case.segs:
                c = R.launch_class(s.kh, s.kw, s.cin, case.cout, prec)
                if case.small:
                    seen.add(("small",))
                    continue
                fam = c["kernel"]
                seen.update({(fam, "nt", c["nt"]), (fam, parity)})
                if fam == "mfma":
                    seen.update({("cgc", c["cgc"]), ("even taps", (s.kh * s.kw) % 2 == 0), ("ring wraps", c["ring_wraps"] > 3),
                                 ("under ring", c["stages"] < 3)})
                elif c["direct"]:
                    seen.update({("direct",), ("direct stages", min(c["stages"], 3)), ("direct ragged group", s.cin % 8 != 0)})
                else:
                    t = s.kh * s.kw
                    seen.update({("tp", "T" if c["tp"] == t else c["tp"], "groups", min(c["nchunks"], 2)), ("pref", c["pref"]),
                                 ("1x1 not direct", t == 1)})
            if 2 in case.precs and len(case.segs) > 1 and case.cout <= 32 and R.blocks(case, 2) > 256:
                seen.add(("seg_flip", "grid%%8=%d" % min(R.blocks(case, 2) % 8, 1)))
    need = {("small",), ("cgc", 1), ("cgc", 2), ("even taps", True), ("ring wraps", True), ("under ring", True), ("direct",),
            ("direct stages", 1), ("direct stages", 2), ("direct stages", 3), ("direct ragged group", True), ("pref", 0), ("pref", 1),
            ("1x1 not direct", True), ("seg_flip", "grid%8=0"), ("seg_flip", "grid%8=1")}
    need |= {(fam, "nt", nt) for fam in ("mfma", "f6") for nt in (1, 2, 3, 4)}
    need |= {(fam, "grid%%8=%d" % p) for fam in ("mfma", "f6") for p in (0, 1)}
    need |= {("tp", tp, "groups", g) for tp in (8, 12, 16, "T") for g in (1, 2)}
    assert need <= seen, sorted(need - seen, key=repr)


def test_mismatch_report_names_the_tile():
    want = np.zeros((2, 19, 40, 40), dtype=np.float32)
    assert R.mismatch_report(want, want.copy(), 16) == ""
    got = want.copy()
    got[1, 17, 35, 33] = 1.0
    got[1, 18, 39, 39] = -0.0          # bit for bit: a sign of zero counts
    msg = R.mismatch_report(got, want, 16, what="probe")
    assert "2 of %d values differ" % want.size in msg and "(1, 17, 35, 33)" in msg
    assert "tile row 1 (row 1 of it), tile column 1 (column 3 of it), cout tile 1 (channel 1 of it)" in msg
    assert "cout tiles hit: [1]" in msg
    assert "shape" in R.mismatch_report(got[:1], want, 16)
    assert [r[0] for r in R.rotations("abc")] == ["a", "b", "c"]
