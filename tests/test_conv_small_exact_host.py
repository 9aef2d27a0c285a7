"""The data of the bit-exact small-channel suite (conv_small_exact_ref.py) has the properties test_conv_small_exact_gpu.py
relies on, for every case: the fp16 split is the intended one, every product is a multiple of 2^-13 and the sum of
|term| of every single output stays below 2^11 (so every fp32 partial sum is exact), the float64 expectation survives
float32 and the G8 planes, and the case CAN fail: without the lo part of its fine side, or read from a neighbouring
channel group, the expectation is another one in every tile.  The case lists cover both dispatch tables, every form of
the column sums and every shape of the weight reads; the LDS arithmetic of the pair launch is restated and held.  No GPU."""
import math

import numpy as np
import pytest

import conv_small_exact_ref as R


def _tiles_hit(diff):
    """does every 16 x 64 tile of every image hold a difference?"""
    n, h, w, _ = diff.shape
    return all(diff[b, y:y + R.TH, x:x + R.TW].any() for b in range(n) for y in range(0, h, R.TH) for x in range(0, w, R.TW))


def _sensitive(true, other, what):
    diff = true != other
    assert diff.mean() > 0.5, (what, float(diff.mean()))
    assert _tiles_hit(diff), what


def _check_tensor(t, fine, what):
    """(v, hi, lo) splits as intended: lo-exact with f = 13 where `fine`, else ternary"""
    v, hi, lo = t
    assert v.dtype == np.float32
    h2, l2 = R.split16(v)
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo), what
    assert np.array_equal(v.astype(np.float64), hi + lo), what
    if fine:
        assert np.array_equal(np.abs(hi), np.ones_like(hi)) and (lo * hi >= 0).all(), what
        assert np.isin(np.abs(lo) * 2.0 ** R.FRAC, [0, 1, 2, 3]).all() and lo.any(), what
    else:
        assert not lo.any() and np.isin(hi, [-1, 0, 1]).all() and hi.any(), what


def _check_packing(p, t, fine, what):
    """the tensor handed to the packer gives the effective filter back exactly; a fine filter goes through wscale, a
    cout_scale and a channel window with foreign channels on both sides"""
    cin = t[0].shape[2]
    assert p.raw.dtype == np.float32 and np.array_equal(p.effective(cin), t[1] + t[2]), what
    if fine:
        assert p.wscale == 2.0 ** -4 and p.c_off >= 1 and p.raw.shape[2] > p.c_off + cin, what
        assert np.isin(p.cout_scale, [0.25, 0.5, 1.0, 2.0, 4.0]).all(), what
        foreign = np.delete(p.raw, np.s_[p.c_off:p.c_off + cin], axis=2)
        assert np.isfinite(foreign).all() and (foreign != 0).all(), what
    else:
        assert p.wscale == 1.0 and p.cout_scale is None and p.c_off == 0 and p.raw.shape[2] == cin, what


def _check_expectation(e64, abs_sum, what):
    bits = R.FRAC + math.log2(float(abs_sum.max()))
    print("%s: sum of |term| up to %.1f: %.1f bits" % (what, float(abs_sum.max()), bits))
    assert abs_sum.max() < R.BOUND, (what, float(abs_sum.max()))              # per output, not a worst-case formula
    assert np.array_equal(e64 * 2.0 ** R.FRAC, np.round(e64 * 2.0 ** R.FRAC)), what
    assert (np.abs(e64) <= abs_sum).all(), what
    e32 = e64.astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), e64), what
    assert np.array_equal(R.g8_roundtrip(e32), e32), what              # the G8 planes keep every bit
    assert e32.any()


@pytest.mark.parametrize("case", R.SINGLE_CASES, ids=repr)
def test_single_case_data_is_exact_and_can_fail(case):
    d = R.case_data(case)
    assert 1 <= len(case.segs) <= 4
    for name, t in d.src.items():
        _check_tensor(t, case.kind == "x", (case, name))
    for s, w, p in zip(case.segs, d.w, d.pack):
        _check_tensor(w, case.kind == "w", (case, s))
        _check_packing(p, w, case.kind == "w", (case, s))
        # one side is coarse: every product is a multiple of 2^-13
        assert R.grid_bits(d.src[d.names[case.segs.index(s)]][0]) + R.grid_bits(w[0]) <= R.FRAC
    if case.bias:
        assert np.array_equal(d.bias * 4, np.round(d.bias * 4)) and d.bias.shape == (case.cout,)
    true = d.expected64()
    _check_expectation(true, d.abs_sum(), case.name)
    if case.act == "relu":          # the clamp has something to do, and leaves most outputs alone
        assert 0.01 < (d.sums() + d.bias <= 0).mean() < 0.4, case
    # the case can fail: the fine side rounded to its hi part
    _sensitive(true, d.expected64(hi_only=True), (case, "hi only"))
    # ... and every window read from a neighbouring group, one segment at a time
    for i, s in enumerate(case.segs):
        if s.window:
            _sensitive(true, d.expected64(goff=lambda j: d.wrong_group(i) if j == i else 0), (case, s, "wrong group"))
            foreign = np.delete(d.src[d.names[i]][0], np.s_[s.c_off:s.c_off + s.cin], axis=3)
            assert np.isfinite(foreign).all() and (foreign != 0).all()


@pytest.mark.parametrize("case", R.AMAX_CASES, ids=repr)
@pytest.mark.parametrize("e", R.AMAX_EXPONENTS)
def test_scaled_data_splits_exactly(case, e):
    """x 2^e is an exact fp32 tensor whose power-of-two scale into [2^8, 2^9) gives the same split, 2^8 times larger; every
    segment's maximum asks for the same scale, and without a bias the expectation times 2^e is an fp32 number"""
    d = R.case_data(case)
    assert d.bias is None
    scales = set()
    for x, xh, xl in d.src.values():
        xs = x * np.float32(2.0 ** e)
        assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) * 2.0 ** e)
        ex = int(np.frexp(np.abs(xs).max())[1])
        scales.add(ex)
        scaled = xs * np.float32(2.0 ** (9 - ex))
        assert 256 <= np.abs(scaled).max() < 512
        hi, lo = R.split16(scaled)
        assert np.array_equal(hi, xh * 2.0 ** 8) and np.array_equal(lo, xl * 2.0 ** 8) and lo.any()
    assert len(scales) == 1
    want = d.expected64() * 2.0 ** e
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and want.any()


@pytest.mark.parametrize("case", R.PAIR_CASES + [R.PAIR_TOO_LARGE], ids=repr)
def test_pair_case_data_is_exact_and_can_fail(case):
    d = R.pair_data(case)
    k = case.kind
    _check_tensor(d.x, k == "x", (case, "x"))
    tensors = [(d.wa, d.pack_a, k == "wa", "A"), (d.wb, d.pack_b, k == "wb", "B")]
    if case.ks is not None:
        tensors.append((d.ws, d.pack_s, k != "x", "shortcut"))
    for t, p, fine, name in tensors:
        if fine:
            _check_tensor(t, True, (case, name))
        else:           # ternary with the case's share of non-zeros
            assert not t[2].any() and np.isin(t[1], [-1, 0, 1]).all() and t[1].any(), (case, name)
            assert np.array_equal(R.split16(t[0])[0], t[1])
        _check_packing(p, t, fine, (case, name))
    for b in (d.bias_a, d.bias_b):
        assert np.array_equal(b * 4, np.round(b * 4))
    # stage A: products on the 2^-13 grid, per-output bound, an fp32 middle
    mid = d.mid()
    assert R.grid_bits(d.x[0]) + R.grid_bits(d.wa[0]) <= R.FRAC
    a_sum = d.abs_sum_a()
    assert a_sum.max() < R.BOUND, (case, float(a_sum.max()))
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid) and (mid <= a_sum).all()
    assert 0.1 < (mid == 0).mean() < 0.9, case                   # relu in the middle clamps, and not everything
    # stage B and the shortcut: the relu'd middle times filter B stays on the grid
    assert R.grid_bits(mid) + R.grid_bits(d.wb[0]) <= R.FRAC, case
    if case.ks is not None:
        assert R.grid_bits(d.x[0]) + R.grid_bits(d.ws[0]) <= R.FRAC
        assert case.ks[0] <= case.ka[0] + case.kb[0] - 1 and case.ks[1] <= case.ka[1] + case.kb[1] - 1
    true = d.expected64()
    print("%s: stage A sum of |term| up to %.1f: %.1f bits" % (case, float(a_sum.max()), R.FRAC + math.log2(float(a_sum.max()))))
    _check_expectation(true, d.abs_sum_b(), case.name + ", stage B")
    if case.act_b == "relu":
        assert 0.01 < (d.pre_b() <= 0).mean() < 0.4, case
    _sensitive(true, d.expected64(hi_only=True), (case, "hi only"))
    if case.seg.window:
        _sensitive(true, d.expected64(goff=d.wrong_group()), (case, "wrong group"))
        foreign = np.delete(d.x[0], np.s_[case.seg.c_off:case.seg.c_off + case.cin], axis=3)
        assert np.isfinite(foreign).all() and (foreign != 0).all()


def test_dispatch_restatement():
    assert [R.chan_bound(c) for c in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    assert R.form(8, 4, 5, 5) == "5x5" and R.form(4, 8, 1, 1) == "1x1" and R.form(8, 8, 5, 5) == "run" == R.form(8, 8, 1, 1)
    assert R.form(1, 1, 5, 1) == "run" == R.form(2, 2, 3, 3)
    assert [R.weight_read(*p) for p in ((1, 1), (2, 1), (1, 4), (4, 4), (8, 4), (8, 8))] == [
        "scalar", "float2", "float4 block", "float4 block", "float4 per channel", "float4 per channel"]
    assert R.kx_unrolled(4, 4, 5, 5) and not R.kx_unrolled(8, 4, 5, 5) and not R.kx_unrolled(1, 1, 3, 3)
    assert R.pair_bounds(1, 1, 1) == (1, 2, 1) and R.pair_bounds(2, 3, 2) == (4, 8, 8) and R.pair_bounds(7, 2, 8) == (8, 2, 8)
    assert sorted({R.pair_bounds(a, b, c) for a in range(1, 9) for b in range(1, 9) for c in range(1, 9)}) == sorted(R.PAIR_INSTANCES)
    # the tile passes: 7 of a single launch, whose last holds 4 of the 1540 pixels of a 7x7 tile
    assert (R.TW + 6) * (R.TH + 6) == 1540 and R.last_pass_pixels(7, 7) == 4 and -(-1540 // 256) == 7
    assert -(-(R.TW + 12) * (R.TH + 12) // 256) == 9


def test_single_cases_cover_the_dispatch():
    names = [c.name for c in R.SINGLE_CASES]
    assert len(set(names)) == len(names)
    allowed_cout, allowed_cin = {1, 2, 3, 4, 5, 8}, {1, 2, 3, 4, 7, 8}
    insts, stages, requested, reach_in, reach_out = set(), set(), set(), {}, {}
    for c in R.SINGLE_CASES:
        assert c.cout in allowed_cout and all(s.cin in allowed_cin for s in c.segs), c
        assert (c.n, c.h <= 32, c.w <= 80) == (2, True, True), c
        cob, cib, segs = c.labels()
        insts.add((cob, cib))
        reach_out.setdefault((cob, cib), set()).add(c.cout)
        reach_in.setdefault((cob, cib), set()).add(max(s.cin for s in c.segs))
        for s, lab in zip(c.segs, segs):
            stages.add(lab + (c.kind,) if "forms" in c.tags else lab)
            requested.add((lab[0], lab[1], (s.kh, s.kw), lab[2]))
    every = [(co, ci) for co in R.BOUNDS for ci in R.BOUNDS]
    assert insts == set(every) and len(every) == 16
    for co, ci in every:       # the bound reached by a ragged and by a full count, on both sides
        assert reach_out[(co, ci)] >= {co, R.RAGGED_COUT[co]} and reach_in[(co, ci)] >= {ci, R.RAGGED_CIN[ci]}, (co, ci)
    # every (CS, COUT) in all three forms: 5x5 and 1x1 on x-fine data, run-time 3x3 on w-fine data
    need = set()
    for cs in R.BOUNDS:
        for co in R.BOUNDS:
            nw, unroll = R.weight_read(cs, co), cs * co <= 16
            if cs * co < 64:
                need |= {(cs, co, "5x5", nw, unroll, "x"), (cs, co, "1x1", nw, unroll, "x")}
            need.add((cs, co, "run", nw, False, "w"))
    form_stages = {s for s in stages if len(s) == 6}
    assert form_stages >= need, sorted(need - form_stages)
    assert {s[:5] for s in form_stages} == {s[:5] for s in need}            # and nothing the enumeration does not know
    assert len(need) == 15 * 2 + 16
    assert {(8, 8, (5, 5), "run"), (8, 8, (1, 1), "run"), (8, 8, (3, 3), "run")} <= requested
    assert {s[3] for s in form_stages} == {"scalar", "float2", "float4 block", "float4 per channel"}
    assert {(s[3], s[2] == "run") for s in form_stages} == {(r, f) for r in ("scalar", "float2", "float4 block", "float4 per channel")
                                                            for f in (False, True)}
    # run-time sizes at float4-per-channel weight reads
    sizes = {(s.kh, s.kw, s.pad_hi) for c in R.SIZE_CASES for s in c.segs}
    assert sizes == {(7, 7, 0), (1, 7, 0), (7, 1, 0), (2, 2, 0), (2, 2, 1), (4, 4, 0), (4, 4, 1)}
    for c in R.SIZE_CASES:
        assert c.labels()[2][0][2:4] == ("run", "float4 per channel"), c
    assert {c.kind for c in R.SIZE_CASES} == {"x", "w"}
    # the seventh tile pass (4 pixels of a 7x7 tile) carries fine activations in one case, meets fine weights in another
    assert {c.kind for c in R.SIZE_CASES if (c.segs[0].kh, c.segs[0].kw) == (7, 7)} == {"x", "w"}
    # segments below the launch's bound, also behind the barrier of a later segment
    assert [[(s.kh, s.kw, s.cin, s.up_log2) for s in c.segs] for c in R.SEG_CASES] == [
        [(5, 5, 2, 0), (1, 1, 8, 0)], [(3, 3, 1, 0), (5, 5, 4, 1), (1, 1, 2, 4), (1, 7, 8, 0)]]
    assert [c.cout for c in R.SEG_CASES] == [1, 3]
    for c in R.SEG_CASES:
        assert any(R.chan_bound(s.cin) < c.cinb for s in c.segs)
    # upsampled sources with fine data
    ups = {(s.up_log2, s.up_x_only) for c in R.UP_CASES for s in c.segs if c.kind == "x"}
    assert ups >= {(1, 0), (2, 0), (4, 0), (2, 1)}
    # windows
    wins = [(s.cin, s.c_off, s.c_total) for c in R.WINDOW_CASES for s in c.segs if len(c.segs) == 1]
    assert sorted(wins) == [(1, 8, 24), (3, 8, 24), (8, 8, 24)]
    two = [c for c in R.WINDOW_CASES if len(c.segs) == 2]
    assert len(two) == 1 and [(s.c_off, s.c_total, s.src) for s in two[0].segs] == [(0, 24, "t"), (16, 24, "t")]
    assert len(R.case_data(two[0]).src) == 1
    # in_amax
    assert {len(c.segs) for c in R.AMAX_CASES} == {1, 2} and R.AMAX_EXPONENTS == (-30, 10)
    assert {c.act for c in R.SINGLE_CASES} == {None, "relu"} and {c.prec for c in R.SINGLE_CASES} == {2, 3}


def test_pair_cases_cover_the_dispatch():
    names = [c.name for c in R.PAIR_CASES]
    assert len(set(names)) == len(names)
    tagged = lambda t: [c for c in R.PAIR_CASES if t in c.tags]
    # (a) all 12 instantiations in the production forms, with counts that reach each bound
    prod = tagged("production")
    assert sorted(c.inst for c in prod) == sorted(R.PAIR_INSTANCES) and len(R.PAIR_INSTANCES) == 12
    assert all((c.ka, c.kb, c.ks, c.kind) == (R.K5, R.K5, R.K1, "x") for c in prod)
    assert {c.cin for c in prod} == {1, 3, 4, 7, 8} and {c.cmid for c in prod} == {2, 3, 8} and {c.cout for c in prod} == {1, 5, 8}
    assert {c.act_b for c in prod} == {None, "relu"}
    for c in R.PAIR_CASES:
        assert c.cin in (1, 3, 4, 7, 8) and c.act_a == "relu" and (c.n, c.h <= 32, c.w <= 80) == (2, True, True)
    # (b) run-time forms
    run = tagged("runtime")
    assert len({c.inst for c in run}) >= 4 and {c.inst[0] for c in run} == {1, 4, 8}
    assert {(c.ka, c.kb, c.ks) for c in run} >= {(R.K3, R.K7, R.K3), (R.K7, R.K3, None), (R.K1, R.K5, R.K5)}
    assert any(c.ks is not None and c.ks[0] > c.ka[0] for c in run)
    # every form and every weight-read class occurs in some stage of some pair launch
    stages = {lab for c in R.PAIR_CASES for lab in c.labels()[1]}
    assert {s[2] for s in stages} == {"5x5", "1x1", "run"}
    assert {s[3] for s in stages} == {"scalar", "float2", "float4 block", "float4 per channel"}
    assert (8, 8, "run", "float4 per channel", False) in stages
    # the ninth pass of the input tile carries fine activations that stage A uses, few and many, inside the image of the
    # first tile row; no tile needs a tenth pass
    used = sorted(R.pair_tile_pixels(c.ka, c.kb)[1] - 2048 for c in tagged("passes") if c.kind == "x")
    assert used == [24, 80] and R.pair_tile_pixels(R.K5, R.K5) == (72 * 24, 72 * 24)
    for c in tagged("passes"):
        last_row = R.TH + c.kb[0] - 1 + c.ka[0] - 1 - 1            # of the tile, at image row last_row - (pad A + pad B)
        assert last_row - (c.ka[0] // 2 + c.kb[0] // 2) < c.h, c
    assert all(R.pair_tile_pixels(c.ka, c.kb)[0] <= 9 * 256 for c in R.PAIR_CASES + [R.PAIR_TOO_LARGE])
    # (c) w-fine, two instantiations
    assert {c.kind for c in tagged("w-fine")} == {"wa", "wb"} and len({c.inst for c in tagged("w-fine")}) == 2
    # (d) upsampling and windows
    assert {(c.seg.up_log2, c.seg.up_x_only) for c in tagged("up")} == {(2, 0), (2, 1)}
    assert sorted((c.cin, c.seg.c_off, c.seg.c_total) for c in tagged("window")) == [(1, 8, 24), (8, 8, 24)]


def test_pair_lds_budget():
    """the byte count of mpg_conv2d_small_pair, restated: 8 -> 8 -> 8 with 7x5 / 5x7 filters and a 3x3 shortcut fits the
    160 KiB of a CU, 7x7 / 7x7 does not (with or without the shortcut)"""
    assert R.LDS_MAX == 163840
    # by hand for 7x7 / 7x7 / 3x3: middle tile 70 x 22 in 6 groups of 4 rows, input tile 76 x 30
    assert 4 * (76 * 30 * 8 + 70 * (24 + 6) * 8 + 2 * 49 * 64 + 9 * 64) == R.PAIR_TOO_LARGE_BYTES == 167552
    assert R.PAIR_TOO_LARGE.lds_bytes() == R.PAIR_TOO_LARGE_BYTES > R.LDS_MAX and not R.PAIR_TOO_LARGE.fits
    assert R.pair_lds_bytes(8, 8, 8, R.K7, R.K7, None) == 165248 > R.LDS_MAX
    fit = [c for c in R.PAIR_CASES if "lds" in c.tags]
    assert len(fit) == 1 and (fit[0].ka, fit[0].kb, fit[0].ks, fit[0].inst) == ((7, 5), (5, 7), R.K3, (8, 8, 8))
    assert fit[0].lds_bytes() == 4 * (74 * 26 * 8 + 70 * 24 * 8 + 2 * 35 * 64 + 9 * 64) == 135552
    # the production block, 1 -> 2 -> 8 at 5x5 / 5x5 / 1x1: tiles of 72 x 24 and 68 x 24 pixels, tables of 50, 400 and 8 words
    assert R.pair_lds_bytes(1, 2, 8, R.K5, R.K5, R.K1) == 4 * (72 * 24 + 68 * 24 * 2 + 52 + 400 + 8)
    for c in R.PAIR_CASES:
        assert c.fits and c.lds_bytes() <= R.LDS_MAX, c


def test_packed_shapes_exist(mpg):
    """every filter of the lists can be packed at the precision its case names"""
    from mpgan_amd import _lib
    lib = _lib.load()
    for c in R.SINGLE_CASES:
        for s in c.segs:
            assert lib.mpg_conv_pack_size(s.kh, s.kw, s.cin, c.cout, c.prec) > s.kh * s.kw * 64 * 4, (c, s)
    for c in R.PAIR_CASES + [R.PAIR_TOO_LARGE]:
        shapes = [(c.ka, c.cin, c.cmid), (c.kb, c.cmid, c.cout)] + ([(c.ks, c.cin, c.cout)] if c.ks is not None else [])
        for k, ci, co in shapes:
            assert lib.mpg_conv_pack_size(k[0], k[1], ci, co, c.prec) > k[0] * k[1] * 64 * 4, (c, k)
    assert lib.mpg_conv_pack_size(9, 9, 1, 8, 2) == 0 and lib.mpg_conv_pack_size(7, 9, 1, 8, 2) == 0      # no 9x9 table exists
