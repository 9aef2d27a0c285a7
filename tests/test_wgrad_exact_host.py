"""The data of the bit-exact weight-gradient suite (wgrad_exact_ref.py) has the properties test_wgrad_exact_gpu.py relies
on, for every case of its list: the fp16 split of x and of the scaled dy is the intended one (also under the power-of-two
scale of mpg::pow2_scale), the sum of |term| over the pixels stays below 2^(24 - f), the float64 expectation survives
float32 at every exponent, and the launch class each case names is the one the library's planner
(mpg_conv2d_wgrad_plan) chooses.  Over the list every kernel instantiation and every run-time branch of the planner
occurs.  No GPU."""
import itertools

import numpy as np
import pytest

import wgrad_exact_ref as R

RING_INST = {("ring", 3, 1, 3), ("ring", 3, 1, 1), ("ring", 3, 2, 3), ("ring", 3, 2, 1), ("ring", 3, 4, 1), ("ring", 4, 1, 3),
             ("ring", 4, 1, 1), ("ring", 4, 2, 3), ("ring", 4, 2, 1), ("ring", 5, 1, 3), ("ring", 5, 1, 1)}
ROW_INST = {("row", kw, cotw, prec) for (kw, cotw) in ((1, 1), (1, 2), (3, 1), (3, 2), (4, 1), (5, 1)) for prec in (3, 1)}


def plan_of(case, prec):
    from mpgan_amd import train_ops
    return train_ops.conv2d_wgrad_plan(case.n, case.h, case.w, case.cin, case.cout, case.kh, case.kw, prec)


def inst(l):
    return (l["form"], l["k"], l["cotw"], l["prec"])


def pow2_scale(amax):
    """mpg::pow2_scale: the power of two that brings amax into [2^8, 2^9)"""
    _, ex = np.frexp(np.float32(amax))
    return 2.0 ** (9 - int(ex))


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_case_data_is_exact(case):
    d = R.case_data(case)
    f = case.frac
    assert R.sum_abs_bound(case.pixels, f) < 2.0 ** (24 - f), (case.pixels, f)
    assert f == 13 or R.sum_abs_bound(case.pixels, f + 1) >= 2.0 ** (23 - f)           # f is chosen from P, not fixed
    assert case.pixels < 8190 and max(case.cin, case.cout) <= 260
    for v, hi, lo in ((d.x, d.xh, d.xl), (d.d, d.dh, d.dl)):
        assert v.dtype == np.float32
        h2, l2 = R.split16(v)
        assert np.array_equal(h2, hi) and np.array_equal(l2, lo)
        assert np.array_equal(v.astype(np.float64), hi + lo)
        assert np.array_equal(np.abs(hi), np.ones_like(hi)) and (lo * hi >= 0).all()      # lo has the sign of hi
        assert np.isin(np.abs(lo) * 2.0 ** f, [0, 1, 2, 3] if f == 13 else [0, 1]).all()
        assert lo.any()
        # scaled by its own maximum (no amax handed in: both tensors; dy always)
        for e in R.EXPONENTS if v is d.d else (0,):
            vs = v * np.float32(2.0 ** e)
            assert np.array_equal(vs.astype(np.float64), v.astype(np.float64) * 2.0 ** e)
            k = pow2_scale(np.abs(vs).max())
            scaled = vs * np.float32(k)
            assert 256 <= np.abs(scaled).max() < 512
            h3, l3 = R.split16(scaled)
            assert np.array_equal(h3, hi * k * 2.0 ** e) and np.array_equal(l3, lo * k * 2.0 ** e)
    assert pow2_scale(256.0) == 1.0                                                        # train_ops.unit_amax: x unscaled
    for e in R.EXPONENTS:
        assert np.array_equal(d.dy(e).astype(np.float64), (d.dh + d.dl) * 2.0 ** e)
        for prec in case.precs:
            e64 = d.expected64(prec, e)
            assert e64.shape == (case.kh, case.kw, case.cin, case.cout)
            assert np.array_equal(e64.astype(np.float32).astype(np.float64), e64), (case, prec, e)
            unit = R.WSCALE * 2.0 ** (e - f)
            assert np.array_equal(e64 / unit, np.round(e64 / unit))
            assert np.abs(e64).max() / unit < 2.0 ** 24
    # lo * lo is not part of the definition: the full product is another number
    full = R.WSCALE * R.wgrad64(d.xh + d.xl, d.dh + d.dl, case.kh, case.kw)
    assert not np.array_equal(full, d.expected64(3, 0))
    assert np.abs(full - d.expected64(3, 0)).max() <= R.WSCALE * case.pixels * 9 * 4.0 ** -f
    # one product is another number than three
    assert not np.array_equal(d.expected64(1, 0), d.expected64(3, 0))


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_case_is_in_its_launch_class(case, mpg):
    for prec in case.precs:
        plan = plan_of(case, prec)
        assert len(plan) >= 1
        if case.launches is not None:
            assert len(plan) == case.launches, (case, prec, plan)
        l = plan[case.cls_launch]
        assert {k: l[k] for k in case.cls} == case.cls, (case, prec, l)
        check_plan(case.shape, prec, plan)


def check_plan(shape, prec, plan):
    """what any plan must satisfy: the row launches tile [0, cin) x [0, cout) without overlap, the waves of a block and its
    LDS fit, the row ranges / splits cover every image row, the grid holds every block"""
    n, h, w, cin, cout, kh, kw = shape
    ring = kh == kw and kh in (3, 4, 5)
    assert all(l["form"] == ("ring" if ring else "row") and l["prec"] == prec for l in plan)
    if ring:
        assert len(plan) == 1
        l = plan[0]
        assert inst(l) in RING_INST and l["k"] == kh
        assert l["chunks"] * 64 >= w > (l["chunks"] - 1) * 64
        assert l["n_ci"] * 32 >= cin > (l["n_ci"] - 1) * 32
        assert l["n_cow"] * 32 * l["cotw"] >= cout > (l["n_cow"] - 1) * 32 * l["cotw"]
        assert l["ranges"] * l["rows_per_range"] >= h > (l["ranges"] - 1) * l["rows_per_range"]
        assert l["n_outer"] == n * l["ranges"] * l["chunks"]
        assert l["blocks"] == -(-l["n_outer"] // 8) * 8 * l["n_ci"] * l["n_cow"]
        assert 0 < l["lds_bytes"] <= 160 * 1024
        return
    covered = np.zeros((cin, cout), dtype=np.int32)
    for l in plan:
        assert inst(l) in ROW_INST and l["k"] == kw
        assert l["cit"] in (1, 2, 4) and l["cog"] in (1, 2, 4) and l["ks"] in (1, 2, 4, 8) and l["cotw"] in (1, 2)
        assert l["cit"] * l["cog"] * l["ks"] <= 8
        assert l["cit"] * 32 >= l["cin"] >= 1 and l["cog"] * l["cotw"] * 32 >= l["cout"] >= 1
        assert l["chunk"] in (32, 64, 128, 256) and l["ks"] * 16 <= l["chunk"]
        assert l["windows"] >= 1
        assert l["nsplit"] * l["rows_per_split"] >= n * h > (l["nsplit"] - 1) * l["rows_per_split"]
        assert l["blocks"] == -(-l["nsplit"] // 8) * 8 * kh * l["windows"]
        npl = 2 if prec == 3 else 1
        xunits = l["cit"] * 4 * npl * (l["chunk"] + 20)
        dunits = l["cog"] * l["cotw"] * 4 * npl * (l["chunk"] + 4)
        assert l["lds_bytes"] == 2 * (xunits + dunits) * 16 <= 160 * 1024
        assert xunits <= 6 * 512 and dunits <= 5 * 512          # LDS-DMA instructions per wave in the copy plan
        assert l["ci0"] % 128 == 0 and l["ci0"] + l["cin"] <= cin and l["co0"] + l["windows"] * l["cout"] <= cout
        covered[l["ci0"]:l["ci0"] + l["cin"], l["co0"]:l["co0"] + l["windows"] * l["cout"]] += 1
    assert (covered == 1).all()


def test_plan_sanity_over_a_sweep(mpg):
    """the invariants of check_plan over a grid of shapes around every threshold of the planner"""
    from mpgan_amd import train_ops
    chans = (1, 8, 32, 33, 64, 65, 96, 97, 128, 129, 192, 256, 260)
    for (kh, kw), cin, cout in itertools.product(((1, 1), (3, 3), (4, 4), (5, 5), (5, 3), (2, 4), (7, 5), (6, 1)), chans, chans):
        for (n, h, w) in ((1, 1, 1), (2, 9, 33), (3, 49, 8), (1, 300, 130), (2, 513, 2), (1, 64, 257)):
            for prec in (3, 1):
                check_plan((n, h, w, cin, cout, kh, kw), prec, train_ops.conv2d_wgrad_plan(n, h, w, cin, cout, kh, kw, prec))


def test_plan_query_refuses_what_the_kernels_refuse(mpg):
    from mpgan_amd import _lib, train_ops
    lib = _lib.load()
    for (kh, kw, prec) in ((3, 2, 3), (8, 3, 3), (3, 7, 1), (0, 1, 3), (3, 3, 2), (3, 3, 0)):
        assert train_ops.conv2d_wgrad_plan(1, 8, 8, 8, 8, kh, kw, prec) == []
    assert lib.mpg_conv2d_wgrad_plan(0, 8, 8, 8, 8, 3, 3, 3, None, 0) == 0
    assert lib.mpg_conv2d_wgrad_plan(1, 8, 8, 8, 0, 3, 3, 3, None, 0) == 0
    # counting only, and a buffer shorter than the plan: nothing behind max_records is written
    import ctypes
    assert lib.mpg_conv2d_wgrad_plan(2, 5, 19, 260, 40, 1, 1, 3, None, 0) == 3
    buf = (ctypes.c_int32 * (3 * _lib.WGRAD_PLAN_INTS))(*([-7] * (3 * _lib.WGRAD_PLAN_INTS)))
    assert lib.mpg_conv2d_wgrad_plan(2, 5, 19, 260, 40, 1, 1, 3, buf, 2) == 3
    assert list(buf[2 * _lib.WGRAD_PLAN_INTS:]) == [-7] * _lib.WGRAD_PLAN_INTS
    assert list(buf[:10]) == [_lib.WGRAD_FORM_ROW, 1, 1, 3, 16, buf[5], 0, 0, 128, 40]
    assert len(train_ops.WGRAD_PLAN_FIELDS) == _lib.WGRAD_PLAN_INTS - 1       # the last int is reserved
    # a layer of the training step, written out: 5x5 128 -> 128 on 16 tiles of 64^2 runs the ring form in 32-wide windows
    (l,) = train_ops.conv2d_wgrad_plan(16, 64, 64, 128, 128, 5, 5, 3)
    assert (l["form"], l["k"], l["cotw"], l["chunks"], l["n_ci"], l["n_cow"]) == ("ring", 5, 1, 1, 4, 4)
    assert (l["ranges"], l["rows_per_range"], l["n_outer"], l["blocks"]) == (4, 16, 64, 1024)


def test_case_list_covers_the_launch_classes(mpg):
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    seen, guard_seen = set(), set()
    for case in R.CASES:
        for prec in case.precs:
            plan = plan_of(case, prec)
            for l in plan:
                seen.add(inst(l))
                if case.guard:
                    guard_seen.add(inst(l))
                if l["form"] == "row":
                    seen.update({("cit", l["cit"]), ("cog", l["cog"]), ("ks", l["ks"]), ("chunk", l["chunk"]),
                                 ("layout", l["cit"], l["cog"], l["ks"], l["cotw"]),
                                 ("windows>=2", l["windows"] >= 2, "kw>=4", l["k"] >= 4), ("merged cit", l["cit"], l["windows"] >= 2),
                                 ("rows_per_split>=2", l["rows_per_split"] >= 2), ("nsplit%8", l["nsplit"] % 8 != 0),
                                 ("launches", min(len(plan), 3)), ("kh", case.kh, "kw", case.kw),
                                 ("ragged cout window", l["cout"] % 32 != 0), ("ragged cin window", l["cin"] % 32 != 0),
                                 ("chunks per row", min(-(-case.w // l["chunk"]), 3)),
                                 ("last chunk < 16", 0 < case.w % l["chunk"] < 16 and case.w > l["chunk"])})
                    if l["rows_per_split"] >= 2:
                        # a split that holds the last row of one image and the first row of the next
                        starts = np.arange(l["nsplit"]) * l["rows_per_split"]
                        seen.add(("split straddles images", bool(((starts % case.h) + l["rows_per_split"] > case.h).any()
                                                                 and case.n > 1), "kh>1", case.kh > 1))
                else:
                    last = case.h - (l["ranges"] - 1) * l["rows_per_range"]
                    seen.update({("ranges", min(l["ranges"], 3)), ("ragged last range", l["ranges"] >= 2 and last < l["rows_per_range"]),
                                 ("row0 % (KH+1)", l["ranges"] >= 2 and l["rows_per_range"] % (l["k"] + 1) != 0),
                                 ("n_outer%8", l["n_outer"] % 8 != 0), ("h<KH", case.h < l["k"]), ("w<8", case.w < 8),
                                 ("ring chunks", min(l["chunks"], 3)), ("ring last chunk k-steps", -(-(case.w - (l["chunks"] - 1) * 64) // 16)),
                                 ("ring w%16", case.w % 16 != 0), ("n_ci", min(l["n_ci"], 5)), ("cin%8", case.cin % 8 != 0),
                                 ("cout%8", case.cout % 8 != 0), ("ragged cout window", case.cout % (32 * l["cotw"]) != 0),
                                 ("absent groups", case.cin % 32 != 0 and case.cin % 32 <= 24), ("n", case.n)})
    need = RING_INST | ROW_INST
    assert len(need) == 23
    assert need <= guard_seen, sorted(need - guard_seen)
    need |= {("cit", v) for v in (1, 2, 4)} | {("cog", v) for v in (1, 2, 4)} | {("ks", v) for v in (1, 2, 4, 8)}
    need |= {("chunk", v) for v in (32, 64, 128, 256)}
    # (cit, cog, ks, cotw): the wave layouts of the one-filter-row kernel
    need |= {("layout",) + v for v in ((1, 1, 8, 1), (1, 2, 4, 1), (1, 4, 2, 1), (2, 1, 4, 1), (2, 2, 2, 1), (2, 4, 1, 1), (4, 1, 2, 1),
                                       (4, 2, 1, 1), (4, 2, 1, 2))}
    need |= {("windows>=2", True, "kw>=4", False), ("windows>=2", True, "kw>=4", True), ("merged cit", 1, True), ("merged cit", 2, True),
             ("merged cit", 4, True), ("rows_per_split>=2", True), ("nsplit%8", True), ("nsplit%8", False), ("launches", 2), ("launches", 3),
             ("split straddles images", True, "kh>1", True), ("split straddles images", True, "kh>1", False),
             ("ragged cout window", True), ("ragged cin window", True), ("chunks per row", 2), ("chunks per row", 3),
             ("last chunk < 16", True)}
    need |= {("kh", kh, "kw", 3) for kh in (1, 2, 5, 6, 7)} | {("kh", 2, "kw", 4), ("kh", 1, "kw", 5), ("kh", 7, "kw", 5), ("kh", 1, "kw", 1)}
    need |= {("ranges", v) for v in (1, 2, 3)} | {("ragged last range", True), ("row0 % (KH+1)", True), ("n_outer%8", True),
                                                  ("n_outer%8", False), ("h<KH", True), ("w<8", True), ("ring w%16", True),
                                                  ("cin%8", True), ("cout%8", True), ("absent groups", True), ("n", 1), ("n", 3),
                                                  ("n_ci", 5)}
    need |= {("ring chunks", v) for v in (1, 2, 3)} | {("ring last chunk k-steps", v) for v in (1, 2, 3, 4)}
    assert need <= seen, sorted(need - seen, key=repr)
    assert {c.frac for c in R.CASES} == {11, 12, 13}
    assert R.GUARD_CASES and R.NORMAL_CASES and len(R.NORMAL_CASES) <= 16


def test_reference_by_hand():
    """wgrad64 on a 3x3 filter over a 2x2 image with integer data: every tap written out, and the float64 autograd of
    test_train_gpu.ref_conv_grads"""
    from test_train_gpu import ref_conv_grads
    rng = np.random.default_rng(11)
    x = rng.integers(-3, 4, size=(2, 2, 2, 3)).astype(np.float64)
    dy = rng.integers(-3, 4, size=(2, 2, 2, 2)).astype(np.float64)
    want = np.zeros((3, 3, 3, 2))
    for ky in range(3):
        for kx in range(3):
            for b in range(2):
                for oy in range(2):
                    for ox in range(2):
                        iy, ix = oy + ky - 1, ox + kx - 1
                        if 0 <= iy < 2 and 0 <= ix < 2:
                            want[ky, kx] += np.outer(x[b, iy, ix], dy[b, oy, ox])
    got = R.wgrad64(x, dy, 3, 3)
    assert np.array_equal(got, want)
    # the centre tap sees every pixel under itself, a corner tap one pixel per image
    assert np.array_equal(got[1, 1], x.reshape(8, 3).T @ dy.reshape(8, 2))
    assert np.array_equal(got[0, 0], sum(np.outer(x[b, 0, 0], dy[b, 1, 1]) for b in range(2)))
    assert np.array_equal(got[2, 0], sum(np.outer(x[b, 1, 0], dy[b, 0, 1]) for b in range(2)))
    _, dw = ref_conv_grads(x, np.zeros((3, 3, 3, 2)), dy, 1, 0.5)
    assert np.array_equal(dw, 0.5 * want)
    # even filters pad (k - 1) // 2 before: a 2x4 filter's tap (0, 1) is the pixel itself
    x = rng.integers(-3, 4, size=(1, 4, 5, 2)).astype(np.float64)
    dy = rng.integers(-3, 4, size=(1, 4, 5, 3)).astype(np.float64)
    got = R.wgrad64(x, dy, 2, 4)
    assert np.array_equal(got[0, 1], x.reshape(20, 2).T @ dy.reshape(20, 3))
    _, dw = ref_conv_grads(x, np.zeros((2, 4, 2, 3)), dy, 1, 1.0)
    assert np.array_equal(dw, got)


def test_mismatch_report_names_the_tap():
    want = np.zeros((3, 3, 40, 70), dtype=np.float32)
    assert R.mismatch_report(want, want.copy()) == ""
    got = want.copy()
    got[0, 2, 33, 65] = 1.0
    got[2, 1, 39, 69] = -0.0          # bit for bit: a sign of zero counts
    msg = R.mismatch_report(got, want, what="probe")
    assert "2 of %d values differ" % want.size in msg and "(0, 2, 33, 65)" in msg
    assert "taps hit: [(0, 2), (2, 1)]" in msg and "ci tiles hit: [1]" in msg and "cout tiles hit: [2]" in msg
    assert "shape" in R.mismatch_report(got[:1], want)
