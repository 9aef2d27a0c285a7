"""CPU twin of test_conv_f6_barrier_gpu.py: for every case of conv_f6_barrier_cases.py the data is lo-exact and splits as
intended, the sum of |term| stays below 2^(24 - f) (every fp32 partial sum is exact in any order, so np.array_equal is
the right assertion), the float64 expectation is an fp32 number, and the case runs the stage loop (`pref`), the stage
count and the cout tiling its comment names -- through conv_exact_ref.launch_class, which is held against
mpg_conv_pack_size.  No GPU."""
import numpy as np
import pytest

import conv_exact_ref as R
import conv_f6_barrier_cases as B

# expectations of the two large cases are formed (and checked) on the GPU box only: same generator, same bound
SMALL_ENOUGH = [c for c in B.CASES if c.n * c.h * c.w <= 4096]


@pytest.mark.parametrize("case", B.CASES, ids=repr)
def test_bound_and_launch_class(mpg, case):
    from mpgan_amd import _lib
    lib = _lib.load()
    assert case.precs == (2,) and not case.small and case.act is None
    assert 1 <= len(case.segs) <= R.MAX_SEG
    assert case.frac == 13 and R.sum_abs_bound(case.k, case.frac) + B.POST_ADD_RANGE < 2.0 ** (24 - case.frac), case.k
    want = [case.cls] + ([dict(kernel="f6", nt=case.cls["nt"], **B.SECOND[case.name])] if len(case.segs) > 1 else [])
    assert len(want) == len(case.segs)
    for s, cls in zip(case.segs, want):
        c = R.launch_class(s.kh, s.kw, s.cin, case.cout, 2)
        if case.post_add:       # the classifier names conv_small_kernel for the shape alone; post_add sends it to the MFMA launch
            assert c["kernel"] == "small" and s.cin <= 8 and case.cout <= 8
            c["kernel"] = "f6"
        assert {k: c[k] for k in cls} == cls, (case, s, c)
        got = lib.mpg_conv_pack_size(s.kh, s.kw, s.cin, case.cout, 2)
        assert got > 0 and got == R.pack_bytes(s.kh, s.kw, s.cin, case.cout, 2), (case, s, got)
        assert c["wstage"] == 8 * c["nt"] * 1024
    assert not case.post_add or all(s.kh * s.kw * s.cin <= 200 for s in case.segs)


def test_case_list_covers_what_the_moved_barrier_can_break():
    names = [c.name for c in B.CASES]
    assert len(set(names)) == len(names) and set(B.SECOND) <= set(names)
    first = {(c.cls["nt"], c.cls["stages"]) for c in B.CASES if len(c.segs) == 1}
    assert first >= {(nt, ns) for nt in (1, 4) for ns in (1, 2, 3, 4)}            # shorter than, as long as, longer than the ring
    cls = lambda c: R.launch_class(c.segs[0].kh, c.segs[0].kw, c.segs[0].cin, c.cout, 2)
    multi = [(c.cls["nt"], cls(c)["pref"], cls(c)["tp"]) for c in B.CASES if cls(c)["nchunks"] > 1]
    assert {m[:2] for m in multi} >= {(nt, 1) for nt in (1, 2, 3, 4)}             # an image in flight across the barrier
    assert {m[1:] for m in multi} >= {(0, 8), (0, 12), (1, 25)}
    assert {m[0] for m in multi if m[1] == 0} >= {1, 2, 3, 4}
    assert {(c.h, c.w) for c in B.CASES} >= {(17, 33), (15, 32), (16, 32), (272, 512)}
    blocks = {c.name: R.blocks(c, 2) for c in B.CASES}
    assert blocks["600 blocks 5x5x16->16"] == 600
    assert blocks["5x5x32 + direct 1x1x128 ->8 272x512"] == 272                  # > 256 blocks of one cout tile: both seg_flip orders
    assert sum(len(c.segs) == 2 for c in B.CASES) == 4


@pytest.mark.parametrize("case", SMALL_ENOUGH, ids=repr)
def test_case_data_is_exact(case):
    d = R.case_data(case)
    for s, x, w, ((xh, xl), (wh, wl)) in zip(case.segs, d.x, d.w, d.parts):
        for v, hi, lo in ((x, xh, xl), (w, wh, wl)):
            assert v.dtype == np.float32
            h2, l2 = R.split16(v)
            assert np.array_equal(h2, hi) and np.array_equal(l2, lo), (case, s)
            assert np.array_equal(np.abs(hi), np.ones_like(hi)) and (lo * hi >= 0).all()
            assert np.isin(np.abs(lo) * 2.0 ** 13, [0, 1, 2, 3]).all() and lo.any()
    e64 = d.expected64(2)
    assert np.array_equal(e64.astype(np.float32).astype(np.float64), e64), case
    assert np.array_equal(e64 * 2.0 ** 13, np.round(e64 * 2.0 ** 13))
    assert not np.array_equal(d.expected(1), d.expected(2))                      # the corrections are in the result
