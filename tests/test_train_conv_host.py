"""What tests/train_conv_ref.py claims, proven without a GPU: the integer references equal float64 autograd and satisfy
the adjoint identity, every contraction of every case is exact in fp32, and the case tables sit in the branches of
mpgan_train_conv.hip they are there for (by the launch arithmetic restated in train_conv_ref)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_conv_ref as R
from oracle.ops import same_pad

CONV_IDS = [repr(c) for c in R.CONV_CASES]
FC_IDS = ["%dx%dx%d-%s" % c for c in R.FC_CASES]


def _autograd(case):
    """float64 torch: y = conv2d(pad_SAME(x), w, (sh, sw)) and its gradients for the upstream dy"""
    d = R.conv_data(case)
    x = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(d["w"], dtype=torch.float64, requires_grad=True)
    _, pt, pb = same_pad(case.h, case.kh, case.sh)
    _, pl, pr = same_pad(case.w, case.kw, case.sw)
    y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w.permute(3, 2, 0, 1), stride=(case.sh, case.sw)).permute(0, 2, 3, 1)
    dx, dw = torch.autograd.grad(y, (x, w), torch.tensor(d["dy"], dtype=torch.float64))
    return y.detach().numpy(), dx.numpy(), dw.numpy()


@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_integer_references_equal_float64_autograd(case):
    y, dx, dw = _autograd(case)
    ref = R.conv_reference(case)
    assert ref["y"].dtype == ref["dx"].dtype == ref["dw"].dtype == np.int64
    assert np.array_equal(ref["y"].astype(np.float64), y)
    assert np.array_equal(ref["dx"].astype(np.float64), dx)
    assert np.array_equal(ref["dw"].astype(np.float64), dw)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_adjoint_identity_in_integers(case):
    d, ref = R.conv_data(case), R.conv_reference(case)
    a = int((ref["y"] * d["dy"]).sum())
    assert a == int((d["x"] * ref["dx"]).sum()) == int((d["w"] * ref["dw"]).sum())


@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_conv_contractions_are_exact_in_fp32(case):
    """a condition on the cases, not a tolerance: sum of |terms| < 2^23, also after cout_scale and the bias in units of the
    smallest step 2^-6 the epilogue can make (wscale 2^-1, cout_scale >= 2^-2, leak 2^-2, the lrelu factor 5/8)"""
    ref = R.conv_reference(case)
    assert ref["dw_terms"].max() < R.EXACT_LIMIT and ref["dx_terms"].max() < R.EXACT_LIMIT and ref["y_terms"].max() < R.EXACT_LIMIT
    assert (np.abs(ref["dw"]) <= ref["dw_terms"]).all()
    worst = ref["y_terms"].max() * R.WSCALE * max(R.COUT_SCALES) + R.BMAX
    assert worst * 2 ** 6 < 2 ** 24


def test_data_ranges():
    for case in R.CONV_CASES:
        d = R.conv_data(case)
        assert np.abs(d["x"]).max() <= R.XMAX and np.abs(d["dy"]).max() <= R.XMAX and np.abs(d["w"]).max() <= R.WMAX
        assert np.abs(d["bias"]).max() <= R.BMAX
        assert set(np.unique(d["cout_scale"])) <= set(np.float32(R.COUT_SCALES))
        assert d["x"].any() and d["dy"].any() and d["w"].any()
    assert R.WSCALE == 0.5 and R.LEAK == 0.25 and all(np.log2(s) == int(np.log2(s)) for s in R.COUT_SCALES)


def test_epilogue_is_exact_and_plain():
    acc = np.array([-7, -1, 0, 1, 6], np.int64)
    assert R.epilogue(acc).tolist() == [-3.5, -0.5, 0.0, 0.5, 3.0]
    assert R.epilogue(acc, act="relu").tolist() == [0.0, 0.0, 0.0, 0.5, 3.0]
    assert R.epilogue(acc, act="lrelu").tolist() == [-0.875, -0.125, 0.0, 0.5, 3.0]
    assert R.epilogue(acc, cout_scale=np.float32(0.25), bias=np.int64(-1), act="lrelu").tolist() == [-0.46875, -0.28125, -0.25, -0.21875, -0.0625]
    assert not np.signbit(R.epilogue(np.array([-1], np.int64), act="relu")).any()
    assert R.scaled_ints(np.float32([-3.5, 0.0, 2.0])).tolist() == [-7, 0, 4]
    with pytest.raises(AssertionError):
        R.scaled_ints(np.float32([0.25]))


# ---------------------------------------------------------------------------------------------------------------------
# the tables cover what they claim
# ---------------------------------------------------------------------------------------------------------------------
def _launch(case):
    return R.wgrad_launch(*case.geom)


def _source():
    """mpgan_train_conv.hip with every run of white space as one blank"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import _lib
    with open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "mpgan_train_conv.hip")) as f:
        return " ".join(f.read().split())


def _ints(pattern, src):
    found = re.findall(pattern, src)
    assert len(found) == 1, "%r: %d matches in mpgan_train_conv.hip -- the restatement in train_conv_ref.py has to follow the source" % (pattern, len(found))
    return tuple(int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],)))


def test_restated_constants_are_those_of_the_source():
    """the case tables were chosen for these constants: when one changes in mpgan_train_conv.hip, this fails, and
    train_conv_ref.py (the constants, then the cases that cross them) has to move with it"""
    src = _source()
    assert _ints(r"inline int micro\(int c\) \{ return c > (\d+) \? 8 : c > (\d+) \? 4 : c > (\d+) \? 2 : 1; \}", src) == R.MICRO_THRESHOLDS[::-1]
    assert _ints(r"constexpr int TM = 16 \* MI, TN = 16 \* NI, TK = (\d+);", src) == (R.WG_TK,)
    assert _ints(r"size_t split = \((\d+) \+ tiles - 1\) / tiles;", src) == (R.WG_TARGET_BLOCKS,)
    assert _ints(r"max_split = \(P \+ (\d+)\) / (\d+);", src) == (R.WG_MIN_PIX - 1, R.WG_MIN_PIX)
    assert _ints(r"if \(split > (\d+)\) split = (\d+);", src) == (R.WG_MAX_SPLIT, R.WG_MAX_SPLIT)
    assert _ints(r"pps = \(pps \+ (\d+)\) & ~\(size_t\)(\d+);", src) == (R.WG_TK - 1, R.WG_TK - 1)
    assert _ints(r"kh <= (\d+) && kw <= (\d+),", src) == (R.FILTER_MAX, R.FILTER_MAX)
    assert _ints(r"const int ogroups = \(cout \+ (\d+)\) / (\d+);", src) == (R.FC_GROUP - 1, R.FC_GROUP)
    assert _ints(r"if \(k >= (\d+) && \(size_t\)rows \* ogroups < (\d+)\)", src) == (R.FC_SPLIT_K, R.FC_SPLIT_BLOCKS)
    assert _ints(r"int splits = \(int\)\((\d+) / \(\(size_t\)rows \* ogroups\)\);", src) == (R.FC_TARGET_BLOCKS,)
    assert _ints(r"if \(splits > k / (\d+)\) splits = k / (\d+);", src) == (R.FC_MIN_TERMS, R.FC_MIN_TERMS)
    assert _ints(r"kchunk = \(\(k \+ splits - 1\) / splits \+ (\d+)\) / (\d+) \* (\d+);", src) == (R.FC_CHUNK - 1, R.FC_CHUNK, R.FC_CHUNK)
    assert len(re.findall(r"MPG_WG\((\d), (\d)\);", src)) == 16


def test_micro_thresholds():
    assert [R.micro(c) for c in (1, 16, 17, 32, 33, 64, 65, 130, 1024)] == [1, 1, 2, 2, 4, 4, 8, 8, 8]


def test_every_wgrad_instantiation_runs():
    table = R.CONV_CASES[:16]
    assert all(c.geom[:3] == (1, 5, 6) and c.geom[5:] == (3, 3, 1, 1) for c in table)
    assert sorted(_launch(c)[:2] for c in table) == [(mi, ni) for mi in (1, 2, 4, 8) for ni in (1, 2, 4, 8)]
    for c in table:
        assert c.why == "wgrad_kernel_%d_%d" % _launch(c)[:2]
    both = sorted(v for pair in R.MICRO_CLASSES.values() for v in pair)
    assert both == [5, 16, 17, 32, 33, 64, 65, 130]
    assert sorted({c.cin for c in table}) == both and sorted({c.cout for c in table}) == both


def _by_why(cases, why):
    (c,) = [c for c in cases if c.why == why]
    return c


def test_conv_cases_cross_the_constants_they_name():
    assert len(set(c.geom for c in R.CONV_CASES)) == len(R.CONV_CASES)
    assert all(1 <= c.kh <= R.FILTER_MAX and 1 <= c.kw <= R.FILTER_MAX for c in R.CONV_CASES)
    # ragged pixel split: three slices, the last neither full nor a multiple of TK
    c = _by_why(R.CONV_CASES, "P300-3_splits_of_104-last_92")
    mi, ni, cit, cot, split, pps = _launch(c)
    assert (c.pixels, split, pps) == (300, 3, 104) and c.pixels - (split - 1) * pps == 92 and 92 % R.WG_TK == 4
    c = _by_why(R.CONV_CASES, "P1023-8_splits-last_127-one_tile")
    mi, ni, cit, cot, split, pps = _launch(c)
    assert (c.pixels, split, pps, cit * cot * c.kh * c.kw) == (1023, 8, 128, 1) and c.pixels - 7 * pps == 127
    c = _by_why(R.CONV_CASES, "kh_ne_kw-sh_ne_sw-two_splits")
    assert c.kh != c.kw and c.sh != c.sw and _launch(c)[4] == 2
    assert same_pad(c.h, c.kh, c.sh)[1] != same_pad(c.w, c.kw, c.sw)[1]         # pt != pl: a swapped pad shows
    # two ragged channel tiles on each axis: 130 = 128 + 2
    assert any(_launch(c)[2] == 2 and c.cin % 128 == 2 for c in R.CONV_CASES)
    assert any(_launch(c)[3] == 2 and c.cout % 128 == 2 for c in R.CONV_CASES)
    assert any(_launch(c)[2:4] == (2, 2) for c in R.CONV_CASES)
    # fewer pixels than one TK step
    assert sorted(c.pixels for c in R.CONV_CASES if c.pixels < R.WG_TK) == [1, 6]
    c = _by_why(R.CONV_CASES, "P1-only_the_centre_tap")
    _, tap = R.touched(c.h, c.w, c.kh, c.kw, c.sh, c.sw)
    assert tap.sum() == 1 and tap[1, 1]
    ref = R.conv_reference(c)
    assert not ref["dw"][~tap].any() and ref["dw"][1, 1].any()
    # stride above the filter: input pixels no tap reads
    for why, holes, pixels in (("stride_above_filter-16_of_40_untouched", 16, 40), ("stride_above_filter-15_of_55_untouched", 15, 55)):
        c = _by_why(R.CONV_CASES, why)
        assert c.sh > c.kh or c.sw > c.kw
        pix, tap = R.touched(c.h, c.w, c.kh, c.kw, c.sh, c.sw)
        assert (pix.size, int((~pix).sum())) == (pixels, holes) and tap.all()
        assert not R.conv_reference(c)["dx"][:, ~pix, :].any()
    assert any(c.sh != c.sw and c.sh > c.kh for c in R.CONV_CASES)
    c = _by_why(R.CONV_CASES, "even_filter-stride2-odd_image")
    assert c.kh % 2 == 0 and c.sh == 2 and c.h % 2 == 1 and c.w % 2 == 1
    c = _by_why(R.CONV_CASES, "1x1_stride2")
    assert (c.kh, c.kw, c.sh, c.sw) == (1, 1, 2, 2) and _launch(c)[:2] == (8, 8)
    c = _by_why(R.CONV_CASES, "filter_limit_16")
    assert max(c.kh, c.kw) == R.FILTER_MAX and c.kh != c.kw


@pytest.mark.parametrize("case", R.FC_CASES, ids=FC_IDS)
def test_fc_reference_and_exactness(case):
    d, ref = R.fc_data(case), R.fc_reference(case)
    want = torch.tensor(d["x"], dtype=torch.float64) @ torch.tensor(d["w"], dtype=torch.float64)
    assert np.array_equal(ref["y"].astype(np.float64), want.numpy())
    assert ref["y_terms"].max() < R.EXACT_LIMIT and case.k * R.XMAX * R.WMAX < R.EXACT_LIMIT
    assert np.abs(d["x"]).max() <= R.XMAX and np.abs(d["w"]).max() <= R.WMAX and np.abs(d["bias"]).max() <= R.BMAX


def test_fc_cases_cross_the_constants_they_name():
    plans = {tuple(c[:3]): R.fc_plan(*c[:3]) for c in R.FC_CASES}
    assert plans == {
        (1, 1, 1): ("one",), (2, 3, 2): ("one",), (1, 255, 1): ("one",), (1, 257, 129): ("one",),
        (2, 16383, 64): ("one",),
        (1, 16384, 65): ("split", 8, 2048),
        (3, 16387, 5): ("split", 8, 2304),
        (511, 16384, 1): ("split", 2, 8192),
        (512, 16384, 1): ("one",),
        (16, 262144, 1): ("split", 64, 4096),
    }
    assert 16387 - 7 * 2304 == 259
    # both sides of k >= FC_SPLIT_K at a shape that would split, and of rows * ogroups < FC_SPLIT_BLOCKS
    assert R.fc_plan(2, 16384, 64)[0] == "split" and R.fc_plan(2, 16383, 64) == ("one",)
    # the no == 1 branch: a last output group of one output, in fc_fwd_kernel and in fc_splitk_kernel
    assert [c for c in R.FC_CASES if c.cout % R.FC_GROUP == 1 and c.cout > 1 and R.fc_plan(*c[:3]) == ("one",)]
    assert [c for c in R.FC_CASES if c.cout % R.FC_GROUP == 1 and c.cout > 1 and R.fc_plan(*c[:3])[0] == "split"]
    assert [c for c in R.FC_CASES if c.cout == 1 and R.fc_plan(*c[:3]) == ("one",)]
    assert [c for c in R.FC_CASES if c.cout == 1 and R.fc_plan(*c[:3])[0] == "split"]
