"""conv_mfma_f6_kernel<1> (MPG_PREC_F16F6, one cout tile) as an 8-wave block with two tile rows per wave, bit for bit.

The launch classes of the kernel are those of test_conv_exact_gpu.py, which runs unchanged.  The cases here are the
smallest shapes at which the ownership of tile rows, image pieces and staging rows by EIGHT waves can go wrong: a second
row of blocks that holds one image row (wave 0 stores one row, seven waves store nothing), a last wave whose second row is
outside the image, a 3x3 tap stream (tp = 12) whose stages end one channel group and begin the next while the next image
is in flight as one piece per wave, the direct 1x1 segment at two rows per wave in the order of block 0 and in the
flipped order of blocks 256.., and the three epilogues.

Data and expectation are those of conv_exact_ref.py (lo-exact: every fp32 partial sum is exact in any order), the
assertion is np.array_equal, the precision MPG_PREC_F16F6 alone.  tanh is no exact function: the launch with tanh and
post_add is held bit for bit against fl32(t + post_add), t being the output of the same launch without post_add (one fp32
addition per value, as the epilogue does it), and t against float64 np.tanh at the project's bound for elementwise fp32
results, relative L2 1e-6 (test_conv_epilogue_gpu.py); the same post_add window on the linear launch is exact.

The CPU test proves for every case what test_conv_exact_host.py proves for its list: the sum of |term| stays below
2^(24 - f), the expectation is an fp32 number, and the case runs where its comment says (one cout tile, the direct path,
tp, the number of blocks).
"""
import numpy as np
import pytest
import torch

import conv_exact_ref as R
from conftest import rel_l2

DEV = "cuda:0"
PREC = 2
S, Case = R.S, R.Case
F6 = (PREC,)

ROWS = Case("narrow 5x5x16->32 17x33", 1, 17, 33, 32, [S(5, 5, 16)], F6)                  # 2 x 2 blocks, one row in the second
LAST_ROW = Case("narrow 5x5x16->24 15x32", 1, 15, 32, 24, [S(5, 5, 16)], F6, g8=True)     # row 15 (wave 7, second row) is outside
TP12 = Case("narrow 3x3x40->8 16x32", 1, 16, 32, 8, [S(3, 3, 40)], F6)                    # five groups, 7.5 stages
B2B_ONE = Case("narrow 5x5x32->8 + 1x1x128 16x32", 1, 16, 32, 8, [S(5, 5, 32), S(1, 1, 128)], F6)
B2B_FLIP = Case("narrow 5x5x32->8 + 1x1x128 272x512", 1, 272, 512, 8, [S(5, 5, 32), S(1, 1, 128)], F6)
EPILOGUE = Case("narrow epilogue 3x3x24->8 19x40", 1, 19, 40, 8, [S(3, 3, 24)], F6, g8=True)     # 2 x 2 blocks, ragged both ways
K_CASES = [ROWS, LAST_ROW, TP12, B2B_ONE, B2B_FLIP]
NARROW_CASES = K_CASES + [EPILOGUE]

_data = {}


def _d(case):
    """the case's tensors and float64 partial sums: made once per process, read only"""
    if case.name not in _data:
        _data[case.name] = R.CaseData(case)
    return _data[case.name]


@pytest.mark.parametrize("case", NARROW_CASES, ids=repr)
def test_narrow_case_is_exact_and_in_its_class(case):
    assert not case.small and case.precs == F6 and (case.cout + 31) // 32 == 1
    assert R.tile_hw(case, PREC) == (16, 32)
    d = _d(case)
    assert case.frac == 13
    assert R.sum_abs_bound(case.k, case.frac) < 2.0 ** (24 - case.frac), (case.k, case.frac)
    e64 = d.expected64(PREC)
    assert np.array_equal(e64.astype(np.float32).astype(np.float64), e64)
    assert np.array_equal(e64 * 2.0 ** case.frac, np.round(e64 * 2.0 ** case.frac))
    if case.g8:
        assert np.array_equal(R.g8_roundtrip(d.expected(PREC)), d.expected(PREC))
    cls = [R.launch_class(s.kh, s.kw, s.cin, case.cout, PREC) for s in case.segs]
    assert all(c["kernel"] == "f6" and c["nt"] == 1 for c in cls)
    assert [c["direct"] for c in cls] == [int(s.kh * s.kw == 1) for s in case.segs]


def test_narrow_cases_are_the_shapes_they_name():
    assert (R.blocks(ROWS, PREC), ROWS.h % 16, ROWS.w % 32) == (4, 1, 1)
    assert (R.blocks(LAST_ROW, PREC), LAST_ROW.h) == (1, 15) and LAST_ROW.cout % 32 == 24
    c = R.launch_class(3, 3, 40, 8, PREC)
    assert (c["tp"], c["nchunks"], c["sc"]) == (12, 5, 8) and (5 * 12) % 8 == 4        # the last stage is half empty
    assert any((g * 12) % 8 for g in range(1, 5))                                      # a stage holds slots of two groups
    assert R.blocks(B2B_ONE, PREC) == 1
    assert R.blocks(B2B_FLIP, PREC) == 272 and R.launch_class(1, 1, 128, 8, PREC)["stages"] == 2
    assert R.blocks(EPILOGUE, PREC) == 4


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _segments(ops, case):
    d = _d(case)
    return [ops.Segment(_t(x), ops.pack_conv_weights(_t(w), prec=PREC), up_log2=s.up_log2, pad_hi=s.pad_hi)
            for s, x, w in zip(case.segs, d.x, d.w)]


def _equal(case, got, want, what):
    msg = R.mismatch_report(got, want, 16, 32, "%s, %s" % (case.name, what))
    assert not msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("case", K_CASES, ids=repr)
def test_narrow_k_loop_bit_exact(gpu_ops, case):
    want = _d(case).expected(PREC)
    segs = _segments(gpu_ops, case)
    y = gpu_ops.conv2d_fused(segs, (case.h, case.w))
    _equal(case, y.cpu().numpy(), want, "fp32 output")
    if len(segs) > 1:       # exact partial sums: the other order of the segments gives the same bits
        y2 = gpu_ops.conv2d_fused(segs[::-1], (case.h, case.w))
        _equal(case, y2.cpu().numpy(), want, "segments reversed")
    if case.g8:
        g = gpu_ops.conv2d_fused(segs, (case.h, case.w), want_f32=False, want_g8=True)
        assert g.c == case.cout and g.groups == (case.cout + 7) // 8       # 24 channels: no group past the third is written
        _equal(case, gpu_ops.from_g8(g).cpu().numpy(), want, "G8 output")


@pytest.mark.gpu
def test_narrow_epilogue_g8_only(gpu_ops):
    """the store from registers: no LDS staging"""
    case, want = EPILOGUE, _d(EPILOGUE).expected(PREC)
    g = gpu_ops.conv2d_fused(_segments(gpu_ops, case), (case.h, case.w), want_f32=False, want_g8=True)
    assert g.c == case.cout and g.groups == 1
    _equal(case, gpu_ops.from_g8(g).cpu().numpy(), want, "G8-only")


@pytest.mark.gpu
def test_narrow_epilogue_f32_and_g8(gpu_ops):
    """both outputs: every wave stages its rows in its own 32 LDS rows"""
    case, want = EPILOGUE, _d(EPILOGUE).expected(PREC)
    segs = _segments(gpu_ops, case)
    y, g = gpu_ops.conv2d_fused(segs, (case.h, case.w), want_f32=True, want_g8=True)
    _equal(case, y.cpu().numpy(), want, "fp32 of fp32 + G8")
    _equal(case, gpu_ops.from_g8(g).cpu().numpy(), want, "G8 of fp32 + G8")
    g2 = gpu_ops.conv2d_fused(segs, (case.h, case.w), want_f32=False, want_g8=True)
    assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16))


@pytest.mark.gpu
def test_narrow_epilogue_post_add_window_and_tanh(gpu_ops):
    """post_add reads channels 3..10 of a 12-channel tensor whose other channels are NaN; integer addends"""
    case, d = EPILOGUE, _d(EPILOGUE)
    segs = _segments(gpu_ops, case)
    pa = np.random.default_rng(5).integers(-8, 9, size=(case.n, case.h, case.w, R.POST_ADD_STRIDE)).astype(np.float32)
    win = slice(R.POST_ADD_COFF, R.POST_ADD_COFF + case.cout)
    poisoned = np.full_like(pa, np.nan)
    poisoned[..., win] = pa[..., win]
    kw = dict(post_add=_t(poisoned), post_add_coff=R.POST_ADD_COFF)
    # linear: exact
    y = gpu_ops.conv2d_fused(segs, (case.h, case.w), **kw)
    _equal(case, y.cpu().numpy(), (d.expected64(PREC) + pa[..., win]).astype(np.float32), "post_add")
    # tanh alone against float64, then tanh + post_add against one fp32 addition to it
    t = gpu_ops.conv2d_fused(segs, (case.h, case.w), act="tanh").cpu().numpy()
    err = rel_l2(t, np.tanh(d.expected64(PREC)))
    print("%s, tanh: relative L2 %.3e" % (case.name, err))
    assert err < 1e-6, err
    assert np.abs(t).max() <= 1.0 and (np.abs(t) < 1.0).any()
    y = gpu_ops.conv2d_fused(segs, (case.h, case.w), act="tanh", **kw)
    _equal(case, y.cpu().numpy(), t + pa[..., win], "tanh + post_add")
