"""Every branch of mpgan_train_conv.hip (mpg_conv2d_wgrad, mpg_conv2d_dgrad, mpg_fc_forward) and mpg_conv2d_direct, bit for
bit against the integer references of tests/train_conv_ref.py (proven on the CPU by test_train_conv_host.py, which also
proves with the restated launch arithmetic that each case sits in the branch its id names).

  constant                  value   source (mpgan_train_conv.hip: function)       cases that cross it
  micro() thresholds        16 / 32 / 64 channels -> 1 / 2 / 4 / 8 a thread   micro, mpg_conv2d_wgrad   the 16 "wgrad_kernel_MI_NI" cases: cin, cout in {5, 16 | 17, 32 | 33, 64 | 65, 130}
  tile width                16 * micro, at most 128   wgrad_kernel: TM, TN        cin / cout 130: two ragged tiles of 128 + 2
  TK                        8 pixels a step           wgrad_kernel: TK            P = 6 and P = 1 (less than one step); last slice of 92 pixels (92 % 8 = 4)
  block target              2048 blocks               launch_wgrad                every case (split = ceil(2048 / tiles) before the pixel cap)
  pixels per split          at least 128, rounded up to 8   launch_wgrad          P = 300: 3 slices of 104, last 92; P = 1023: 8 slices of 128, last 127; 3x5 s1x2: 2 slices
  filter limit              16                        MPG_GEOM_CHECK              16x1 runs, 17 is refused
  stride                    any >= 1, sh and sw apart   fill_geom, dgrad_kernel   3x5 s1x2, 2x7 s3x1 (sh != sw); 2x2 s3x3, 2x7 s3x1 (stride above the filter); stride 0 is refused
  outputs per fc block      64; a last group of one output takes the no == 1 branch   fc_fwd_kernel, fc_splitk_kernel   cout 1, 129 (one pass); cout 1, 65 (split)
  fc split: k               k >= 16384                mpg_fc_forward              (2, 16383, 64) one pass, (1, 16384, 65) split
  fc split: blocks          rows * ogroups < 512      mpg_fc_forward              (511, 16384, 1) split in two, (512, 16384, 1) one pass
  fc split: terms a block   at least 2048, kchunk rounded up to 256   mpg_fc_forward   (3, 16387, 5): 8 chunks of 2304, last 259; (16, 262144, 1): 64 chunks of 4096

The data is small integers with wscale 2^-1 (train_conv_ref): every fp32 partial sum in any order is exact, so the fp32
atomics and FMA chains have one right answer and the assertion is equality, without a tolerance."""
import numpy as np
import pytest
import torch

import train_conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CONV_IDS = [repr(c) for c in R.CONV_CASES]
FC_IDS = ["%dx%dx%d-%s" % c for c in R.FC_CASES]


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device=DEV)        # a copy: the reference's arrays are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _abi():
    from mpgan_amd import _lib, ops
    return _lib.load(), _lib, ops._stream, ops._ptr


def _conv_dev(case):
    d = R.conv_data(case)
    return {k: _dev(v) for k, v in d.items()}


def _same(got, want, what):
    msg = R.mismatch_report(_np(got), want, what)
    assert msg == "", msg


def _all_plus_zero(t):
    """every value is +0.0: no NaN, no -0.0, nothing left over"""
    return not bool(t.view(torch.int32).any())


# ---------------------------------------------------------------------------------------------- convolution gradients
@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_wgrad_exact(gpu_ops, case):
    from mpgan_amd import train_ops
    d, ref = _conv_dev(case), R.conv_reference(case)
    want = R.epilogue(ref["dw"])
    dw = train_ops.conv2d_wgrad(d["x"], d["dy"], case.kh, case.kw, (case.sh, case.sw), R.WSCALE)
    _same(dw, want, "dw")
    # a tap no output pixel reads inside the image: left by the clear, exactly +0.0
    _, tap = R.touched(case.h, case.w, case.kh, case.kw, case.sh, case.sw)
    if not tap.all():
        assert _all_plus_zero(dw[torch.as_tensor(~tap, device=DEV)])
    # the atomics must not show: a second run gives the same bits
    again = train_ops.conv2d_wgrad(d["x"], d["dy"], case.kh, case.kw, (case.sh, case.sw), R.WSCALE)
    assert torch.equal(dw, again) and torch.equal(dw.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_wgrad_of_zero_dy_is_zero(gpu_ops, case):
    """into a buffer that holds the gradient of a non-zero dy (the clear runs on every call), then into one full of NaN"""
    lib, _lib, stream, ptr = _abi()
    d, ref = _conv_dev(case), R.conv_reference(case)
    dw = torch.full((case.kh, case.kw, case.cin, case.cout), float("nan"), dtype=torch.float32, device=DEV)

    def run(dy):
        _lib.check(lib.mpg_conv2d_wgrad(stream(), ptr(d["x"]), case.n, case.h, case.w, case.cin, ptr(dy), case.cout, case.kh,
                                        case.kw, case.sh, case.sw, R.WSCALE, ptr(dw)), "mpg_conv2d_wgrad")

    run(d["dy"])
    _same(dw, R.epilogue(ref["dw"]), "dw into a NaN buffer")
    assert bool(dw.any())
    run(torch.zeros_like(d["dy"]))
    assert _all_plus_zero(dw)
    dw.fill_(float("nan"))
    run(-torch.zeros_like(d["dy"]))            # dy = -0.0: products of either sign of zero
    assert _all_plus_zero(dw)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_dgrad_exact(gpu_ops, case):
    from mpgan_amd import train_ops
    d, ref = _conv_dev(case), R.conv_reference(case)
    dx = train_ops.conv2d_dgrad(d["dy"], d["w"], (case.h, case.w), (case.sh, case.sw), R.WSCALE)
    _same(dx, R.epilogue(ref["dx"]), "dx")
    # input pixels no tap reads (stride above the filter) receive no gradient: exactly 0.0
    pix, _ = R.touched(case.h, case.w, case.kh, case.kw, case.sh, case.sw)
    if not pix.all():
        holes = dx[:, torch.as_tensor(~pix, device=DEV), :]
        assert holes.numel() == case.n * int((~pix).sum()) * case.cin and _all_plus_zero(holes)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_direct_exact(gpu_ops, case):
    d, ref = _conv_dev(case), R.conv_reference(case)
    cpu = R.conv_data(case)
    stride = (case.sh, case.sw)
    _same(gpu_ops.conv2d_direct(d["x"], d["w"], stride, R.WSCALE), R.epilogue(ref["y"]), "y plain")
    for act in R.ACTS:
        y = gpu_ops.conv2d_direct(d["x"], d["w"], stride, R.WSCALE, cout_scale=d["cout_scale"], bias=d["bias"], act=act, leak=R.LEAK)
        _same(y, R.epilogue(ref["y"], cout_scale=cpu["cout_scale"], bias=cpu["bias"], act=act), "y cout_scale bias %s" % act)
    y = gpu_ops.conv2d_direct(d["x"], d["w"], stride, R.WSCALE, bias=d["bias"])
    _same(y, R.epilogue(ref["y"], bias=cpu["bias"]), "y bias alone")


@pytest.mark.parametrize("case", R.CONV_CASES, ids=CONV_IDS)
def test_adjoint_identity_of_the_kernels(gpu_ops, case):
    """<conv(x, w), dy> = <x, dgrad(dy, w)> = <w, wgrad(x, dy)> in int64, formed on the host from what the kernels wrote"""
    from mpgan_amd import train_ops
    d, cpu = _conv_dev(case), R.conv_data(case)
    stride = (case.sh, case.sw)
    y = R.scaled_ints(_np(gpu_ops.conv2d_direct(d["x"], d["w"], stride, R.WSCALE)))
    dx = R.scaled_ints(_np(train_ops.conv2d_dgrad(d["dy"], d["w"], (case.h, case.w), stride, R.WSCALE)))
    dw = R.scaled_ints(_np(train_ops.conv2d_wgrad(d["x"], d["dy"], case.kh, case.kw, stride, R.WSCALE)))
    a, b, c = int((y * cpu["dy"]).sum()), int((cpu["x"] * dx).sum()), int((cpu["w"] * dw).sum())
    assert a == b == c, (a, b, c)


# ---------------------------------------------------------------------------------------------- fully connected layer
_FC_DEV = {}


def _fc_dev(case):
    """device copies of one case's data (the largest is 32 MB), shared by its tests"""
    if case not in _FC_DEV:
        _FC_DEV.clear()
        _FC_DEV[case] = {k: _dev(v) for k, v in R.fc_data(case).items()}
    return _FC_DEV[case]


@pytest.mark.parametrize("case", R.FC_CASES, ids=FC_IDS)
def test_fc_forward_exact(gpu_ops, case):
    from mpgan_amd import train_ops
    d, cpu, ref = _fc_dev(case), R.fc_data(case), R.fc_reference(case)
    for bias in (None, "bias"):
        for act in R.ACTS:
            y = train_ops.fc_forward(d["x"], d["w"], R.WSCALE, d["bias"] if bias else None, act, R.LEAK)
            want = R.epilogue(ref["y"], bias=cpu["bias"] if bias else None, act=act)
            _same(y, want, "y %s %s" % (bias, act))


@pytest.mark.parametrize("case", R.FC_CASES, ids=FC_IDS)
def test_fc_forward_twice_into_one_buffer(gpu_ops, case):
    """the split path adds into y with atomics: it has to clear y on every call, whatever the buffer holds (NaN, then its
    own previous result); the one-pass path overwrites"""
    lib, _lib, stream, ptr = _abi()
    d, cpu, ref = _fc_dev(case), R.fc_data(case), R.fc_reference(case)
    y = torch.full((case.rows, case.cout), float("nan"), dtype=torch.float32, device=DEV)
    want = R.epilogue(ref["y"], bias=cpu["bias"], act="lrelu")
    for turn in ("first", "second"):
        _lib.check(lib.mpg_fc_forward(stream(), ptr(d["x"]), case.rows, case.k, ptr(d["w"]), case.cout, R.WSCALE, ptr(d["bias"]),
                                      _lib.ACT_LRELU, R.LEAK, ptr(y)), "mpg_fc_forward")
        _same(y, want, "y %s call" % turn)


# ---------------------------------------------------------------------------------------------- refusals
def _small_case():
    return R.CONV_CASES[0]


def _refused(_lib, rc, entry, word):
    assert rc != _lib.MPG_OK
    with pytest.raises(_lib.MpgError) as err:
        _lib.check(rc, entry)
    assert entry in str(err.value).split(": ", 1)[1] and word in str(err.value), str(err.value)


def test_refusals_name_the_entry_and_launch_nothing(gpu_ops):
    """a filter above 16, a stride of 0 and an activation out of range are turned down on the host: MpgError with the
    entry's name, the output untouched, the device usable afterwards"""
    from mpgan_amd import train_ops
    lib, _lib, stream, ptr = _abi()
    case = _small_case()
    d, ref = _conv_dev(case), R.conv_reference(case)
    n, h, w, cin, cout = case.n, case.h, case.w, case.cin, case.cout
    sentinel = 12345.0
    dw = torch.full((17 * 17 * cin * cout,), sentinel, dtype=torch.float32, device=DEV)
    dx = torch.full((n * h * w * cin,), sentinel, dtype=torch.float32, device=DEV)
    wbig = torch.zeros((17 * 17 * cin * cout,), dtype=torch.float32, device=DEV)
    for kh, kw, sh, sw, word in ((17, 3, 1, 1, "bad filter 17x3"), (3, 17, 1, 1, "bad filter 3x17"), (3, 3, 0, 1, "bad stride"),
                                 (3, 3, 1, 0, "bad stride"), (0, 3, 1, 1, "bad filter 0x3")):
        rc = lib.mpg_conv2d_wgrad(stream(), ptr(d["x"]), n, h, w, cin, ptr(d["dy"]), cout, kh, kw, sh, sw, R.WSCALE, ptr(dw))
        _refused(_lib, rc, "mpg_conv2d_wgrad", word)
        rc = lib.mpg_conv2d_dgrad(stream(), ptr(d["dy"]), n, h, w, cin, ptr(wbig), cout, kh, kw, sh, sw, R.WSCALE, ptr(dx))
        _refused(_lib, rc, "mpg_conv2d_dgrad", word)
    with pytest.raises(_lib.MpgError, match="mpg_conv2d_wgrad: bad filter 17x17"):
        train_ops.conv2d_wgrad(d["x"], d["dy"], 17, 17, (1, 1), R.WSCALE)
    with pytest.raises(_lib.MpgError, match="mpg_conv2d_dgrad: bad filter 17x1"):
        train_ops.conv2d_dgrad(d["dy"], wbig[:17 * cin * cout].view(17, 1, cin, cout), (h, w), (1, 1), R.WSCALE)
    fc = R.FC_CASES[1]
    f = {k: _dev(v) for k, v in R.fc_data(fc).items()}
    y = torch.full((fc.rows, fc.cout), sentinel, dtype=torch.float32, device=DEV)
    for act in (-1, _lib.ACT_TANH + 1, 99):
        rc = lib.mpg_fc_forward(stream(), ptr(f["x"]), fc.rows, fc.k, ptr(f["w"]), fc.cout, R.WSCALE, ptr(f["bias"]), act, R.LEAK, ptr(y))
        _refused(_lib, rc, "mpg_fc_forward", "bad activation %d" % act)
    rc = lib.mpg_fc_forward(stream(), ptr(f["x"]), fc.rows, 0, ptr(f["w"]), fc.cout, R.WSCALE, ptr(f["bias"]), 0, R.LEAK, ptr(y))
    _refused(_lib, rc, "mpg_fc_forward", "bad shape")
    torch.cuda.synchronize()
    assert bool((dw == sentinel).all()) and bool((dx == sentinel).all()) and bool((y == sentinel).all())
    # the device still works
    _same(train_ops.conv2d_wgrad(d["x"], d["dy"], case.kh, case.kw, (case.sh, case.sw), R.WSCALE), R.epilogue(ref["dw"]), "dw afterwards")
    _same(train_ops.fc_forward(f["x"], f["w"], R.WSCALE), R.epilogue(R.fc_reference(fc)["y"]), "fc afterwards")
