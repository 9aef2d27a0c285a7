"""conv_small_kernel and conv_small_pair_kernel (csrc/mpgan_conv_small.hip) compared bit for bit with their definition,
on data whose lo planes are NOT zero, in every instantiation of both dispatch tables.

The other exact tests of these kernels use small integers (no lo plane, no fraction in the weight table), and the
relative-L2 checks cannot see a local fault: one tile pass, one halo column or one image of the batch that loses its lo
plane, a table rounded to fp16, a channel window taken from the wrong group.  The data here (conv_small_exact_ref.py)
is exact with fine activations (hi = +-1, lo = hi l 2^-13) against ternary filters, or fine filters against ternary
activations: every product is a multiple of 2^-13 and every partial sum stays below 2^11, so any order of the fmaf
chain gives the float64 sum, and the assertion is equality of bits.  There is no tolerance in this module.

test_conv_small_exact_host.py proves on the CPU that every case has these properties, that it would fail without the lo
parts or with a wrong channel group, and that the lists cover the 16 + 12 instantiations, the three forms of the column
sums and the four shapes of the weight reads.

A failure says where: the number of mismatches, the first (n, y, x, c) and its tile row, tile column and channel.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_small_exact_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 7.0


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _pack(ops, p, cin, prec):
    """the filter through mpg_conv_pack_weights: a fine one as a channel window of a wider HWIO tensor, with its wscale
    and cout_scale"""
    cs = _t(p.cout_scale) if p.cout_scale is not None else None
    return ops.pack_conv_weights(_t(p.raw), wscale=p.wscale, cout_scale=cs, c_off=p.c_off, cin=cin, prec=prec)


def _report(got, want, what):
    msg = R.mismatch_report(got.cpu().numpy(), want, R.TH, R.TW, what)
    assert not msg, msg


def _check_outputs(ops, launch, cout, want, what, g8=True):
    """`launch(want_f32, want_g8)`: the fp32 output equals `want` bit for bit; the G8 output of the same launch holds the
    same values, a G8-only launch the same int16 bits, and the channels of the group beyond cout are zero"""
    if not g8:
        y = launch(True, False)
        _report(y, want, what)
        return y
    y, g = launch(True, True)
    _report(y, want, what)
    _report(ops.from_g8(g), R.g8_roundtrip(want), what + ", G8 output")
    g2 = launch(False, True)
    assert torch.equal(g2.buf.view(torch.int16), g.buf.view(torch.int16)), what + ": G8-only launch differs"
    assert g2.c == cout and g2.groups == 1
    if cout < 8:
        assert not g2.buf[..., cout:].any().item(), what + ": channels beyond cout are not zero"
    return y


# ---------------------------------------------------------------------------------------------------------------------
# single launch
# ---------------------------------------------------------------------------------------------------------------------
def _segments(ops, case, d, scale=1.0, amax=None):
    """an fp32 tensor where the segment reads all of it (converted by the binding), else a channel window of a wider G8
    tensor that the segments naming it share; `scale` (a power of two) multiplies the activations, `amax` is the device
    scalar they are converted with"""
    shared, segs = {}, []
    for s, name, p in zip(case.segs, d.names, d.pack):
        xt = _t(d.src[name][0] * np.float32(scale))
        if amax is not None or s.window:
            assert s.c_off % 8 == 0
            if name not in shared:
                shared[name] = ops.to_g8(xt, amax=amax)
            xt = shared[name]
        segs.append(ops.Segment(xt, _pack(ops, p, s.cin, case.prec), c_off=s.c_off, up_log2=s.up_log2, pad_hi=s.pad_hi,
                                up_x_only=s.up_x_only))
    return segs


def _check(ops, case, segs, d, want, what="", g8=True, **kw):
    bias = _t(d.bias) if d.bias is not None else None
    launch = lambda f32, g8_: ops.conv2d_fused(segs, (case.h, case.w), bias=bias, act=case.act, want_f32=f32, want_g8=g8_, **kw)
    return _check_outputs(ops, launch, case.cout, want, case.name + what, g8)


@pytest.mark.parametrize("case", R.PLAIN_CASES, ids=repr)
def test_single_launch_bit_exact(gpu_ops, case):
    d = R.case_data(case)
    _check(gpu_ops, case, _segments(gpu_ops, case, d), d, d.expected())


@pytest.mark.parametrize("case", R.SEG_CASES, ids=repr)
def test_segments_in_every_rotation(gpu_ops, case):
    """segments below the launch's channel bound, each behind the barrier of the one before it in some rotation; partial
    sums are exact, so every order gives the same bits"""
    d = R.case_data(case)
    segs, first = _segments(gpu_ops, case, d), None
    for k, rot in enumerate(R.rotations(segs)):
        y = _check(gpu_ops, case, rot, d, d.expected(), ", rotation %d" % k)
        first = y if first is None else first
        assert torch.equal(y.view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("e", R.AMAX_EXPONENTS)
@pytest.mark.parametrize("case", R.AMAX_CASES, ids=repr)
def test_in_amax_undoes_the_power_of_two_scale(gpu_ops, case, e):
    """fine activations times 2^e, converted with to_g8(..., amax = max |x|) and convolved with in_amax: the expectation
    times 2^e, bit for bit"""
    d = R.case_data(case)
    x0 = d.src[d.names[0]][0]
    amax = gpu_ops.absmax(_t(x0 * np.float32(2.0 ** e)))
    assert float(amax) == float(np.abs(x0).max()) * 2.0 ** e
    want = (d.expected64() * 2.0 ** e).astype(np.float32)
    _check(gpu_ops, case, _segments(gpu_ops, case, d, scale=2.0 ** e, amax=amax), d, want, ", 2^%d" % e, g8=False, in_amax=amax)


# ---------------------------------------------------------------------------------------------------------------------
# pair
# ---------------------------------------------------------------------------------------------------------------------
def _pair_args(ops, case, d):
    """(x, c_off, packed A, packed B, packed shortcut or None, keywords) of ops.conv2d_small_pair"""
    s = case.seg
    x = _t(d.x[0])
    if s.window:
        x = ops.to_g8(x)
    pk_s = _pack(ops, d.pack_s, case.cin, case.prec) if case.ks is not None else None
    kw = dict(bias_a=_t(d.bias_a), act_a=case.act_a, bias_b=_t(d.bias_b), act_b=case.act_b, up_x_only=s.up_x_only)
    return x, s.c_off, _pack(ops, d.pack_a, case.cin, case.prec), _pack(ops, d.pack_b, case.cmid, case.prec), pk_s, kw


@pytest.mark.parametrize("case", R.PAIR_CASES, ids=repr)
def test_pair_bit_exact(gpu_ops, case):
    d = R.pair_data(case)
    x, c_off, pa, pb, ps, kw = _pair_args(gpu_ops, case, d)
    launch = lambda f32, g8: gpu_ops.conv2d_small_pair(x, c_off, case.seg.up_log2, pa, pb, ps, (case.h, case.w), want_f32=f32,
                                                       want_g8=g8, **kw)
    _check_outputs(gpu_ops, launch, case.cout, d.expected(), case.name)


def _pair_desc(ops, case, d, y):
    """the descriptor ops.conv2d_small_pair would hand to the library, with the fp32 output `y`; the tensors it points
    to are returned with it, so that they outlive the launch"""
    from mpgan_amd import _lib
    x, c_off, pa, pb, ps, kw = _pair_args(ops, case, d)
    xg = x if isinstance(x, ops.G8) else ops.to_g8(x)
    keep = (xg, pa, pb, ps, kw, y)
    p = _lib.SmallPairDesc()
    p.n, p.h, p.w = case.n, case.h, case.w
    p.x, p.cin, p.cgroups, p.g_off, p.up_log2, p.up_x_only = xg.buf.data_ptr(), case.cin, xg.groups, c_off // 8, case.seg.up_log2, case.seg.up_x_only
    p.wpack_a, p.kh_a, p.kw_a, p.cmid = pa.buf.data_ptr(), pa.kh, pa.kw, case.cmid
    p.wpack_b, p.kh_b, p.kw_b, p.cout = pb.buf.data_ptr(), pb.kh, pb.kw, case.cout
    if ps is not None:
        p.wpack_s, p.kh_s, p.kw_s = ps.buf.data_ptr(), ps.kh, ps.kw
    p.bias_a, p.bias_b = kw["bias_a"].data_ptr(), kw["bias_b"].data_ptr()
    p.act_a, p.leak_a, p.act_b, p.leak_b = _lib.act_id(case.act_a), 0.2, _lib.act_id(case.act_b), 0.2
    p.prec = case.prec
    p.y = y.data_ptr()
    return p, keep


def _refused(ops, p, y, what):
    """the launch returns MPG_ERR_ARG (MpgError through the checked binding), says why, and writes nothing"""
    from mpgan_amd import _lib
    lib = _lib.load()
    rc = lib.mpg_conv2d_small_pair(ops._stream(), ctypes.byref(p))
    assert rc == 1, (what, rc)
    with pytest.raises(_lib.MpgError):
        _lib.check(rc, what)
    assert lib.mpg_last_error()
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()), what + ": the output was written"


def test_pair_beyond_the_lds_budget_is_refused(gpu_ops):
    """8 -> 8 -> 8 with 7x7 / 7x7 filters and a 3x3 shortcut needs 167552 bytes of LDS (held on the CPU), more than a CU
    has: an error, not a launch"""
    case = R.PAIR_TOO_LARGE
    assert case.lds_bytes() == R.PAIR_TOO_LARGE_BYTES > R.LDS_MAX
    y = torch.full((case.n, case.h, case.w, case.cout), SENTINEL, dtype=torch.float32, device=DEV)
    p, keep = _pair_desc(gpu_ops, case, R.pair_data(case), y)
    _refused(gpu_ops, p, y, case.name)


def test_pair_shortcut_larger_than_7x7_is_refused(gpu_ops):
    """5x5 / 5x5 filters leave room for a 9x9 shortcut in the input tile, but no table of more than 7x7 taps can be
    packed and the sums run over at most 7 filter rows: kh_s or kw_s = 9 is MPG_ERR_ARG, nothing is launched.  The
    unchanged descriptor does launch."""
    case = R.PAIR_CASES[1]
    assert (case.ka, case.kb, case.ks) == (R.K5, R.K5, R.K1)
    d = R.pair_data(case)
    y = torch.full((case.n, case.h, case.w, case.cout), SENTINEL, dtype=torch.float32, device=DEV)
    for ks in ((9, 9), (7, 9), (9, 7)):
        p, keep = _pair_desc(gpu_ops, case, d, y)
        p.kh_s, p.kw_s = ks
        _refused(gpu_ops, p, y, "%s with a %d x %d shortcut" % (case.name, ks[0], ks[1]))
    from mpgan_amd import _lib
    p, keep = _pair_desc(gpu_ops, case, d, y)
    assert _lib.load().mpg_conv2d_small_pair(gpu_ops._stream(), ctypes.byref(p)) == 0
    torch.cuda.synchronize()
    _report(y, d.expected(), case.name + ", by descriptor")
