"""The bf6 (e3m2) quantisers of MPG_PREC_F16F6 read out of the kernels exactly, on data with arbitrary exponents and
mantissas (conv_f6_quant_ref.py holds the model and the data, test_conv_f6_quant_host.py proves their properties):

  (a) the byte image of mpg_conv_pack_weights(prec = 2) of general weights, decoded and compared with the model: fp16
      values, scale bytes and codes;
  (b) the activation quantiser (block maximum, exponent, v_cvt_scalef32_pk32_bf6_f16) through one-hot weights: output
      channel co holds the single weight s 2^j at one K index, so y = s 2^j (a_hi + q(a_lo)) there, and with the weight
      s 2^j (1 + 2^-12), whose lo part is one bf6 code, plus s 2^(j - 12) q(a_hi): exact in fp32;
  (c) the weight codes and scale bytes as the kernel applies them, through impulse activations: y around an impulse of 1.0 is
      w_hi + q(w_lo), around one of 1 + 2^-12 plus 2^-12 q(w);
  (d) dense general data on both sides against the model, within the bound of fp32 accumulation in any order.

(a) - (c) compare bit for bit.  A failure of (b) or (c) names the first (n, y, x, c) and its tile.
"""
import numpy as np
import pytest
import torch

import conv_exact_ref as R
import conv_f6_quant_ref as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _g8(ops, hi, lo, cin):
    """fp16 planes [n, groups, h, w, 8] -> the G8 tensor [n, groups, 2, h, w, 8], built by hand"""
    buf = torch.as_tensor(np.ascontiguousarray(np.stack([hi, lo], axis=2)), device=DEV)
    assert buf.dtype == torch.float16
    n, _, _, h, w, _ = buf.shape
    return ops.G8(buf, n, h, w, cin)


def _launch(ops, case, size, xs, ws):
    segs = [ops.Segment(x, ops.pack_conv_weights(_t(w), prec=2) if isinstance(w, np.ndarray) else w) for x, w in zip(xs, ws)]
    return ops.conv2d_fused(segs, size).cpu().numpy()


def _assert_none(msgs):
    assert not msgs, "%d launches differ; the first: %s" % (len(msgs), " || ".join(msgs[:3]))


@pytest.mark.parametrize("shape", Q.PACK_SHAPES, ids=repr)
def test_pack_image_byte_for_byte(gpu_ops, shape):
    kh, kw, cin_total, c_off, cin, cout, wscale, _ = shape
    w, cs = Q.pack_case(shape)
    pk = gpu_ops.pack_conv_weights(_t(w), wscale=wscale, cout_scale=None if cs is None else _t(cs), c_off=c_off, cin=cin, prec=2)
    got = Q.decode_pack_image(pk.buf.cpu().numpy(), kh, kw, cin, cout)
    want = Q.weight_model(w, wscale, cs, c_off, cin)
    assert np.array_equal(got.hi16.view(np.uint16), want.hi16.view(np.uint16)), "fp16 fragments"
    assert np.array_equal(got.eh, want.eh), "scale byte of the w_hi blocks"
    assert np.array_equal(got.el, want.el), "scale byte of the w_lo blocks"
    assert np.array_equal(got.scale_bytes[0], got.scale_bytes[1]), "the two planes hold the same scale word"
    assert not got.scale_bytes[..., 2:].any() and not got.spare.any(), "bytes 10-15 of half 1"
    for name in ("code_hi", "code_lo"):
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, "%s: %d codes differ, first at (row, block, element) %s: got %d, expected %d" % (
            name, len(bad), tuple(bad[0]), got[name][tuple(bad[0])], want[name][tuple(bad[0])])


@pytest.mark.parametrize("size", Q.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", Q.B_CASES, ids=repr)
def test_activation_codes_through_one_hot_weights(gpu_ops, case, size):
    xs = [_g8(gpu_ops, hi, lo, cin) for (hi, lo), (_, _, cin) in zip(Q.b_activations(case, size), case.segs)]
    msgs = []
    for launch in range(Q.b_launches(case)):
        for second in (False, True):
            y = _launch(gpu_ops, case, size, xs, Q.b_weights(case, launch, second))
            want = Q.to_f32(sum(Q.b_terms(case, size, launch, second)))
            assert want.any()
            msg = R.mismatch_report(y, want, 16, 32, "%s %dx%d, launch %d%s" % (case, size[0], size[1], launch, ", w_lo" if second else ""))
            if msg:
                msgs.append(msg)
    _assert_none(msgs)


@pytest.mark.parametrize("size", Q.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", Q.C_CASES, ids=repr)
def test_weight_codes_through_impulses(gpu_ops, case, size):
    pks = [gpu_ops.pack_conv_weights(_t(w), prec=2) for w in Q.c_weights(case)]
    msgs = []
    for launch in range(Q.c_launches(case, size)):
        for second in (False, True):
            hi, lo = Q.c_activations(case, size, launch, second)
            y = _launch(gpu_ops, case, size, [_g8(gpu_ops, hi, lo, case.segs[0][2])], pks)
            want = Q.to_f32(sum(Q.c_terms(case, size, launch, second)))
            assert want.any()
            msg = R.mismatch_report(y, want, 16, 32, "%s %dx%d, launch %d%s" % (case, size[0], size[1], launch, ", a_lo" if second else ""))
            if msg:
                msgs.append(msg)
    _assert_none(msgs)


@pytest.mark.parametrize("case", Q.D_CASES, ids=repr)
def test_dense_general_data_within_the_accumulation_bound(gpu_ops, case):
    """|y - expected64| <= (3 K_padded + 1) 2^-23 sum |terms| per element (conv_f6_quant_ref.d_expected: derived, not
    measured).  Largest observed ratio to the bound on an MI355X: 0.0038 (3x3x24->40), 0.0042 (5x5x16->128)."""
    size = Q.D_SIZE
    xs = [_g8(gpu_ops, hi, lo, cin) for (hi, lo), (_, _, cin) in zip(Q.b_activations(case, size), case.segs)]
    y = _launch(gpu_ops, case, size, xs, Q.d_weights(case)).astype(np.float64)
    e, bound = Q.d_expected(case)
    err = np.abs(y - e)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: largest |y - expected| / bound = %.4f" % (case, ratio.max()))
    assert np.isfinite(y).all()
    assert (err <= bound).all(), "%s: %d of %d beyond the bound, largest ratio %.3f at %s" % (
        case, int((err > bound).sum()), err.size, ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
