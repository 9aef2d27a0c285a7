"""Cases, data and float64 reference of the direct tests of ConvFn / ConvDgradFn / ConvWgradFn (mpgan_amd/train.py), the
three autograd Functions that give the WGAN-GP critics convolution gradients of any order (test_conv_triad_gpu.py; the
properties claimed here are proven on the CPU by test_conv_triad_host.py).

Reference: conv() below, tf.nn.conv2d SAME on NHWC / HWIO in float64 torch, differentiated by torch.autograd.  For one
case, with leaves x, w, b and u (the upstream gradient of y) and fixed projections px, pw, pb:

    y = conv(x, w * wscale) + b            (dx, dw, db) = grad(y, (x, w, b), u, create_graph=True)
    S1 = <dx, px>:  gw1 = dS1/dw = wgrad(px, u)     gu1 = dS1/du = conv(px, w)      dS1/dx = 0
    S2 = <dw, pw>:  gx2 = dS2/dx = dgrad(u, pw)     gu2 = dS2/du = conv(x, pw)      dS2/dw = 0
    S3 = <db, pb>:  gu3 = dS3/du = pb broadcast over the pixels

one projection at a time, so that each of the nine outputs is what ONE kernel path of the triad wrote.

Data: "exact" is small integers (x, u, px in [-3, 3], w, pw in [-2, 2], b, pb in [-3, 3]) and wscale = 2^-1.  Every
product is a multiple of 2^-1 and the sum of |term| of every contraction stays below 2^24 lsb, so every fp32 partial sum
in any order is exact in every kernel: the MFMA kernels at F16X3 get lo planes of zero, the abs-max scales are powers of
two, the VALU FMAs and the fp32 atomics add exact numbers.  The assertion on it is np.array_equal.  "normal" is seeded
standard normal with the He scale sqrt(2) / sqrt(kh kw cin) the networks use; "small" is the same with u and px times
1e-6, the magnitude of WGAN-GP gradients (x, w, pw stay O(1): ConvWgradFn.backward packs its upstream gradient as a
weight, without an abs-max scale).

Nothing here touches the GPU or the library under test.
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ops import same_pad

OUTPUTS = ("y", "dx", "dw", "db", "gw1", "gu1", "gx2", "gu2", "gu3")
ZEROS = ("gx1", "gw2")      # dS1/dx and dS2/dw: structurally zero
LEAVES = ("x", "w", "b", "u")
KINDS = ("exact", "normal", "small")

# which of the triad's three kernel paths writes an output (db: mpg_channel_sum_ordered; gu3: a broadcast view)
PATH_OF = {"y": "fwd", "gu1": "fwd", "gu2": "fwd", "dx": "dgrad", "gx2": "dgrad", "dw": "wgrad", "gw1": "wgrad",
           "db": "sum", "gu3": "sum"}

# relative L2 the project holds its kernels to (tests/test_train_gpu.py): an output of an MFMA kernel at F16X3, of an
# fp32 vector-ALU kernel (conv2d_direct, conv2d_dgrad, conv2d_wgrad, fc_forward, the ordered channel sum)
TOL_MFMA, TOL_VALU = 2e-5, 1e-5


class Case(collections.namedtuple("Case", "name n h w cin cout kh kw stride fc s2d fwd dgrad wgrad chunks")):
    """one layer shape.  s2d: driven as TrainSession drives a 4x4 stride-2 layer, as the 3x3 stride-1 convolution of
    strided4_as_3x3(w) over space_to_depth2(x), and compared with the stride-2 reference on the original x, w.
    fwd / dgrad / wgrad: the branch of _conv_fwd / _conv_dgrad / _conv_wgrad the case is there for ("mfma", "direct",
    "fc", "valu"; wgrad "ring" / "row" = the two matrix-core forms); chunks: (launches of _mfma_conv on the forward
    side, on the data-gradient side), 0 where that side is no MFMA launch.  The host test checks all of them."""

    __slots__ = ()

    def __repr__(self):
        return self.name

    @property
    def launch(self):
        """(cin, cout, kh, kw, stride) of the convolution the Functions see"""
        if self.s2d:
            return 4 * self.cin, self.cout, 3, 3, 1
        return self.cin, self.cout, self.kh, self.kw, self.stride

    @property
    def out_hw(self):
        return -(-self.h // self.stride), -(-self.w // self.stride)

    def tol(self, name):
        path = PATH_OF[name]
        if path == "sum":
            return TOL_VALU
        return TOL_MFMA if getattr(self, path) in ("mfma", "ring", "row") else TOL_VALU


def C(name, n, h, w, cin, cout, kh, kw, stride=1, fc=False, s2d=False, fwd="mfma", dgrad="mfma", wgrad="ring", chunks=(1, 1)):
    return Case(name, n, h, w, cin, cout, kh, kw, stride, fc, s2d, fwd, dgrad, wgrad, chunks)


CASES = [
    # MFMA forward, MFMA data gradient, ring weight gradient; an odd, ragged image
    C("3x3 8->16 9x11", 2, 9, 11, 8, 16, 3, 3),
    # even filter: asymmetric SAME pad (1 before, 2 after), the data gradient runs with pad_hi=1 over mirrored weights
    C("4x4 16->24 8x10", 2, 8, 10, 16, 24, 4, 4),
    # _mfma_conv in chunks of 128 + 8: over cout on the forward side, over cin on the data-gradient side
    C("4x4 136->136 6x8", 1, 6, 8, 136, 136, 4, 4, chunks=(2, 2)),
    # kw = 1: the one-filter-row weight-gradient kernel
    C("1x1 9->17 12x12", 2, 12, 12, 9, 17, 1, 1, wgrad="row"),
    # wgrad_mfma_ok false (kw = 7): vector-ALU weight gradient beside MFMA forward and data gradient
    C("7x7 4->4 8x8", 2, 8, 8, 4, 4, 7, 7, wgrad="valu"),
    # _mfma_ok false by width on the forward side (conv2d_direct); MFMA data gradient with a 520-long contraction
    C("1x1 8->520 4x4", 2, 4, 4, 8, 520, 1, 1, fwd="direct", wgrad="row", chunks=(0, 1)),
    # stride 2 on odd sizes: conv2d_direct, conv2d_dgrad, conv2d_wgrad
    C("4x4s2 6->12 9x7", 2, 9, 7, 6, 12, 4, 4, stride=2, fwd="direct", dgrad="valu", wgrad="valu", chunks=(0, 0)),
    # the rewrite TrainSession applies to 4x4 stride-2 layers on even images: 3x3 stride 1 over 24 channels
    C("4x4s2 6->12 8x10 as 3x3", 2, 8, 10, 6, 12, 4, 4, stride=2, s2d=True),
    # the fully connected layer: fc_forward, vector-ALU gradients under cfg["fc"]
    C("fc 300->1", 4, 1, 1, 300, 1, 1, 1, fc=True, fwd="fc", dgrad="valu", wgrad="valu", chunks=(0, 0)),
]

# the only shape at which _conv_prec picks MPG_PREC_F16F6 (kh kw cin > F16F6_MIN_K, cout <= 128): the chunked case
# with cout = 128.  Forward and data gradient (136 -> 128 is two launches of 128 + 8 output channels there, and the
# 8-wide one has kh kw cin = 16 * 128 > 256 too) at F16F6, weight gradient at F16X3
F16F6_CASE = C("4x4 136->128 6x8 f16f6", 1, 6, 8, 136, 128, 4, 4, chunks=(1, 2))
TOL_F16F6 = 1.5e-4          # per-layer bound of test_conv2d_fused_f16f6

EXACT_WSCALE = 0.5
XMAX, WMAX, BMAX = 3, 2, 3


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def shapes(case):
    oh, ow = case.out_hw
    return dict(x=(case.n, case.h, case.w, case.cin), w=(case.kh, case.kw, case.cin, case.cout), b=(case.cout,),
                u=(case.n, oh, ow, case.cout), px=(case.n, case.h, case.w, case.cin),
                pw=(case.kh, case.kw, case.cin, case.cout), pb=(case.cout,))


@functools.lru_cache(maxsize=None)
def make_data(case, kind):
    """(dict of float32 arrays x, w, b, u, px, pw, pb, wscale)"""
    assert kind in KINDS
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (case.name, "exact" if kind == "exact" else "normal")).encode()))
    d = {}
    for name, shape in shapes(case).items():
        if kind == "exact":
            m = WMAX if name in ("w", "pw") else BMAX if name in ("b", "pb") else XMAX
            d[name] = rng.integers(-m, m + 1, size=shape).astype(np.float32)
        else:
            d[name] = rng.standard_normal(shape).astype(np.float32)
    if kind == "small":
        d["u"] = (d["u"] * np.float32(1e-6)).astype(np.float32)
        d["px"] = (d["px"] * np.float32(1e-6)).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    if kind == "exact":
        return d, EXACT_WSCALE
    return d, float(np.float32(math.sqrt(2.0) / math.sqrt(case.kh * case.kw * case.cin)))


def term_bounds(case):
    """worst-case sum of |term|, in units of the smallest step 2^-1 = EXACT_WSCALE, of the three contractions on the
    exact data: forward over kh kw cin, data gradient over kh kw cout, weight gradient over the n oh ow pixels"""
    oh, ow = case.out_hw
    return dict(fwd=case.kh * case.kw * case.cin * XMAX * WMAX, dgrad=case.kh * case.kw * case.cout * XMAX * WMAX,
                wgrad=case.n * oh * ow * XMAX * XMAX)


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def conv(x, w, stride=1):
    """tf.nn.conv2d(x, w, stride, "SAME"): x [N,H,W,Cin], w [kh,kw,Cin,Cout] torch tensors -> [N,OH,OW,Cout]"""
    _, pt, pb = same_pad(x.shape[1], w.shape[0], stride)
    _, pl, pr = same_pad(x.shape[2], w.shape[1], stride)
    y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w.permute(3, 2, 0, 1), stride=stride)
    return y.permute(0, 2, 3, 1)


def conv_loop(x, w, stride):
    """the same in explicit numpy loops, from the definition: out[n, Y, X, o] = sum x[n, Y s + a - pt, X s + b - pl, c]
    w[a, b, c, o] over the taps that fall inside the image"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    oh, pt, _ = same_pad(h, kh, stride)
    ow, pl, _ = same_pad(wd, kw, stride)
    out = np.zeros((n, oh, ow, cout))
    for i in range(n):
        for yy in range(oh):
            for xx in range(ow):
                for a in range(kh):
                    for b in range(kw):
                        sy, sx = yy * stride + a - pt, xx * stride + b - pl
                        if 0 <= sy < h and 0 <= sx < wd:
                            out[i, yy, xx] += x[i, sy, sx] @ w[a, b]
    return out


def derivatives(fn, t, allow_zero=False):
    """the outputs of OUTPUTS + ZEROS of y = fn(x, w, b) for the leaves t = dict(x, w, b, u, px, pw, pb), taken with the
    autograd calls of the module docstring.  Shared by the reference and the GPU test: the calls are the same, only fn
    and the tensors differ.  A structural zero comes back as None (autograd found no path) or as a tensor."""
    x, w, b, u = t["x"], t["w"], t["b"], t["u"]
    y = fn(x, w, b)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), u, create_graph=True)
    gx1, gw1, gu1 = torch.autograd.grad((dx * t["px"]).sum(), (x, w, u), retain_graph=True, allow_unused=True)
    gx2, gw2, gu2 = torch.autograd.grad((dw * t["pw"]).sum(), (x, w, u), retain_graph=True, allow_unused=True)
    (gu3,) = torch.autograd.grad((db * t["pb"]).sum(), (u,), allow_unused=allow_zero)
    return dict(y=y, dx=dx, dw=dw, db=db, gw1=gw1, gu1=gu1, gx2=gx2, gu2=gu2, gu3=gu3, gx1=gx1, gw2=gw2)


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """dict name -> float64 array (None for a structural zero autograd left out), computed once per (case, kind)"""
    d, wscale = make_data(case, kind)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k in LEAVES) for k, v in d.items()}
    out = derivatives(lambda x, w, b: conv(x, w * wscale, case.stride) + b, t)
    res = {}
    for k, v in out.items():
        res[k] = None if v is None else v.detach().numpy()
        if res[k] is not None:
            res[k].setflags(write=False)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# diagnosis
# ---------------------------------------------------------------------------------------------------------------------
def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def mismatch_report(got, want, what=""):
    """'' when the fp32 arrays are equal bit for bit (a zero of either sign equals a zero); else how many values differ,
    the first index, the values there and the largest difference (the model is conv_exact_ref.mismatch_report)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if got.dtype != np.float32 or want.dtype != np.float32:
        return "%s: dtypes %s / %s, expected float32" % (what, got.dtype, want.dtype)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return ""
    idx = tuple(int(v) for v in bad[0])
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ratio = float(got[idx]) / float(want[idx]) if want[idx] != 0 else float("nan")
    return ("%s: %d of %d values differ (max |diff| %.3e); first at %s: got %r, expected %r (ratio %.6g)"
            % (what, len(bad), got.size, float(err.max()), idx, float(got[idx]), float(want[idx]), ratio))
