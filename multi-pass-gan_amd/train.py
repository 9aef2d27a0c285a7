"""Training step of the 4x multi-pass GAN on the HIP kernels.

The reference builds one TF graph and lets ``tf.gradients`` + ``AdamOptimizer.minimize`` walk it
(multipassGAN-4x.py:728-902, training loop :1300-1360).  Here the same ``graph`` nodes are executed
eagerly by ``TrainSession``; every layer is a ``torch.autograd.Function`` whose forward AND backward
are kernels of libmpgan_hip.so (conv forward + data gradient on the MFMA kernel, weight gradient,
batch-norm statistics, activation / resize / pool / pixel-norm backward).  torch supplies the tape,
views (reshape / concat / slice), the scalar loss reductions and device memory, as north_star puts
the losses and optimiser bookkeeping host/PyTorch side; the Adam update itself is ``mpg_adam_step``
with TensorFlow's epsilon placement.
"""
import contextlib
import math
import os

import numpy as np

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops, train_ops
from . import graph as G
from .session import seeded_normal

TRAINABLE_KINDS = ("weight", "bias", "gamma", "beta")


def _mfma_ok(kh, kw, width, stride):
    """the fused MFMA kernel takes stride-1 filters up to 7x7; a launch covers up to 128 output channels, and layers of
    up to 512 (the 256-wide d_c4, multipassGAN-4x.py:614) run as one launch per 128 (_mfma_conv)"""
    return stride == (1, 1) and kh <= 7 and kw <= 7 and width <= 512


def _conv_prec(prec, kh, kw, cin, cout):
    """the precision a forward / data-gradient convolution of the training step runs at when the trainer asks for `prec`:
    MPG_PREC_F16F6 (the inference default: 1e-4-grade, 1.6x faster on the wide layers) where the kernels cover the shape and
    the contraction is long enough to pay for it (the session's rule), else the fp32-grade three-product mode"""
    if prec != ops.PREC_F16F6:
        return prec
    if kh * kw * cin > ops.F16F6_MIN_K and ops.f6_available(cout, [(kh, kw, cin)]):
        return ops.PREC_F16F6
    return ops.PREC_F16X3


def _wgrad_prec(prec):
    """weight gradients contract over pixels on fp16 hi/lo splits only: three products unless one is asked for"""
    return prec if prec == ops.PREC_F16X1 else ops.PREC_F16X3


def _cached_g8(t, scaled):
    """(G8 form of t, the abs-max it was scaled by or None), kept on the tensor object.
    scaled False: the plain hi/lo split of an activation -- a block's input feeds two convolutions (first conv and 1x1
    shortcut), the second one finds the form the first one made.  scaled True: t times the power of two of its abs-max -- a
    gradient that enters both the data- and the weight-gradient convolution of a layer (or a second-order forward and its
    weight gradient) is reduced and converted once.
    A cached copy is valid while the tensor holds the values it was made from.  The tag (`_version`, `data_ptr`, shape) sees
    in-place torch operations and a swapped storage; it does NOT see a library kernel writing through the raw pointer, so no
    tensor that is converted here may be rewritten that way afterwards.  Today none is: the kernels' outputs are fresh tensors,
    and what the library updates in place (the optimisers' flat parameter buffers, the batch-norm moving averages) are
    variables, which are packed as weights or read as vectors and never come here."""
    tags = getattr(t, "_mpg_g8", None)
    tag = None if tags is None else tags.get(scaled)
    if tag is None or tag[2:] != (t._version, t.data_ptr(), tuple(t.shape)):
        tc = t.detach().contiguous()
        am = ops.absmax(tc) if scaled else None
        tag = (ops.to_g8(tc, 0, tc.shape[3], amax=am), am, t._version, t.data_ptr(), tuple(t.shape))
        try:
            if tags is None:
                tags = t._mpg_g8 = {}
            tags[scaled] = tag
        except AttributeError:      # a tensor type that takes no attributes: convert every time
            pass
    return tag[0], tag[1]


def _attach_g8(t, g8):
    """hand _cached_g8 the unscaled G8 form of t that the kernel producing t wrote alongside (mpg_bn_infer_act)"""
    t._mpg_g8 = {False: (g8, None, t._version, t.data_ptr(), tuple(t.shape))}


def _dgrad_weights(w):
    """[kh,kw,cin,cout] -> [kh,kw,cout,cin] with the taps mirrored: the data gradient as a forward convolution over dy"""
    return w.flip(0, 1).permute(0, 1, 3, 2).contiguous()


def _mfma_conv(x, w, wscale, prec, bias=None, act=None, leak=0.2, pad_hi=0, rescale=False, amax=None, keep=None):
    """conv2d_SAME(x, w * wscale) [+ bias, act] on the MFMA kernel, output channels in chunks of 128.
    rescale: x is a gradient (1e-4 .. 1e-8 in magnitude, below the fp16 normal range): it is split into
    fp16 hi/lo after a power-of-two scaling by its absolute maximum, and the sum is scaled back in the epilogue.
    keep: a list that receives the G8 form of x the kernel read (the weight gradient reads the same tensor)"""
    kh, kw, cin, cout = w.shape
    outs = []
    if not rescale:
        amax = None
        if isinstance(x, torch.Tensor):
            x = _cached_g8(x.contiguous(), False)[0]
    elif isinstance(x, torch.Tensor):
        amax = ops.absmax(x) if amax is None else amax
        x = ops.to_g8(x.contiguous(), 0, x.shape[3], amax=amax)
    for c0 in range(0, cout, 128):
        c1 = min(cout, c0 + 128)
        wc = w if (c0 == 0 and c1 == cout) else w[..., c0:c1].contiguous()
        pk = ops.pack_conv_weights(wc, wscale=wscale, prec=_conv_prec(prec, kh, kw, cin, c1 - c0))
        bc = None if bias is None else (bias if (c0 == 0 and c1 == cout) else bias[c0:c1].contiguous())
        seg = ops.Segment(x, pk, pad_hi=pad_hi)
        if len(outs) == 0 and keep is not None:
            keep.append(seg.x)
        if len(outs) == 0 and c1 < cout and isinstance(x, torch.Tensor):
            x = seg.x                       # reuse the G8 conversion for the other chunks
        outs.append(ops.conv2d_fused([seg], (seg.x.h, seg.x.w), bias=bc, act=act, leak=leak, in_amax=amax))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=3)


class ConvLayerFn(torch.autograd.Function):
    """act(bn_train?(conv2d_SAME(x, W * wscale) + b)) as GAN.convolutional_layer builds it
    (GAN.py:80-119); one fused conv launch (+ the batch-statistics passes when BN is on)."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, cfg):
        stride, wscale, act, leak = cfg["stride"], cfg["wscale"], cfg["act"], cfg["leak"]
        kh, kw, cin, cout = w.shape
        x = x.contiguous()
        x_g8 = None
        bn = gamma is not None
        conv_act = None if bn else act
        if cfg.get("fc"):
            lin = train_ops.fc_forward(x.reshape(x.shape[0], cin), w.detach().reshape(cin, cout), wscale, b, conv_act,
                                       leak).reshape(x.shape[0], 1, 1, cout)
        elif _mfma_ok(kh, kw, cout, stride):
            keep = [] if (ctx.needs_input_grad[1] and train_ops.wgrad_mfma_ok(kh, kw, stride)) else None
            lin = _mfma_conv(x, w.detach().contiguous(), wscale, cfg["prec"], b.detach() if b is not None else None,
                             conv_act, leak, keep=keep)
            x_g8 = keep[0] if keep else None
        else:
            lin = ops.conv2d_direct(x, w.detach().contiguous(), stride, wscale, None, b, conv_act, leak)
        if bn:
            mm, mv = cfg.get("moving", (None, None))
            y, mean, var = train_ops.bn_train_fwd(lin, gamma, beta, cfg["eps"], act, leak, mm, mv, cfg.get("decay", 0.999))
            cfg["batch_stats"] = (mean, var)
            ctx.save_for_backward(x, w, lin, mean, var, gamma, y)
        else:
            y = lin
            ctx.save_for_backward(x, w, y)
        ctx.cfg, ctx.bn, ctx.has_bias = cfg, bn, b is not None
        ctx.x_g8 = x_g8                      # the forward input as the kernel read it (hi/lo fp16, unscaled): the weight gradient's operand
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        cfg = ctx.cfg
        stride, wscale, act, leak = cfg["stride"], cfg["wscale"], cfg["act"], cfg["leak"]
        x_g8, ctx.x_g8 = ctx.x_g8, None
        if ctx.bn:
            x, w, lin, mean, var, gamma, y = ctx.saved_tensors
        else:
            x, w, y = ctx.saved_tensors
        kh, kw, cin, cout = w.shape
        d = dy.contiguous()
        # max |d| (the power-of-two scale of both gradient convolutions) comes out of the kernel that produces d
        need_amax = stride == (1, 1) and not cfg.get("fc")
        d_amax = None
        if act is not None:
            if need_amax and not ctx.bn:
                d, d_amax = train_ops.act_bwd(d, y, act, leak, want_amax=True)
            else:
                d = train_ops.act_bwd(d, y, act, leak)
        dgamma = dbeta = None
        if ctx.bn:
            if need_amax:
                d, dgamma, dbeta, d_amax = train_ops.bn_train_bwd(d, lin, mean, var, gamma, cfg["eps"], want_amax=True)
            else:
                d, dgamma, dbeta = train_ops.bn_train_bwd(d, lin, mean, var, gamma, cfg["eps"])
        db = train_ops.channel_sum(d) if ctx.has_bias else None
        dw = None
        if need_amax and d_amax is None:
            d_amax = ops.absmax(d)                                                      # shared by both gradients
        wgrad_mm = ctx.needs_input_grad[1] and train_ops.wgrad_mfma_ok(kh, kw, stride) and not cfg.get("fc")
        dgrad_mm = ctx.needs_input_grad[0] and _mfma_ok(kh, kw, cin, stride) and not cfg.get("fc")
        d_g8 = None
        if x_g8 is not None and wgrad_mm:
            # one scaled hi/lo conversion of d feeds both gradient kernels; x comes from the forward launch
            d_g8 = ops.to_g8(d, 0, cout, amax=d_amax)
        if ctx.needs_input_grad[1]:
            if d_g8 is not None:
                dw = train_ops.conv2d_wgrad_g8(x_g8, d_g8, kh, kw, wscale, _wgrad_prec(cfg["prec"]), None, d_amax)
            elif wgrad_mm:
                # x is the layer's forward input (an activation): split unscaled, no abs-max pass over it
                dw = train_ops.conv2d_wgrad_mfma(x, d, kh, kw, wscale, _wgrad_prec(cfg["prec"]), d_amax,
                                                 train_ops.unit_amax(x.device))
            else:
                dw = train_ops.conv2d_wgrad(x, d, kh, kw, stride, wscale)
        dx = None
        if ctx.needs_input_grad[0]:
            if dgrad_mm:
                dx = _mfma_conv(d if d_g8 is None else d_g8, _dgrad_weights(w.detach()), wscale, cfg["prec"], pad_hi=1,
                                rescale=True, amax=d_amax)
            else:
                dx = train_ops.conv2d_dgrad(d, w.detach(), (x.shape[1], x.shape[2]), stride, wscale)
        return dx, dw, db, dgamma, dbeta, None


# ----------------------------------------------------------------------------------------------
# Layers whose backward is itself differentiable (WGAN-GP: the gradient penalty of multipassGAN-8x.py
# :1123-1140 differentiates |dD/dx| with respect to the discriminator weights).  Convolution, its data
# gradient and its weight gradient are closed under differentiation:
#   y  = conv(x, w)      : dx = dgrad(dy, w)     dw = wgrad(x, dy)
#   dx = dgrad(dy, w)    : d(dy) = conv(g, w)    dw = wgrad(g, dy)
#   dw = wgrad(x, dy)    : dx = dgrad(dy, G)     d(dy) = conv(x, G)
# so three Functions that call each other give gradients of any order from the same kernels.
# ----------------------------------------------------------------------------------------------
def _conv_fwd(x, w, b, cfg):
    """x may be the autograd tensor itself (its scaled G8 form is cached on it); w, b detached"""
    kh, kw, cin, cout = w.shape
    if cfg.get("fc"):
        xd = x.detach()
        return train_ops.fc_forward(xd.reshape(xd.shape[0], cin), w.reshape(cin, cout), cfg["wscale"], b).reshape(
            xd.shape[0], 1, 1, cout)
    if _mfma_ok(kh, kw, cout, cfg["stride"]):
        if cfg.get("rescale_fwd") and x.dim() == 4:
            g8, am = _cached_g8(x, True)
            return _mfma_conv(g8, w.contiguous(), cfg["wscale"], cfg["prec"], b, rescale=True, amax=am)
        return _mfma_conv(x.detach().contiguous(), w.contiguous(), cfg["wscale"], cfg["prec"], b)
    return ops.conv2d_direct(x.detach().contiguous(), w.contiguous(), cfg["stride"], cfg["wscale"], None, b)


def _conv_dgrad(dy, w, cfg, hw):
    kh, kw, cin, cout = w.shape
    if _mfma_ok(kh, kw, cin, cfg["stride"]) and not cfg.get("fc"):
        g8, am = _cached_g8(dy, True)
        return _mfma_conv(g8, _dgrad_weights(w), cfg["wscale"], cfg["prec"], pad_hi=1, rescale=True, amax=am)
    return train_ops.conv2d_dgrad(dy.detach(), w, hw, cfg["stride"], cfg["wscale"])


def _conv_wgrad(x, dy, cfg, kh, kw):
    if train_ops.wgrad_mfma_ok(kh, kw, cfg["stride"]) and not cfg.get("fc"):
        xg, xam = _cached_g8(x, True)
        dg, dam = _cached_g8(dy, True)
        return train_ops.conv2d_wgrad_g8(xg, dg, kh, kw, cfg["wscale"], _wgrad_prec(cfg["prec"]), xam, dam)
    return train_ops.conv2d_wgrad(x.detach(), dy.detach(), kh, kw, cfg["stride"], cfg["wscale"])


class ConvFn(torch.autograd.Function):
    """y = conv2d_SAME(x, w * wscale) + b, differentiable to any order"""

    @staticmethod
    def forward(ctx, x, w, b, cfg):
        ctx.save_for_backward(x, w)
        ctx.cfg, ctx.has_bias = cfg, b is not None
        return _conv_fwd(x, w.detach(), b.detach() if b is not None else None, cfg)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = ConvDgradFn.apply(dy, w, ctx.cfg, (x.shape[1], x.shape[2])) if ctx.needs_input_grad[0] else None
        dw = ConvWgradFn.apply(x, dy, ctx.cfg, w.shape[0], w.shape[1]) if ctx.needs_input_grad[1] else None
        db = ChannelSumFn.apply(dy) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, None


class ChannelSumFn(torch.autograd.Function):
    """the bias gradient: sum of dy [..., C] over everything but the channels.  Linear: its gradient is the upstream vector
    broadcast over the pixels, a view that autograd differentiates again by itself"""

    @staticmethod
    def forward(ctx, dy):
        ctx.shape = tuple(dy.shape)
        return train_ops.channel_sum(dy.detach())

    @staticmethod
    def backward(ctx, g):
        return g.expand(ctx.shape)


class ConvDgradFn(torch.autograd.Function):
    """dx = the data gradient of conv2d_SAME(x, w * wscale) for an upstream dy, on an input of spatial size hw"""

    @staticmethod
    def forward(ctx, dy, w, cfg, hw):
        ctx.save_for_backward(dy, w)
        ctx.cfg = cfg
        return _conv_dgrad(dy, w.detach(), cfg, hw)

    @staticmethod
    def backward(ctx, g):
        dy, w = ctx.saved_tensors
        # g is a gradient of a gradient: as small as dy itself, so the forward conv over it is abs-max scaled too
        ddy = ConvFn.apply(g, w, None, dict(ctx.cfg, rescale_fwd=True)) if ctx.needs_input_grad[0] else None
        dw = ConvWgradFn.apply(g, dy, ctx.cfg, w.shape[0], w.shape[1]) if ctx.needs_input_grad[1] else None
        return ddy, dw, None, None


class ConvWgradFn(torch.autograd.Function):
    """dw = the weight gradient of conv2d_SAME(x, w * wscale) for an upstream dy.
    Known limit: backward hands its upstream gradient gw to ConvDgradFn / ConvFn as their weight, and weights are packed
    (ops.pack_conv_weights) into fp16 hi/lo without an abs-max scale: a gw of gradient magnitude (1e-6 and below) would land
    in fp16 subnormals and lose precision.  Fine for an O(1) gw, which is all the tests feed it; WGAN-GP never calls this
    rule, which takes a third derivative (the penalty differentiates dD/dx, a ConvDgradFn output, once)."""

    @staticmethod
    def forward(ctx, x, dy, cfg, kh, kw):
        ctx.save_for_backward(x, dy)
        ctx.cfg = cfg
        return _conv_wgrad(x, dy, cfg, kh, kw)

    @staticmethod
    def backward(ctx, gw):
        x, dy = ctx.saved_tensors
        dx = ConvDgradFn.apply(dy, gw, ctx.cfg, (x.shape[1], x.shape[2])) if ctx.needs_input_grad[0] else None
        ddy = ConvFn.apply(x, gw, None, ctx.cfg) if ctx.needs_input_grad[1] else None
        return dx, ddy, None, None, None


# The elementwise and resampling layers below are linear (or piecewise linear) in their input: forward runs the kernel on
# detached inputs, backward is another Function's apply, so gradients of any order come from the same kernels and one
# Function serves the first-order step and the WGAN-GP critics alike (under plain first-order training the nested apply
# records nothing).
class ActFn(torch.autograd.Function):
    """act(a [+ b]) (tf.nn.relu(tf.add(B, s)), multipassGAN-4x.py:523); act None = the plain sum"""

    @staticmethod
    def forward(ctx, a, b, act, leak):
        y = ops.add_act(a.detach().contiguous(), b.detach().contiguous() if b is not None else None, act, leak)
        ctx.save_for_backward(y)
        ctx.act, ctx.leak, ctx.two = act, leak, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        d = ActBwdFn.apply(dy, y, ctx.act, ctx.leak) if ctx.act is not None else dy
        return d, (d if ctx.two else None), None, None


class ActBwdFn(torch.autograd.Function):
    """dx = dy * act'(.) with the mask taken from the activation output: linear in dy.  relu / lrelu are piecewise linear
    (the second derivative is zero almost everywhere: nothing goes to y); tanh is not: dx = dy (1 - y^2) sends
    -2 y dy g to y (TanhBwd2Fn), for which dy is kept too"""

    @staticmethod
    def forward(ctx, dy, y, act, leak):
        if act == "tanh":
            ctx.save_for_backward(y, dy)
        else:
            ctx.save_for_backward(y)
        ctx.act, ctx.leak = act, leak
        return train_ops.act_bwd(dy.detach(), y.detach(), act, leak)

    @staticmethod
    def backward(ctx, g):
        y = ctx.saved_tensors[0]
        d_y = None
        if ctx.act == "tanh" and ctx.needs_input_grad[1]:
            d_y = TanhBwd2Fn.apply(ctx.saved_tensors[1], y, g)
        return ActBwdFn.apply(g, y, ctx.act, ctx.leak), d_y, None, None


class TanhBwd2Fn(torch.autograd.Function):
    """d_y = -2 y dy g (mpg_act_bwd2): the term of ActBwdFn's backward that goes to the tanh output.  A derivative of it
    would be a third derivative of tanh, which has no kernel: it raises instead of reading as zero"""

    @staticmethod
    def forward(ctx, dy, y, g):
        return train_ops.act_bwd2(dy.detach(), y.detach(), g.detach(), "tanh")

    @staticmethod
    def backward(ctx, gg):
        raise NotImplementedError("third-order gradient through tanh")


class AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[1], x.shape[2])
        return ops.avg_pool2(x.detach().contiguous())

    @staticmethod
    def backward(ctx, dy):
        return AvgPoolBwdFn.apply(dy, ctx.hw)


class AvgPoolBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, hw):
        return train_ops.avg_pool2_bwd(dy.detach(), *hw)

    @staticmethod
    def backward(ctx, g):
        return AvgPoolFn.apply(g), None


class ResizeNearestFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        ctx.hw = (x.shape[1], x.shape[2])
        return ops.resize_nearest(x.detach().contiguous(), oh, ow)

    @staticmethod
    def backward(ctx, dy):
        return ResizeNearestBwdFn.apply(dy, ctx.hw), None, None


class ResizeNearestBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, hw):
        ctx.ohw = (dy.shape[1], dy.shape[2])
        return train_ops.resize_nearest_bwd(dy.detach(), *hw)

    @staticmethod
    def backward(ctx, g):
        return ResizeNearestFn.apply(g, *ctx.ohw), None


class ResizeFn(torch.autograd.Function):
    """tf.image.resize_images(x, [oh, ow], method) with method 0 (bilinear) or 2 (bicubic): the upsampling inside the first
    8x generator with upsampleMode 0 / 2 (multipassGAN-8x.py:629).  Linear in x: only the shapes and the method are kept,
    and ResizeBwdFn's backward is this forward again, so the pair differentiates to any order"""
    @staticmethod
    def forward(ctx, x, oh, ow, method):
        ctx.hw, ctx.method = (x.shape[1], x.shape[2]), method
        return ops.resize_images(x.detach().contiguous(), oh, ow, method)

    @staticmethod
    def backward(ctx, dy):
        return ResizeBwdFn.apply(dy, ctx.hw, ctx.method), None, None, None


class ResizeBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, hw, method):
        ctx.ohw, ctx.method = (dy.shape[1], dy.shape[2]), method
        return train_ops.resize_bwd(dy.detach(), hw[0], hw[1], method)

    @staticmethod
    def backward(ctx, g):
        return ResizeFn.apply(g, ctx.ohw[0], ctx.ohw[1], ctx.method), None, None


class LerpFn(torch.autograd.Function):
    """lerp(x, y, t) (multipassGAN-8x.py:598-599); x may be None (tf.zeros_like).  Linear in both operands: the backward is
    made of lerps.  train_ops.lerp clamps t to [0, 1], and 1 - clamp(t) = clamp(1 - t), so t is kept as given"""

    @staticmethod
    def forward(ctx, x, y, t):
        ctx.t, ctx.has_x = float(t), x is not None
        return train_ops.lerp(x.detach() if x is not None else None, y.detach(), ctx.t)

    @staticmethod
    def backward(ctx, dy):
        dyy = LerpFn.apply(None, dy, ctx.t) if ctx.needs_input_grad[1] else None
        dx = LerpFn.apply(None, dy, 1.0 - ctx.t) if (ctx.has_x and ctx.needs_input_grad[0]) else None
        return dx, dyy, None


class BNTrain2Fn(torch.autograd.Function):
    """batch_norm(is_training=True) without its activation (GAN.py:108-110), differentiable twice; like the first-order
    path (ConvLayerFn) every evaluation advances the moving averages once"""

    @staticmethod
    def forward(ctx, lin, gamma, beta, cfg):
        mm, mv = cfg.get("moving", (None, None))
        y, mean, var = train_ops.bn_train_fwd(lin.detach(), gamma.detach(), beta.detach(), cfg["eps"], None, 0.2, mm, mv,
                                              cfg.get("decay", 0.999))
        ctx.save_for_backward(lin, gamma, mean, var)
        ctx.eps = cfg["eps"]
        return y

    @staticmethod
    def backward(ctx, dz):
        lin, gamma, mean, var = ctx.saved_tensors
        dx, dgamma, dbeta = BNTrainBwd2Fn.apply(dz, lin, gamma, mean, var, ctx.eps)
        return dx, dgamma, dbeta, None


class BNTrainBwd2Fn(torch.autograd.Function):
    """(dz, x, gamma) -> (dx, dgamma, dbeta) of the normalisation (mean, var: the forward's batch statistics, constants
    here: the formulas of mpg_bn_train_bwd2_ordered already carry their dependence on x)"""

    @staticmethod
    def forward(ctx, dz, lin, gamma, mean, var, eps):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(dz, lin, gamma, mean, var)
        ctx.eps = eps
        dx, dgamma, dbeta = train_ops.bn_train_bwd(dz.detach(), lin.detach(), mean, var, gamma.detach(), eps)
        return dx, dgamma.clone(), dbeta.clone()        # separate storages, not two views of one [2, C] buffer

    @staticmethod
    def backward(ctx, gdx, gdgamma, gdbeta):
        if gdx is None and gdgamma is None and gdbeta is None:
            return None, None, None, None, None, None
        dz, lin, gamma, mean, var = ctx.saved_tensors
        g_dz, g_x, g_gamma = train_ops.bn_train_bwd2(dz.detach(), lin.detach(), mean, var, gamma.detach(), ctx.eps,
                                                     gdx, gdgamma, gdbeta)
        return g_dz, g_x, g_gamma, None, None, None


class MinibatchStddevFn(torch.autograd.Function):
    """GAN.minibatch_stddev_layer (GAN.py:476-488), differentiable twice"""

    @staticmethod
    def forward(ctx, x, group_size):
        ctx.save_for_backward(x)
        ctx.group_size = group_size
        return ops.minibatch_stddev(x.detach().contiguous(), group_size)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return MinibatchStddevBwdFn.apply(dy, x, ctx.group_size), None


class MinibatchStddevBwdFn(torch.autograd.Function):
    """dx = dy[..., :C] + D_m u / (K G s_f): linear in dy, the statistic's second derivative in x"""

    @staticmethod
    def forward(ctx, dy, x, group_size):
        ctx.save_for_backward(dy, x)
        ctx.group_size = group_size
        return train_ops.minibatch_stddev_bwd(dy.detach(), x.detach(), group_size)

    @staticmethod
    def backward(ctx, ggx):
        dy, x = ctx.saved_tensors
        g_dy, g_x = train_ops.minibatch_stddev_bwd2(ggx, dy.detach(), x.detach(), ctx.group_size)
        return g_dy, g_x, None


class DepthToSpaceFn(torch.autograd.Function):
    """tf.depth_to_space(x, r) of GAN.pixel_shuffle (GAN.py:554-560).  Linear: its gradient is the adjoint
    space_to_depth, whose gradient is depth_to_space again, so gradients of any order use the two copy kernels."""

    @staticmethod
    def forward(ctx, x, r):
        ctx.r = r
        return ops.depth_to_space(x.detach().contiguous(), r)

    @staticmethod
    def backward(ctx, dy):
        return SpaceToDepthFn.apply(dy, ctx.r), None


class SpaceToDepthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, r):
        ctx.r = r
        return ops.space_to_depth(dy.detach().contiguous(), r)

    @staticmethod
    def backward(ctx, g):
        return DepthToSpaceFn.apply(g, ctx.r), None


def space_to_depth2(x):
    """[N,H,W,C] -> [N,H/2,W/2,4C], channel (r*2+s)*C + c holds x[2Y+r, 2X+s, c]"""
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4 * c)


def strided4_as_3x3(w):
    """The 4x4 stride-2 SAME filter of the discriminators (multipassGAN-4x.py:607-613) as a 3x3 stride-1
    filter over the space-to-depth input: y[Y,X] = sum_{a,b,r,s} z[Y+a-1, X+b-1, (r,s,c)] * W[2a+r-1, 2b+s-1, c]
    (taps outside 0..3 are zero).  With it the strided convs, their data and weight gradients all run on
    the matrix-core kernels; 16 of the 36 (a,b,r,s) positions carry weights."""
    kh, kw, c, co = w.shape
    wp = torch.nn.functional.pad(w, (0, 0, 0, 0, 1, 1, 1, 1))            # zero ring: [6,6,C,Co]
    return wp.reshape(3, 2, 3, 2, c, co).permute(0, 2, 1, 3, 4, 5).reshape(3, 3, 4 * c, co)


class MaxPoolFn(torch.autograd.Function):
    """tf.nn.max_pool VALID.  The index plane fixes a selection, so the backward is linear in dy: MaxPoolBwdFn scatters with
    it, MaxPoolGatherFn is that scatter's adjoint, and the two are each other's backward to any order (as TensorFlow's
    MaxPoolGrad / MaxPoolGradGrad, the second derivative in x is zero)"""

    @staticmethod
    def forward(ctx, x, k, s):
        x = x.contiguous()
        y, arg = ops.max_pool(x, k, s, want_arg=True)
        ctx.save_for_backward(arg)
        ctx.geom = (x.shape[1], x.shape[2], k, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        return MaxPoolBwdFn.apply(dy, arg, ctx.geom), None, None


class MaxPoolBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, arg, geom):
        ctx.save_for_backward(arg)
        ctx.geom = geom
        return train_ops.max_pool_bwd(dy.detach(), arg, *geom)

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        return MaxPoolGatherFn.apply(g, arg, ctx.geom), None, None


class MaxPoolGatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, arg, geom):
        ctx.save_for_backward(arg)
        ctx.geom = geom
        return train_ops.max_pool_gather(g.detach(), arg, geom[2], geom[3])

    @staticmethod
    def backward(ctx, d):
        (arg,) = ctx.saved_tensors
        return MaxPoolBwdFn.apply(d, arg, ctx.geom), None, None


class PixelNorm2Fn(torch.autograd.Function):
    """GAN.pixel_norm inside higher_order_scopes: the kernels of PixelNormFn, differentiable twice (the backward is
    PixelNormBwdFn); as with BNTrain2Fn the first-order Function stays what the first-order step runs"""

    @staticmethod
    def forward(ctx, x, eps):
        ctx.save_for_backward(x)            # the input itself: PixelNormBwdFn sends its second-order term back through it
        ctx.eps = eps
        return ops.pixel_norm(x.detach().contiguous(), eps)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return PixelNormBwdFn.apply(dy, x, ctx.eps), None


class PixelNormBwdFn(torch.autograd.Function):
    """dx = r dy - r^3 mean_c(x dy) x, a symmetric linear operator on dy: its derivative in dy is itself applied to g, the one
    in x is mpg_pixel_norm_bwd2.  Both are kernel calls without a tape, so a third derivative raises (once_differentiable)
    instead of reading as zero"""

    @staticmethod
    def forward(ctx, dy, x, eps):
        ctx.save_for_backward(dy, x)
        ctx.eps = eps
        return train_ops.pixel_norm_bwd(dy.detach(), x.detach(), eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dy, x = ctx.saved_tensors
        g_dy = train_ops.pixel_norm_bwd(g, x, ctx.eps) if ctx.needs_input_grad[0] else None
        g_x = train_ops.pixel_norm_bwd2(dy, x, g, ctx.eps) if ctx.needs_input_grad[1] else None
        return g_dy, g_x, None


# First-order only: a second derivative through these raises (once_differentiable) instead of reading as zero.
class PixelNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.eps = eps
        return ops.pixel_norm(x, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return train_ops.pixel_norm_bwd(dy, x, ctx.eps), None


class PairLossFn(torch.autograd.Function):
    """sum |a - b| (mode 0) / sum (a - b)^2 (mode 1) with the reduction in ``mpg_pair_reduce``; the
    backward is elementwise"""

    @staticmethod
    def forward(ctx, a, b, mode):
        ctx.save_for_backward(a, b)
        ctx.mode = mode
        return train_ops.pair_reduce(a, b, mode)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        d = a - b
        ga = (torch.sign(d) if ctx.mode == 0 else 2.0 * d) * g
        return (ga if ctx.needs_input_grad[0] else None), (-ga if ctx.needs_input_grad[1] else None), None


class ResampleFn(torch.autograd.Function):
    """tensorResample(value, pos) (multipassGAN-4x.py:398-441); pos is data, the gradient goes to value"""

    @staticmethod
    def forward(ctx, value, pos, clamp):
        ctx.save_for_backward(pos)
        ctx.clamp = clamp
        return train_ops.tensor_resample(value, pos, clamp)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (pos,) = ctx.saved_tensors
        return train_ops.tensor_resample_bwd(dy, pos, ctx.clamp), None, None


class TempoVelPackFn(torch.autograd.Function):
    """the useVelInTDisc input of the temporal critic (multipassGAN-8x.py:1204-1208): frames [3B,th,th,1] next to the
    scaled, bilinearly upsampled velocity of x_t, in the reference's [B, 12 th th] order; x_t is data, the gradient goes
    to the frames (the gradient penalty differentiates with respect to the packed tensor, never through the pack)"""

    @staticmethod
    def forward(ctx, frames, x_t, scale):
        ctx.th = frames.shape[1]
        return train_ops.tempo_vel_pack(frames, x_t, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return train_ops.tempo_vel_pack_bwd(dout, ctx.th), None, None


class TrainSession(object):
    """Eager, differentiable evaluation of ``graph`` nodes; parameters are leaf tensors keyed by
    the TF variable path.  ``run(fetches, feeds)`` returns torch tensors that carry the tape."""

    def __init__(self, variables, graph=None, prec=ops.PREC_F16X3, bn_decay=0.999, device="cuda:0", higher_order_scopes=()):
        self.graph = graph or G.get_default_graph()
        self.vars = variables
        if prec not in (ops.PREC_F16X3, ops.PREC_F16X1, ops.PREC_F16F6):
            raise _lib.MpgError("training precision %r: MPG_PREC_F16X3 (default, fp32-grade), F16X1 or F16F6" % (prec,))
        # F16F6: forward and data-gradient convolutions at the inference default where the kernels cover the shape
        # (_conv_prec); the weight gradients contract over pixels with fp16 hi/lo operands and stay at three products
        self.prec = prec
        self.bn_decay = bn_decay
        self.device = torch.device(device)
        # variable-name prefixes whose layers must support gradients of gradients (the WGAN-GP discriminators)
        self.higher_order_scopes = tuple(higher_order_scopes)
        self.params = {}
        self._scalar_feeds = {}
        self._noise_gen = {}     # random_normal node id -> its generator
        # True inside evaluation(): the reference's `train: False` feed (batch norm on its moving averages, nothing updated)
        self.eval_mode = False
        self._consumers = {}

    def parameters(self):
        """name -> leaf tensor for every variable of the graph (trainable ones require grad)"""
        self.vars.ensure(self.graph)
        for name, spec in self.graph.variables.items():
            if name not in self.params:
                t = self.vars.get(name).detach().clone().contiguous()
                t.requires_grad_(spec.kind in TRAINABLE_KINDS)
                self.params[name] = t
        return self.params

    def trainable(self, tag):
        """tf.trainable_variables() filtered like the reference: `tag in var.name` (multipassGAN-4x.py:780-784)"""
        ps = self.parameters()
        return {n: p for n, p in ps.items() if p.requires_grad and tag in n}

    def sync_to_store(self):
        for name, p in self.params.items():
            self.vars.values[name] = p.detach().clone()
        self.vars.version += 1

    @contextlib.contextmanager
    def evaluation(self):
        """the reference's `train: False` (multipassGAN-4x.py:1417, -8x.py:2100): inside, run() normalises with the moving
        averages and leaves them alone, records no tape and keeps nothing for a backward pass"""
        prev, self.eval_mode = self.eval_mode, True
        try:
            with torch.no_grad():
                yield self
        finally:
            self.eval_mode = prev

    # ------------------------------------------------------------------ evaluation
    def run(self, fetches, feeds):
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.MpgError("no GPU visible: the training step has no CPU fallback")
        self.parameters()
        env = {}
        self._scalar_feeds = {}
        for node, t in feeds.items():
            if isinstance(node, G.Scalar):
                self._scalar_feeds[node.node] = float(t)
            else:
                env[node.id] = torch.as_tensor(t, dtype=torch.float32, device=self.device)
        cons = G.consumers(fetches)
        users = {nid: len(readers) for nid, readers in cons.items()}      # a fetch counts as a reader
        self._consumers = cons if self.eval_mode else {}      # evaluation asks whether a layer's only reader takes G8
        # the UPDATE_OPS of tf.contrib.layers.batch_norm (multipassGAN-4x.py:773-776,889-899) run inside
        # mpg_bn_train_fwd_ordered: every evaluated batch-norm layer advances its moving averages once
        return [self._eval(f, env, users) for f in fetches]

    def _feeds_one_mfma_conv(self, n):
        """is the only reader of node n a stride-1 convolution of the matrix-core kernel reading it as its input?"""
        r = G.sole_reader(self._consumers, n)
        if r is None or r.op != "conv2d" or r.inputs[0] is not n:
            return False
        kh, kw, _, cout = self.graph.variables[r.inputs[1].attrs["var"]].shape
        return _mfma_ok(kh, kw, cout, tuple(r.attrs["stride"]))

    @staticmethod
    def _noise_seed(n):
        """one stream per noise node (the reference draws from TensorFlow's global generator), as session.Session does"""
        return n.attrs["seed"] if n.attrs["seed"] is not None else n.id

    def _higher(self, n):
        """does this node sit in a variable scope that needs differentiable backward passes?"""
        return any(n.scope.startswith(p) for p in self.higher_order_scopes)

    def _eval(self, n, env, users):
        if n.id in env:
            return env[n.id]
        v = self._compute(n, env, users)
        env[n.id] = v
        return v

    def _compute(self, n, env, users):
        op = n.op
        ev = lambda m: self._eval(m, env, users)   # noqa: E731
        if op == "placeholder":
            raise G.GraphError("placeholder %r was not fed" % (n,))
        if op == "variable":
            return self.params[n.attrs["var"]]
        if op in ("act", "batch_norm", "bias_add", "conv2d", "matmul"):
            # a layer [act](batch_norm?(bias_add?(conv2d|matmul))) whose inner nodes feed nothing else is one function
            chain = G.match_layer(n, lambda m: users.get(m.id, 0) == 1, ("conv2d", "matmul"))
            if chain is not None:
                return self._conv_layer(chain, ev, n)
            if op == "act":
                x = n.inputs[0]
                if x.op == "add" and users.get(x.id, 0) == 1:
                    return ActFn.apply(ev(x.inputs[0]), ev(x.inputs[1]), n.attrs["act"], n.attrs.get("leak", 0.2))
                return ActFn.apply(ev(x), None, n.attrs["act"], n.attrs.get("leak", 0.2))
            raise G.GraphError("training: no lowering for %r" % (n,))
        if op == "add":
            return ActFn.apply(ev(n.inputs[0]), ev(n.inputs[1]), None, 0.2)
        if op == "reshape":
            return ev(n.inputs[0]).reshape(n.attrs["target"])
        if op == "concat":
            return torch.cat([ev(i) for i in n.inputs], dim=-1)
        if op == "slice":
            b, s = n.attrs["begin"], n.attrs["size"]
            return ev(n.inputs[0])[..., b:b + s]
        if op == "slice_flat":
            x = ev(n.inputs[0])
            return x.reshape(x.shape[0], -1)[:, :n.attrs["count"]]
        if op == "pixel_norm":
            fn = PixelNorm2Fn if self._higher(n) else PixelNormFn
            return fn.apply(ev(n.inputs[0]), n.attrs["eps"])
        if op == "avg_pool":
            return AvgPoolFn.apply(ev(n.inputs[0]))
        if op == "lerp":
            t = n.attrs["t"]
            t = t.value(self._scalar_feeds) if isinstance(t, G.Scalar) else float(t)
            x = None if n.attrs["zero_x"] else ev(n.inputs[0])
            y = ev(n.inputs[-1])
            return LerpFn.apply(x, y, t)
        if op == "random_normal":
            return seeded_normal(self._noise_gen, n, ev(n.inputs[0]), self._noise_seed(n))
        if op == "gaussian_noise":
            # x + N(0, 1) * (s * sqrt(C)) (multipassGAN-8x.py:601-603): linear in x, so it differentiates to any order
            x = ev(n.inputs[0])
            s = n.attrs["strength"].value(self._scalar_feeds)
            if s == 0.0:
                return x
            noise = seeded_normal(self._noise_gen, n, x, self._noise_seed(n)) * (s * math.sqrt(x.shape[-1]))
            return ActFn.apply(x, noise, None, 0.2)
        if op == "max_pool":
            if self.eval_mode:                          # no argmax plane: nothing runs backward
                return ops.max_pool(ev(n.inputs[0]).contiguous(), n.attrs["k"], n.attrs["s"])
            return MaxPoolFn.apply(ev(n.inputs[0]), n.attrs["k"], n.attrs["s"])
        if op == "advect":
            src, vel = ev(n.inputs[0]), ev(n.inputs[1])
            flags = ev(n.inputs[2]) if len(n.inputs) > 2 else torch.zeros_like(src[..., :1])
            at = n.attrs
            return train_ops.advect(src, vel.detach(), flags.detach(), at["dt"], at["order"], at["strength"], at["start_bz"])
        if op == "minibatch_stddev":
            return MinibatchStddevFn.apply(ev(n.inputs[0]), n.attrs["group_size"])
        if op == "depth_to_space":
            return DepthToSpaceFn.apply(ev(n.inputs[0]), n.attrs["r"])
        if op == "resize":
            x = ev(n.inputs[0])
            if n.attrs["method"] == 1:
                return ResizeNearestFn.apply(x, n.attrs["oh"], n.attrs["ow"])
            if x.requires_grad:                         # the generator's feature maps with upsampleMode 0 / 2
                return ResizeFn.apply(x, n.attrs["oh"], n.attrs["ow"], n.attrs["method"])
            # network inputs, eval_mode, the critic's low-res condition: nothing to differentiate, no graph node
            return ops.resize_images(x.contiguous(), n.attrs["oh"], n.attrs["ow"], n.attrs["method"])
        raise G.GraphError("training: no lowering for %r" % (n,))

    def _conv_layer_eval(self, x, w4, b, bn, cfg, is_fc, top):
        """the layer with `train: False`: one forward launch, batch norm through mpg_bn_infer_act on the moving averages
        (read, never written); no G8 operand kept for a weight gradient, no batch statistics, nothing saved"""
        kh, kw, cin, cout = w4.shape
        act, leak, wscale = cfg["act"], cfg["leak"], cfg["wscale"]
        # x is kept as the object it is: the G8 form a batch-norm layer wrote travels on it (_cached_g8)
        x, w = x.contiguous(), w4.detach().contiguous()
        bd = b.detach() if b is not None else None
        conv_act = None if bn is not None else act
        if is_fc:
            lin = train_ops.fc_forward(x.reshape(x.shape[0], cin), w.reshape(cin, cout), wscale, bd, conv_act,
                                       leak).reshape(x.shape[0], 1, 1, cout)
        elif _mfma_ok(kh, kw, cout, cfg["stride"]):
            lin = _mfma_conv(x, w, wscale, cfg["prec"], bd, conv_act, leak)
        else:
            lin = ops.conv2d_direct(x, w, cfg["stride"], wscale, None, bd, conv_act, leak)
        y = lin
        if bn is not None:
            gamma, beta, mm, mv = (self.params[bn.inputs[i].attrs["var"]] for i in (1, 2, 3, 4))
            if not is_fc and self._feeds_one_mfma_conv(top):
                # the reader finds the G8 form on the tensor (_cached_g8) instead of converting y
                y, g8 = train_ops.bn_infer_act(lin, mm, mv, gamma, beta, bn.attrs["eps"], act, leak, want_g8=True)
                _attach_g8(y, g8)
            else:
                y = train_ops.bn_infer_act(lin, mm, mv, gamma, beta, bn.attrs["eps"], act, leak)
        return y.reshape(y.shape[0], -1) if is_fc else y

    def _conv_layer(self, chain, ev, chain_top=None):
        conv, bias, bn, act, leak = chain
        x = ev(conv.inputs[0])
        w = self.params[conv.inputs[1].attrs["var"]]
        b = self.params[bias.inputs[1].attrs["var"]] if bias is not None else None
        is_fc = conv.op == "matmul"
        if is_fc:
            nrow = x.shape[0]
            x = x.reshape(nrow, 1, 1, -1)
            w4 = w.reshape(1, 1, w.shape[0], w.shape[1])
            stride = (1, 1)
        else:
            w4, stride = w, tuple(conv.attrs["stride"])
            if stride == (2, 2) and tuple(w.shape[:2]) == (4, 4) and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0:
                # 4x4 stride-2 convs as 3x3 stride-1 convs over space-to-depth inputs
                x, w4, stride = space_to_depth2(x), strided4_as_3x3(w), (1, 1)
        cfg = {"stride": stride, "wscale": conv.attrs["wscale"], "act": act, "leak": leak, "prec": self.prec, "fc": is_fc,
               "eps": bn.attrs["eps"] if bn is not None else 0.0}
        if self.eval_mode:
            return self._conv_layer_eval(x, w4, b, bn, cfg, is_fc, chain_top)
        wname = conv.inputs[1].attrs["var"]
        if any(wname.startswith(p) for p in self.higher_order_scopes):
            y = ConvFn.apply(x, w4, b, cfg)
            if bn is not None:      # the tail convolutions d_cA1 / d_cB1, t_cA1 / t_cB1 with batchNorm 1 (-8x.py:850-854,910-913)
                if not bn.attrs["training"]:
                    raise G.GraphError("TrainSession needs batch_norm(training=True) nodes (build the nets with train=True)")
                bcfg = {"eps": bn.attrs["eps"], "decay": self.bn_decay,
                        "moving": (self.params[bn.inputs[3].attrs["var"]], self.params[bn.inputs[4].attrs["var"]])}
                y = BNTrain2Fn.apply(y, self.params[bn.inputs[1].attrs["var"]], self.params[bn.inputs[2].attrs["var"]], bcfg)
            if act is not None:
                y = ActFn.apply(y, None, act, leak)
            return y.reshape(y.shape[0], -1) if is_fc else y
        gamma = beta = None
        if bn is not None:
            if not bn.attrs["training"]:
                raise G.GraphError("TrainSession needs batch_norm(training=True) nodes (build the nets with train=True)")
            gamma = self.params[bn.inputs[1].attrs["var"]]
            beta = self.params[bn.inputs[2].attrs["var"]]
            cfg["moving"] = (self.params[bn.inputs[3].attrs["var"]], self.params[bn.inputs[4].attrs["var"]])
            cfg["decay"] = self.bn_decay
        y = ConvLayerFn.apply(x, w4, b, gamma, beta, cfg)
        return y.reshape(y.shape[0], -1) if is_fc else y


class AdamTF(object):
    """tf.train.AdamOptimizer(lr, beta1, beta2=0.999, epsilon=1e-8) over a set of leaf tensors, one
    flat fp32 buffer per optimiser: p -= lr_t * m / (sqrt(v) + eps) (``mpg_adam_step``)."""

    def __init__(self, params, lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, comm=None):
        self.comm = comm        # dist.Comm: gradients are averaged over the ranks before the update (one bucket)
        self.names = sorted(params)
        self.params = [params[n] for n in self.names]
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.empty(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self._grad_views = []
        with torch.no_grad():
            for _, p, sl in self._slices():
                self.flat[sl].copy_(p.reshape(-1))
                p.data = self.flat[sl].view(p.shape)       # parameters alias the flat buffer
                self._grad_views.append(self.grad[sl].view(p.shape))
        self.lr, self.b1, self.b2, self.eps, self.t = lr, beta1, beta2, eps, 0
        self.lr_t = torch.zeros(1, dtype=torch.float32, device=dev)      # read by the kernel: replayable in a graph

    def _slices(self):
        """(name, parameter, its slice of the flat buffers) for every variable, in buffer order"""
        off = 0
        for name, p in zip(self.names, self.params):
            yield name, p, slice(off, off + p.numel())
            off += p.numel()

    def _gather(self, grads):
        """grads (aligned with self.params; None = zero, as tf treats unconnected variables) into the flat gradient buffer,
        averaged over the ranks"""
        if any(g is None for g in grads):
            self.grad.zero_()
        dst = [v for v, g in zip(self._grad_views, grads) if g is not None]
        torch._foreach_copy_(dst, [g.contiguous() for g in grads if g is not None])
        if self.comm is not None:
            self.comm.all_reduce_mean(self.grad)

    def advance(self, lr=None):
        """host side of a step: t += 1 and the bias-corrected step size into device memory"""
        self.t += 1
        lr = self.lr if lr is None else lr
        self.lr_t.fill_(lr * math.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t))

    def step(self, grads, lr=None, advance=True):
        """grads: list aligned with self.params (None = zero gradient, as tf treats unconnected variables)"""
        if advance:
            self.advance(lr)
        self._gather(grads)
        train_ops.adam_step(self.flat, self.grad, self.m, self.v, self.lr_t, self.b1, self.b2, self.eps)

    def slot_state(self, tag):
        """the optimiser's slots under the names tf.train.Saver gives them (``<variable>/Adam``, ``<variable>/Adam_1``;
        the step count as TF's ``beta1_power`` = beta1^(t+1), prefixed with `tag` because every optimiser of a graph
        owns one): what a checkpoint needs so that a resumed run continues like the reference's Saver restore"""
        out = {}
        m, v = self.m.cpu().numpy(), self.v.cpu().numpy()
        for n, p_, sl in self._slices():
            out[n + "/Adam"] = m[sl].reshape(tuple(p_.shape))
            out[n + "/Adam_1"] = v[sl].reshape(tuple(p_.shape))
        out[tag + "/beta1_power"] = np.float32(self.b1 ** (self.t + 1))
        out[tag + "/adam_t"] = np.int64(self.t)
        return out

    def load_slot_state(self, state, tag):
        """inverse of slot_state; variables without slots in `state` keep theirs.  Returns the number restored."""
        hit = 0
        with torch.no_grad():
            for n, _, sl in self._slices():
                if n + "/Adam" in state and n + "/Adam_1" in state:
                    self.m[sl].copy_(torch.as_tensor(np.asarray(state[n + "/Adam"], np.float32).reshape(-1)))
                    self.v[sl].copy_(torch.as_tensor(np.asarray(state[n + "/Adam_1"], np.float32).reshape(-1)))
                    hit += 1
        if tag + "/adam_t" in state:
            self.t = int(state[tag + "/adam_t"])
        return hit


def stage_variable_names(names, stage, levels):
    """the variables stage z of the growing schedule optimises (multipassGAN-8x.py:1316-1321,1331-1336,1347-1352): all of
    them at the last stage, otherwise those whose TF name contains one of "1", "2", .., "2^(z+1)" as a substring"""
    if stage >= levels - 1:
        return list(names)
    keys = ["%i" % (2 ** i) for i in range(stage + 2)]
    return [n for n in names if any(k in n for k in keys)]


class StagedAdam(AdamTF):
    """The optimisers of one network of the 8x training graph (multipassGAN-8x.py:1305-1362): per growing stage an Adam
    with its OWN moments and step count over that stage's variable subset (a fresh one takes over at every stage change;
    `copyAdamVariables` (:1783-1802) builds assign ops it never runs and then re-initialises the new stage's slots, i.e.
    changes nothing), optional dynamic loss scaling (:490-541: the loss is multiplied by 2^ls_var, gradients by
    2^-ls_var / len(grads); a non-finite gradient skips the update and lowers ls_var by 1, an applied one raises it by
    0.0005), and for the generator the MovingAverageOptimizer shadows of each stage (:1356).
    One flat parameter buffer; the stage's subset is a 0/1 mask over it; every decision is taken on the device."""

    LS_INIT, LS_INC, LS_DEC = 64.0, 0.0005, 1.0

    def __init__(self, params, levels, lr=1e-4, beta1=0.0, beta2=0.99, eps=1e-8, comm=None, loss_scaling=False,
                 ema_decay=None):
        super().__init__(params, lr, beta1, beta2, eps, comm)
        dev = self.flat.device
        self.levels, self.loss_scaling, self.ema_decay = levels, bool(loss_scaling), ema_decay
        n = self.flat.numel()
        self.masks, self.counts = [], []
        for z in range(levels):
            chosen = set(stage_variable_names(self.names, z, levels))
            mask = torch.zeros(n, dtype=torch.float32, device=dev)
            for name, _, sl in self._slices():
                if name in chosen:
                    mask[sl] = 1.0
            self.masks.append(None if len(chosen) == len(self.names) else mask)
            self.counts.append(len(chosen))
        self.ms = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(levels)]
        self.vs = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(levels)]
        # per stage: [ls_var, coef, ok, t, lr_t, -, -, -]; ls_var is ONE variable per network in the reference (:501-503)
        self.state = [torch.zeros(8, dtype=torch.float32, device=dev) for _ in range(levels)]
        for st in self.state:
            st[0] = self.LS_INIT
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self.shadows = None
        if ema_decay is not None:       # shadows start from the variables' initial values
            self.shadows = [self.flat.detach().clone() for _ in range(levels)]
        self._last_stage = None

    def _enter(self, stage):
        """the network has ONE ls_var (:501-503): when another stage's optimiser takes over, the value moves with it"""
        stage = self.levels - 1 if stage is None else int(stage)
        if self.loss_scaling and self._last_stage is not None and stage != self._last_stage:
            self.state[stage][0] = self.state[self._last_stage][0]
        self._last_stage = stage
        return stage

    def loss_scale(self, stage):
        """2^ls_var as a device scalar (apply_loss_scaling, :506-507); None when loss scaling is off"""
        if not self.loss_scaling:
            return None
        return torch.exp(self.state[self._enter(stage)][0] * math.log(2.0))

    def step(self, grads, lr=None, stage=None):
        stage = self._enter(stage)
        if lr is not None:
            self.lr = lr
        self.lr_dev.fill_(float(self.lr))
        self._gather(grads)
        train_ops.adam_step_staged(self.flat, self.grad, self.ms[stage], self.vs[stage], self.masks[stage], self.state[stage],
                                   self.lr_dev, self.counts[stage], self.loss_scaling, self.b1, self.b2, self.eps,
                                   self.LS_INC, self.LS_DEC, None if self.shadows is None else self.shadows[stage],
                                   self.ema_decay if self.ema_decay is not None else 0.0)

    def slot_state(self, tag):
        """every stage's moments (TF uniquifies the slot names of the z-th optimiser of a variable: ``Adam_<2z>`` /
        ``Adam_<2z+1>``, the first pair without / with ``_1``), step counts and ls_var"""
        out = {}
        for z in range(self.levels):
            m, v = self.ms[z].cpu().numpy(), self.vs[z].cpu().numpy()
            chosen = set(stage_variable_names(self.names, z, self.levels))
            for n, p_, sl in self._slices():
                if n in chosen:
                    out[n + self._slot(2 * z)] = m[sl].reshape(tuple(p_.shape))
                    out[n + self._slot(2 * z + 1)] = v[sl].reshape(tuple(p_.shape))
            st = self.state[z].cpu().numpy()
            out["%s/stage%d/adam_t" % (tag, z)] = np.int64(st[3])
            out["%s/stage%d/ls_var" % (tag, z)] = np.float32(st[0])
        return out

    @staticmethod
    def _slot(i):
        return "/Adam" if i == 0 else "/Adam_%d" % i

    def load_slot_state(self, state, tag):
        hit = 0
        with torch.no_grad():
            for z in range(self.levels):
                for n, _, sl in self._slices():
                    km, kv = n + self._slot(2 * z), n + self._slot(2 * z + 1)
                    if km in state and kv in state:
                        self.ms[z][sl].copy_(torch.as_tensor(np.asarray(state[km], np.float32).reshape(-1)))
                        self.vs[z][sl].copy_(torch.as_tensor(np.asarray(state[kv], np.float32).reshape(-1)))
                        hit += 1
                if "%s/stage%d/adam_t" % (tag, z) in state:
                    self.state[z][3] = float(state["%s/stage%d/adam_t" % (tag, z)])
                    self.state[z][0] = float(state["%s/stage%d/ls_var" % (tag, z)])
        return hit

    def ema_params(self, stage=None):
        """name -> moving-average tensor of the stage's shadows (swapping_saver of the last stage's optimiser, :1369)"""
        stage = self.levels - 1 if stage is None else stage
        return {name: self.shadows[stage][sl].view(p.shape) for name, p, sl in self._slices()}


def sigmoid_ce(logits, label):
    """tf.nn.sigmoid_cross_entropy_with_logits, mean over the batch: max(x,0) - x*z + log(1+exp(-|x|))"""
    return (torch.clamp(logits, min=0) - logits * label + torch.log1p(torch.exp(-logits.abs()))).mean()


class _SlotStateMixin(object):
    """the optimiser book-keeping both trainers share; a trainer has opt_d, opt_g and, with a temporal critic, opt_t"""

    def optimisers(self):
        """-> [(tag, optimiser)] in the order the reference creates them (multipassGAN-4x.py:812-900)"""
        return [("disc", self.opt_d), ("gen", self.opt_g)] + ([("tempo", self.opt_t)] if hasattr(self, "opt_t") else [])


    def slot_state(self):
        out = {}
        for tag, o in self.optimisers():
            out.update(o.slot_state(tag))
        return out

    def load_slot_state(self, state):
        return sum(o.load_slot_state(state, tag) for tag, o in self.optimisers())


class _HeldOutMixin(object):
    """The "test model" section of the training loops (multipassGAN-4x.py:1410-1500, -8x.py:2094-2196) and the test image
    (generateTestImage, 4x.py:1050-1087, 8x.py:1539-1597) for both trainers: forward passes with `train: False`
    (TrainSession.evaluation), the means of the critic outputs from mpg_logit_stats.  A trainer supplies
    `_eval_spatial`, `_eval_tempo`, `_adv_stat` and `_sample`."""

    def evaluate(self, x, y, x_test, y_test, tempo=None, tempo_test=None, percentage=None, stage=None):
        """-> dict of device scalars, the quantities the reference's test section fetches:
          out_disc_train / out_gen_train   mean sigmoid(D(y)) / sigmoid(D(G(x))) on the train-split batch (x, y)
          out_disc_test / out_gen_test, d_loss_y, d_loss_g, g_loss_d   the same means and the losses on (x_test, y_test)
          t_out_disc_train .. t_loss_g, g_loss_t [, tl_gen_loss]   on the advected triples tempo / tempo_test =
                                            (x_t, y_t, y_pos) of a trainer with a temporal critic (tl: lambda_t_l2)
        with the losses of the configured trainer (sigmoid-CE, LSGAN or WGAN; the gradient penalty is not fetched).
        Batch norm runs on its moving averages; no parameter, moving average, optimiser slot or counter is written and
        nothing is kept for a backward pass.  `percentage` (8x) is the fed blending value; `stage` (8x) is the growing
        stage train_step runs at: no optimiser takes part here, so it is only checked to be one of the trainer's stages."""
        self._check_stage(percentage, stage)
        out = {}
        with self.sess.evaluation():
            sd, sg = self._eval_spatial(x, y, percentage)
            out["out_disc_train"], out["out_gen_train"] = sd[1], sg[1]
            sd, sg = self._eval_spatial(x_test, y_test, percentage)
            out["out_disc_test"], out["out_gen_test"] = sd[1], sg[1]
            out["d_loss_y"], out["d_loss_g"] = self._adv_stat(sd, True), self._adv_stat(sg, False)
            out["g_loss_d"] = self._adv_stat(sg, True)
            if tempo is not None and self.use_tempo:
                sd, sg, _ = self._eval_tempo(tempo, percentage)
                out["t_out_disc_train"], out["t_out_gen_train"] = sd[1], sg[1]
            if tempo_test is not None and (self.use_tempo or getattr(self, "use_tempo_l2", False)):
                sd, sg, tl = self._eval_tempo(tempo_test, percentage)
                if self.use_tempo:
                    out["t_out_disc_test"], out["t_out_gen_test"] = sd[1], sg[1]
                    out["t_loss_y"], out["t_loss_g"] = self._adv_stat(sd, True), self._adv_stat(sg, False)
                    out["g_loss_t"] = self._adv_stat(sg, True)
                if tl is not None:
                    out["tl_gen_loss"] = tl
        return out

    def _check_stage(self, percentage, stage):
        if stage is None:
            return
        levels = getattr(self, "currentUpres", None)
        if levels is None:
            raise _lib.MpgError("evaluate: this trainer has no growing stages (stage %r)" % (stage,))
        if not 0 <= int(stage) < levels:
            raise _lib.MpgError("evaluate: growing stage %d of %d" % (stage, levels))

    def sample_frame_image(self, tiCr, index, out_dir, image_no=0, sim_size_high=None, percentage=None, use_vorticity=False):
        """generateTestImage: the tiles of frame `index` (tiCr.getFrameTiles; index = (sim_no - fromSim) * frame_max +
        frame_no) through the sampler one tile at a time with `train: False`, the generator outputs assembled into the
        (sim_size_high / tileSizeHigh)^2 mosaic on the device (mpg_tiles_to_gray8) and written as
        out_dir/img_%04d.png.  use_vorticity: the low-res tiles get their three vorticity channels first (useVorticities:
        the network was built three channels wider than the tile creator's layout).  Returns the path."""
        from . import heldout, vorticity
        low, high = tiCr.getFrameTiles(index)
        th = self.tileSizeHigh
        side = (sim_size_high // th) if sim_size_high else int(round(math.sqrt(len(low))))
        if side * side != len(low):
            raise _lib.MpgError("sample_frame_image: %d tiles do not fill a %d x %d mosaic" % (len(low), side, side))
        dev = self.sess.device
        lows = torch.as_tensor(np.ascontiguousarray(low, dtype=np.float32)).to(dev)
        if use_vorticity:
            lows = vorticity.append(lows)
        lows = lows.reshape(len(low), -1)
        highs = torch.as_tensor(np.ascontiguousarray(high, dtype=np.float32)).to(dev).reshape(len(high), -1)
        tiles = []
        with self.sess.evaluation():
            for t in range(lows.shape[0]):
                tiles.append(self._sample(lows[t:t + 1], highs[t:t + 1], percentage).reshape(1, th, th, 1))
        grey = train_ops.tiles_to_gray8(torch.cat(tiles, dim=0), side, side)[0]
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "img_%04d.png" % image_no)
        heldout.write_gray_png(path, grey.cpu().numpy())
        return path


class Trainer4x(_SlotStateMixin, _HeldOutMixin):
    """The GAN training iteration of multipassGAN-4x.py (graph :728-768,880-902, loop :1317-1356):
    ``discRuns`` discriminator updates then ``genRuns`` generator updates on tile batches, spatial
    discriminator with feature losses, sigmoid cross entropy + lambda * L1 (+ lambda2 * layer loss)."""

    def __init__(self, tileSizeLow=16, upRes=4, n_inputChannels=4, batch_norm=True, upsampling_mode=2, device="cuda:0",
                 learning_rate=2e-4, beta1=0.5, lambda_l1=1.0, lambda2=0.0, lambda2_l=(1.0, 1.0, 1.0, 1.0),
                 weight_dld=1.0, bn_decay=0.999, variables=None, prec=ops.PREC_F16X3, seed=777, comm=None,
                 use_tempo=False, lambda_t=1.0, adv_flag=True, clamping=True, lambda_t_l2=0.0):
        from . import arch
        from .session import VariableStore
        self.tileSizeLow, self.upRes, self.C = tileSizeLow, upRes, n_inputChannels
        self.tileSizeHigh = tileSizeLow * upRes
        self.n_input = tileSizeLow * tileSizeLow * n_inputChannels
        if upsampling_mode in (1, 3):
            self.n_input = self.tileSizeHigh * self.tileSizeHigh * n_inputChannels
        self.n_output = self.tileSizeHigh * self.tileSizeHigh
        self.k, self.k2, self.k2_l, self.weight_dld = lambda_l1, lambda2, lambda2_l, weight_dld
        g = G.reset_default_graph()
        self.graph = g
        self.x = G.placeholder([None, self.n_input], name="x")
        self.x_disc = G.placeholder([None, self.n_input], name="x_disc")
        self.y = G.placeholder([None, self.n_output], name="y")
        self.gen_part = arch.gen_resnet(self.x, tileSizeLow, upRes, n_inputChannels, upsampling_mode=upsampling_mode,
                                        use_batch_norm=batch_norm, train=True)
        dkw = dict(tileSizeLow=tileSizeLow, upRes=upRes, n_input=self.n_input, n_inputChannels=n_inputChannels,
                   upsampling_mode=upsampling_mode, use_batch_norm=batch_norm, train=True, bn_decay=bn_decay)
        self.disc = arch.disc_binclass(self.x_disc, self.y, **dkw)
        self.gen = arch.disc_binclass(self.x_disc, self.gen_part, reuse=True, **dkw)
        # temporal discriminator (multipassGAN-4x.py:790-885): three advected frames as channels
        self.use_tempo, self.kt, self.adv_flag, self.clamping, self.n_t = use_tempo, lambda_t, adv_flag, clamping, 3
        # useTempoL2 (multipassGAN-4x.py:147-152,815-826): the l2 distance of consecutive advected generator frames
        self.ktl = float(lambda_t_l2)
        self.use_tempo_l2 = self.ktl > 1e-6
        if use_tempo or self.use_tempo_l2:
            self.x_t = G.placeholder([None, self.n_input], name="x_t")
            self.gen_part_t = arch.gen_resnet(self.x_t, tileSizeLow, upRes, n_inputChannels, upsampling_mode=upsampling_mode,
                                              reuse=True, use_batch_norm=batch_norm, train=True)
        if use_tempo:
            self.t_fake = G.placeholder([None, self.n_output * self.n_t], name="t_fake")
            self.t_real = G.placeholder([None, self.n_output * self.n_t], name="t_real")
            tk = dict(tileSizeLow=tileSizeLow, upRes=upRes, n_t_channels=self.n_t, use_batch_norm=batch_norm, train=True,
                      bn_decay=bn_decay)
            self.gen_t = arch.disc_binclass_cond_tempo(self.t_fake, reuse=False, **tk)
            self.disc_t = arch.disc_binclass_cond_tempo(self.t_real, reuse=True, **tk)
        self.sess = TrainSession(variables or VariableStore(device, seed=seed), graph=g, prec=prec, bn_decay=bn_decay,
                                 device=device)
        self.g_var = self.sess.trainable("g_")
        self.d_var = self.sess.trainable("d_")
        self.opt_d = AdamTF(self.d_var, learning_rate, beta1, comm=comm)
        self.opt_g = AdamTF(self.g_var, learning_rate, beta1, comm=comm)
        if use_tempo:
            self.t_var = {n: p for n, p in self.sess.trainable("t_").items() if n.startswith("discriminatorTempo")}
            self.opt_t = AdamTF(self.t_var, learning_rate, beta1, comm=comm)

    def set_learning_rate(self, lr):
        """the fed learning rate of all optimisers (the decayLR schedule of :773-774 is evaluated by the caller)"""
        for _, o in self.optimisers():
            o.lr = float(lr)

    def losses(self, batch_xs, batch_ys):
        """-> dict of the loss tensors of multipassGAN-4x.py:744-768 (one forward of G, D(real), D(fake))"""
        feeds = {self.x: batch_xs, self.x_disc: batch_xs, self.y: batch_ys}
        fetch = [self.gen_part] + list(self.disc) + list(self.gen)
        out = self.sess.run(fetch, feeds)
        gen_part, (disc, dy1, dy2, dy3, dy4), (gen, gy1, gy2, gy3, gy4) = out[0], out[1:6], out[6:11]
        y = torch.as_tensor(batch_ys, dtype=torch.float32, device=gen_part.device).reshape(gen_part.shape)
        ones, zeros = torch.ones_like(disc), torch.zeros_like(disc)
        L = {}
        L["disc_loss_disc"] = sigmoid_ce(disc, ones)
        L["disc_loss_gen"] = sigmoid_ce(gen, zeros)
        layer = 0.0
        for kf, a, b in zip(self.k2_l, (dy1, dy2, dy3, dy4), (gy1, gy2, gy3, gy4)):
            layer = layer + (kf * 0.5) * PairLossFn.apply(a, b, 1)   # tf.nn.l2_loss
        L["disc_loss_layer"] = layer
        L["disc_loss"] = L["disc_loss_disc"] * self.weight_dld + L["disc_loss_gen"]
        L["gen_loss"] = sigmoid_ce(gen, ones)
        L["gen_l2_loss"] = 0.5 * PairLossFn.apply(y, gen_part, 1)
        L["gen_l1_loss"] = PairLossFn.apply(y, gen_part, 0) / float(gen_part.numel())
        L["gen_loss_complete"] = L["gen_loss"] + L["gen_l1_loss"] * self.k + L["disc_loss_layer"] * self.k2
        L["gen_part"] = gen_part
        return L

    # ------------------------------------------------------------------ temporal branch
    def _frames_as_channels(self, frames, y_pos):
        """[3B, n_output] frame rows (+ look-up positions [3B, 2 n_output]) -> [B, n_output * 3]: advect every
        frame to the centre time with tensorResample when adv_flag (:801-812), then pack the n_t frames of a
        tile as channels (reshape [-1, n_t, n_output], transpose (0, 2, 1), :813-814)"""
        th = self.tileSizeHigh
        v = frames.reshape(-1, th, th, 1)
        if self.adv_flag:
            pos = torch.as_tensor(y_pos, dtype=torch.float32, device=v.device).reshape(-1, th, th, 2)
            v = ResampleFn.apply(v, pos, self.clamping)
        return v.reshape(-1, self.n_t, self.n_output).permute(0, 2, 1).reshape(-1, self.n_output * self.n_t)

    def _tempo_forward(self, batch_xts, batch_yts, batch_y_pos=None):
        """the forward passes tempo_losses and evaluate share -> (tl_gen_loss or None, D_t(fake) logits, D_t(real) logits;
        both None without a temporal critic)"""
        dev = self.sess.device
        xts = torch.as_tensor(batch_xts, dtype=torch.float32, device=dev).reshape(-1, self.n_input)
        yts = torch.as_tensor(batch_yts, dtype=torch.float32, device=dev).reshape(-1, self.n_output)
        gen_part_t = self.sess.run([self.gen_part_t], {self.x_t: xts})[0]
        fake = self._frames_as_channels(gen_part_t, batch_y_pos)
        tl = None
        if self.use_tempo_l2:
            # tl_gen_loss = sum_i mean((frame_i - frame_i+1)^2) over the n_t advected generator frames (:821-826)
            f = fake.reshape(-1, self.n_output, self.n_t)
            fr = [f[:, :, i].contiguous() for i in range(self.n_t)]
            for i in range(self.n_t - 1):
                term = PairLossFn.apply(fr[i], fr[i + 1], 1) / float(fr[i].numel())
                tl = term if tl is None else tl + term
        if not self.use_tempo:
            return tl, None, None
        real = self._frames_as_channels(yts, batch_y_pos)
        gen_t, disc_t = self.sess.run([self.gen_t, self.disc_t], {self.t_fake: fake, self.t_real: real})
        return tl, gen_t, disc_t

    def tempo_losses(self, batch_xts, batch_yts, batch_y_pos=None):
        """-> t_disc_loss, t_gen_loss (:834-866) for a coherent batch from TileCreator.selectRandomTempoTiles"""
        tl, gen_t, disc_t = self._tempo_forward(batch_xts, batch_yts, batch_y_pos)
        L = {}
        if tl is not None:
            L["tl_gen_loss"] = tl
        if not self.use_tempo:
            return L
        L["t_disc_loss_disc"] = sigmoid_ce(disc_t, torch.ones_like(disc_t))
        L["t_disc_loss_gen"] = sigmoid_ce(gen_t, torch.zeros_like(gen_t))
        L["t_disc_loss"] = L["t_disc_loss_disc"] * self.weight_dld + L["t_disc_loss_gen"]
        L["t_gen_loss"] = sigmoid_ce(gen_t, torch.ones_like(gen_t))
        return L

    def tempo_disc_step(self, batch_xts, batch_yts, batch_y_pos=None, advance=True):
        L = self.tempo_losses(batch_xts, batch_yts, batch_y_pos)
        grads = torch.autograd.grad(L["t_disc_loss"], self.opt_t.params, allow_unused=True)
        self.opt_t.step(grads, advance=advance)
        return L

    def gen_step_tempo(self, batch_xs, batch_ys, batch_xts, batch_yts, batch_y_pos=None, advance=True):
        """generator update with the temporal term: gen_loss_complete + lambda_t * t_gen_loss (:866-868,897-899)"""
        L = self.losses(batch_xs, batch_ys)
        Lt = self.tempo_losses(batch_xts, batch_yts, batch_y_pos)
        L.update(Lt)
        if self.use_tempo_l2:
            L["gen_loss_complete"] = L["gen_loss_complete"] + self.ktl * Lt["tl_gen_loss"]      # :826
        if self.use_tempo:
            L["gen_loss_complete"] = L["gen_loss_complete"] + self.kt * Lt["t_gen_loss"]          # :866
        grads = torch.autograd.grad(L["gen_loss_complete"], self.opt_g.params, allow_unused=True)
        self.opt_g.step(grads, advance=advance)
        return L

    # ------------------------------------------------------------------ held-out evaluation (_HeldOutMixin)
    def _adv_stat(self, st, real):
        """sigmoid cross entropy against label 1 / 0 out of the mpg_logit_stats vector (:744-768)"""
        return st[2] if real else st[3]

    def _eval_spatial(self, bx, by, percentage=None):
        dev = self.sess.device
        bx = torch.as_tensor(bx, dtype=torch.float32, device=dev).reshape(-1, self.n_input)
        by = torch.as_tensor(by, dtype=torch.float32, device=dev).reshape(-1, self.n_output)
        disc, gen = self.sess.run([self.disc[0], self.gen[0]], {self.x: bx, self.x_disc: bx, self.y: by})
        return train_ops.logit_stats(disc), train_ops.logit_stats(gen)

    def _eval_tempo(self, tempo, percentage=None):
        """-> (stats of D_t(real), stats of D_t(fake), tl_gen_loss or None) for a coherent batch"""
        tl, gen_t, disc_t = self._tempo_forward(*tempo)
        if not self.use_tempo:
            return None, None, tl
        return train_ops.logit_stats(disc_t), train_ops.logit_stats(gen_t), tl

    def _sample(self, low, high, percentage=None):
        return self.sess.run([self.gen_part], {self.x: low})[0]

    def disc_step(self, batch_xs, batch_ys, advance=True):
        L = self.losses(batch_xs, batch_ys)
        grads = torch.autograd.grad(L["disc_loss"], self.opt_d.params, allow_unused=True)
        self.opt_d.step(grads, advance=advance)
        return L

    def gen_step(self, batch_xs, batch_ys, advance=True):
        L = self.losses(batch_xs, batch_ys)
        grads = torch.autograd.grad(L["gen_loss_complete"], self.opt_g.params, allow_unused=True)
        self.opt_g.step(grads, advance=advance)
        return L

    def train_step_graphed(self, batch_xs, batch_ys):
        """the same iteration (discRuns = genRuns = 1) replayed from one captured hipGraph: ~1500 launches
        of the eager step become one graph launch.  Shapes are fixed by the first call; every later
        call copies the batch into the static inputs, bumps the Adam step sizes in device memory and
        replays.  Returns (disc_loss, gen_loss_complete) device scalars of the replayed iteration."""
        dev = self.opt_d.flat.device
        xs = torch.as_tensor(batch_xs, dtype=torch.float32, device=dev)
        ys = torch.as_tensor(batch_ys, dtype=torch.float32, device=dev)
        if getattr(self, "_graph", None) is None:
            self._gx, self._gy = xs.clone(), ys.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.train_step(self._gx, self._gy)        # allocator / lazy initialisation warm-up
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            self.opt_d.advance()
            self.opt_g.advance()
            with torch.cuda.graph(self._graph):
                Ld = self.disc_step(self._gx, self._gy, advance=False)
                Lg = self.gen_step(self._gx, self._gy, advance=False)
                self._gout = (Ld["disc_loss"].detach(), Lg["gen_loss_complete"].detach())
            self._graph.replay()       # capture does not execute: run the captured iteration once
            return self._gout
        if xs.shape != self._gx.shape or ys.shape != self._gy.shape:
            raise _lib.MpgError("train_step_graphed: batch shape changed after capture")
        self._gx.copy_(xs)
        self._gy.copy_(ys)
        self.opt_d.advance()
        self.opt_g.advance()
        self._graph.replay()
        return self._gout

    def train_step(self, batch_xs, batch_ys, discRuns=1, genRuns=1, tempo=None):
        """one iteration of the reference loop (:1317-1356): returns (disc_loss, gen_loss_complete) device scalars.
        tempo = (batch_xts, batch_yts, batch_y_pos) adds the temporal discriminator update and loss term."""
        for _ in range(discRuns):
            Ld = self.disc_step(batch_xs, batch_ys)
        if tempo is not None:
            for _ in range(discRuns):
                self.tempo_disc_step(*tempo)
        for _ in range(genRuns):
            Lg = self.gen_step_tempo(batch_xs, batch_ys, *tempo) if tempo is not None else self.gen_step(batch_xs, batch_ys)
        # detached: holding a loss would keep the tape (and its stream bookkeeping) alive across iterations
        return Ld["disc_loss"].detach(), Lg["gen_loss_complete"].detach()


GDROP_BETA, GDROP_LIM, GDROP_COEF, GDROP_EXP = 0.9, 0.5, 0.2, 2.0        # multipassGAN-8x.py:168-171 (gdrop_* constants)


def gdrop_schedule(score, curr_fake):
    """the end-of-iteration gDrop update (multipassGAN-8x.py:2086-2092, check_gdrop_interval 1, LSGAN only): `score` is the
    running value, `curr_fake` the mean critic output on generated data of the generator step
    -> (new score, new noise strength)"""
    score = score * GDROP_BETA + (1.0 - curr_fake) * (1.0 - GDROP_BETA)
    return score, GDROP_COEF * max(score - GDROP_LIM, 0.0) ** GDROP_EXP


class Trainer8x(_SlotStateMixin, _HeldOutMixin):
    """One stage of the progressive-growing training of multipassGAN-8x.py (graph :1023-1144, optimisers
    :1305-1362): WGAN-GP (lambda 10, target 1, epsilon penalty 1e-3) or LSGAN or sigmoid-CE losses, L1 and
    layer losses for the generator, Adam(beta1, beta2) per network, and the 0.999 moving average of the
    generator weights (tf.contrib.opt.MovingAverageOptimizer).  ``percentage`` in [0, log2(upRes)] is fed per
    step (3.0 = the final 8x stage)."""

    def __init__(self, cfg, device="cuda:0", learning_rate=1e-4, beta1=0.0, beta2=0.99, lambda_l1=1.0, lambda2=0.0,
                 k2_ls=None, weight_dld=1.0, use_wgan_gp=True, use_LSGAN=False, variables=None,
                 prec=ops.PREC_F16X3, seed=777, comm=None, ema_decay=0.999, use_tempo=False, lambda_t=1.0,
                 adv_flag=True, clamping=True, loss_scaling=False, adv_mode=0, batch_norm=False):
        from . import arch
        from .session import VariableStore
        self.cfg = cfg
        if cfg.upsampling_mode == 0:
            raise NotImplementedError("Trainer8x: training upsampling_mode 0 is not built (the faded heads need "
                                      "GAN.avg_depool(scale=[1, 2], mode=1), multipassGAN-8x.py:729-737, and the "
                                      "[tileSizeHigh, tileSizeLow] tiles of :298,378-382); the mode runs in inference only")
        self.k, self.k2, self.weight_dld = lambda_l1, lambda2, weight_dld
        self.use_wgan_gp, self.use_LSGAN = use_wgan_gp, use_LSGAN
        # `batchNorm 1` / `use_mb_stddev 1` (multipassGAN-8x.py:85,149,847,907; both 0 in the reference runs) with the WGAN-GP
        # penalty: the critic is differentiated twice through BNTrain2Fn / MinibatchStddevFn (mpg_bn_train_bwd2_ordered,
        # mpg_minibatch_stddev_bwd2)
        self.batch_norm = bool(batch_norm)
        if use_wgan_gp:
            self.wgan_lambda, self.wgan_target, self.wgan_epsilon = (150.0, 30.0, 1e-3) if use_LSGAN else (10.0, 1.0, 1e-3)
        self.currentUpres = int(round(math.log(cfg.upRes, 2)))
        # `gDrop 1` (use_gdrop, multipassGAN-8x.py:155): the strengths are fed only under use_LSGAN (:1993-2014); without it
        # the reference's discriminator step leaves the placeholder unfed and TensorFlow raises
        self.gdrop = bool(getattr(cfg, "gDrop", False))
        if self.gdrop and not use_LSGAN:
            raise _lib.MpgError("gDrop 1 needs use_LSGAN 1: the reference feeds the noise strengths only under use_LSGAN "
                                "(multipassGAN-8x.py:1993-2014)")
        # 4 channels (d, vx, vy, vz) or 7: the same with the three vorticity channels behind them (useVorticities)
        if cfg.useVelInTDisc and not (use_tempo and adv_flag and cfg.n_inputChannels in (4, 7)):
            raise _lib.MpgError("useVelInTDisc 1 needs the temporal critic, adv_flag 1 and a 4-channel low-res tile whose "
                                "channels 1..3 are the velocity (multipassGAN-8x.py:1185,1204-1208); got use_tempo %r, "
                                "adv_flag %r, %d channels" % (use_tempo, adv_flag, cfg.n_inputChannels))
        g = G.reset_default_graph()
        self.graph = g
        self.percentage = G.scalar_placeholder("percentage")
        self.gdrop_str_d = G.scalar_placeholder("gdrop_str_d") if self.gdrop else None
        self.gdrop_str_t = G.scalar_placeholder("gdrop_str_t") if self.gdrop else None
        self.x = G.placeholder([None, cfg.n_input], name="x")
        self.x_disc = G.placeholder([None, cfg.n_input], name="x_disc")
        self.y_gp = G.placeholder([None, cfg.n_output], name="y_gp")
        if cfg.upsampling_mode == 2:
            self.y2 = None
            self.y_in = G.placeholder([None, cfg.n_output], name="y_in")
            x_in = self.x
        else:       # later networks: `y` carries (target, previous pass) as two channels (:1041-1060)
            self.y2 = G.placeholder([None, cfg.n_output * 2], name="y")
            x_in, self.y_in = arch.later_network_input(self.x, self.y2, cfg)
        self.gen_y = arch.growing_gen(x_in, cfg, self.percentage, use_batch_norm=self.batch_norm, train=True,
                                      currentUpres=self.currentUpres)
        dk = dict(cfg=cfg, use_batch_norm=self.batch_norm, train=True, currentUpres=self.currentUpres)
        gd = dict(gstr=self.gdrop_str_d)
        self.disc, self.f_y = arch.growing_disc(self.y_in, self.x_disc, self.percentage, reuse=False, **dk, **gd)
        self.gen, self.f_g = arch.growing_disc(self.gen_y, self.x_disc, self.percentage, reuse=True, **dk, **gd)
        # the penalty critics pass no gstr: strength 0 (:1249,1283)
        self.d_out, _ = arch.growing_disc(self.y_gp, self.x_disc, self.percentage, reuse=True, **dk)
        self.k2_ls = list(k2_ls) if k2_ls is not None else [1.0] * len(self.f_y)
        # temporal discriminator (multipassGAN-8x.py:1158-1300; final growing stage, tensorResample advection)
        self.use_tempo, self.kt, self.adv_flag, self.clamping, self.n_t = use_tempo, lambda_t, adv_flag, clamping, 3
        # 0: tensorResample on positions computed by the tile creator; 1 / 2: GAN.advect on the low-res velocity channels
        # of x_t, semi-Lagrangian / MacCormack (:1193-1199,1221-1225)
        self.adv_mode = int(adv_mode)
        if use_tempo and adv_flag and self.adv_mode and cfg.n_inputChannels not in (4, 7):
            raise _lib.MpgError("adv_mode %d reads the velocity from channels 1..3 of a 4-channel low-res tile (:1187), "
                                "got %d channels" % (self.adv_mode, cfg.n_inputChannels))
        if use_tempo:
            self.x_t = G.placeholder([None, cfg.n_input], name="x_t")
            if cfg.upsampling_mode == 2:
                self.y_t2, x_t_in = None, self.x_t
            else:   # (:1171-1172) previous pass of the three frames = channel 1 of y_t
                self.y_t2 = G.placeholder([None, cfg.n_output * 2], name="yt")
                x_t_in, _ = arch.later_network_input(self.x_t, self.y_t2, cfg)
            self.gen_ts = arch.growing_gen(x_t_in, cfg, self.percentage, reuse=True, use_batch_norm=self.batch_norm, train=True,
                                             currentUpres=self.currentUpres)
            tk = dict(cfg=cfg, n_t_channels=self.n_t, use_batch_norm=self.batch_norm, train=True, currentUpres=self.currentUpres)
            # useVelInTDisc: every frame carries its three scaled velocity channels (:1204-1208), 12 values per pixel
            tw = cfg.n_output * (12 if cfg.useVelInTDisc else self.n_t)
            self.t_fake = G.placeholder([None, tw], name="t_fake")
            self.t_real = G.placeholder([None, tw], name="t_real")
            self.t_gp = G.placeholder([None, tw], name="t_gp")
            self.gen_s = arch.growing_disc_tempo(self.t_fake, self.percentage, reuse=False, gstr=self.gdrop_str_t, **tk)
            self.disc_s = arch.growing_disc_tempo(self.t_real, self.percentage, reuse=True, gstr=self.gdrop_str_t, **tk)
            self.t_out = arch.growing_disc_tempo(self.t_gp, self.percentage, reuse=True, **tk)
        self.sess = TrainSession(variables or VariableStore(device, seed=seed), graph=g, prec=prec, device=device)
        if use_wgan_gp:
            self.sess.higher_order_scopes = ("spatial-disc", "tempo-disc")
        self.g_var = self.sess.trainable("g_")
        self.d_var = self.sess.trainable("d_")
        lv = self.currentUpres
        self.loss_scaling = bool(loss_scaling)
        self.opt_d = StagedAdam(self.d_var, lv, learning_rate, beta1, beta2, comm=comm, loss_scaling=loss_scaling)
        self.opt_g = StagedAdam(self.g_var, lv, learning_rate, beta1, beta2, comm=comm, loss_scaling=loss_scaling,
                                ema_decay=ema_decay)
        if use_tempo:
            self.t_var = {n: p for n, p in self.sess.trainable("t_").items() if n.startswith("tempo-disc")}
            self.opt_t = StagedAdam(self.t_var, lv, learning_rate, beta1, beta2, comm=comm, loss_scaling=loss_scaling)
        self.ema_decay = ema_decay
        self.rng = torch.Generator(device="cpu").manual_seed(seed)

    # ------------------------------------------------------------------ losses
    def _adv(self, logits, real):
        """(discriminator term, generator term) of one critic output"""
        if self.use_LSGAN:
            tgt = 1.0 if real else 0.0
            return 0.5 * ((logits - tgt) ** 2).mean()
        if self.use_wgan_gp:
            return (-logits).mean() if real else logits.mean()
        return sigmoid_ce(logits, torch.ones_like(logits) if real else torch.zeros_like(logits))

    def _gdrop_feeds(self, feeds, gdrop_str_d=None, gdrop_str_t=None):
        """adds the gDrop noise strengths a run of the spatial (gdrop_str_d) / temporal (gdrop_str_t) critic reads"""
        if self.gdrop:
            if gdrop_str_d is not None:
                feeds[self.gdrop_str_d] = float(gdrop_str_d)
            if gdrop_str_t is not None:
                feeds[self.gdrop_str_t] = float(gdrop_str_t)
        return feeds

    def losses(self, batch_xs, batch_ys, percentage=3.0, lerp_factor=None, need_gp=True, gdrop_str_d=0.0):
        """-> dict of loss tensors (multipassGAN-8x.py:1082-1142); batch_ys at full tileSizeHigh resolution"""
        dev = self.sess.device
        xs = torch.as_tensor(batch_xs, dtype=torch.float32, device=dev)
        ys = torch.as_tensor(batch_ys, dtype=torch.float32, device=dev)
        if self.y2 is None:
            ys = self._to_full_res(ys)
            feeds = {self.x: xs, self.x_disc: xs, self.y_in: ys, self.percentage: percentage}
        else:
            feeds = {self.x: xs, self.x_disc: xs, self.y2: ys, self.percentage: percentage}
            ys = ys.reshape(-1, self.cfg.n_output, 2)[:, :, 0].contiguous()        # the target channel
        self._gdrop_feeds(feeds, gdrop_str_d=gdrop_str_d)
        out = self.sess.run([self.gen_y, self.disc, self.gen] + list(self.f_y) + list(self.f_g), feeds)
        nf = len(self.f_y)
        gen_y, disc, gen = out[0], out[1], out[2]
        f_y, f_g = out[3:3 + nf], out[3 + nf:3 + 2 * nf]
        L = {"gen_y": gen_y}
        layer = 0.0
        for kf, a, b in zip(self.k2_ls, f_y, f_g):
            layer = layer + (kf * 0.5) * PairLossFn.apply(a, b, 1)
        L["disc_loss_layer"] = layer
        L["d_loss_y"], L["d_loss_g"] = self._adv(disc, True), self._adv(gen, False)
        disc_loss = L["d_loss_y"] * self.weight_dld + L["d_loss_g"]
        L["gen_l2_loss"] = 0.5 * PairLossFn.apply(ys, gen_y, 1)
        L["l1_loss"] = PairLossFn.apply(ys, gen_y, 0) / float(gen_y.numel())
        L["g_loss_d"] = self._adv(gen, True)
        if self.gdrop:
            L["d_sig_g"] = gen.detach().mean()                                   # what the gDrop schedule reads (:2088)
        if self.use_wgan_gp and need_gp:
            if lerp_factor is None:
                lerp_factor = torch.rand((xs.shape[0], 1), generator=self.rng)
            lf = torch.as_tensor(lerp_factor, dtype=torch.float32, device=dev).reshape(-1, 1)
            # d(penalty)/d(generator) is never used: the discriminator step only updates d_var (:1340-1350)
            y_gp = (lf * ys + (1.0 - lf) * gen_y.detach()).requires_grad_(True)
            d_out = self.sess.run([self.d_out], {self.x_disc: xs, self.y_gp: y_gp, self.percentage: percentage})[0]
            (grads_d,) = torch.autograd.grad(d_out.mean(), y_gp, create_graph=True)
            norm = torch.sqrt(((grads_d + 1e-4) ** 2).sum(dim=1))
            L["grad_penalty_d"] = (self.wgan_lambda * (norm - self.wgan_target) ** 2).mean()
            L["epsilon_penalty_d"] = (disc ** 2).mean()
            disc_loss = disc_loss + L["epsilon_penalty_d"] * self.wgan_epsilon + L["grad_penalty_d"]
        L["disc_loss"] = disc_loss
        L["gen_loss_complete"] = L["g_loss_d"] + L["l1_loss"] * self.k + L["disc_loss_layer"] * self.k2
        return L

    def _to_full_res(self, ys):
        """targets of an earlier growing stage come at tileSizeLow * 2^stage: nearest resize to tileSizeHigh
        (tf.image.resize_images(..., method=1), multipassGAN-8x.py:1055-1058)"""
        th = self.cfg.tileSizeHigh
        if ys.shape[1] == th * th:
            return ys
        cur = int(round(math.sqrt(ys.shape[1])))
        if cur * cur != ys.shape[1] or th % cur:
            raise _lib.MpgError("targets of %d values per tile do not fit tileSizeHigh %d" % (ys.shape[1], th))
        return ops.resize_nearest(ys.reshape(-1, cur, cur, 1).contiguous(), th, th).reshape(-1, th * th)

    # ------------------------------------------------------------------ temporal branch
    def _frames_as_channels(self, frames, y_pos, xts=None, cur_size=None, percentage=None):
        """advection look-up at the CURRENT stage's resolution (the positions come at tileSizeLow * 2^stage):
        generated frames are nearest-downsampled to it, resampled, and resized back (:1178-1200).  With useVelInTDisc
        the frames leave next to upresFac * the bilinearly upsampled velocity of x_t (:1204-1208, TempoVelPackFn)"""
        th = self.cfg.tileSizeHigh
        frames = frames.reshape(frames.shape[0], -1)
        cur = int(round(math.sqrt(frames.shape[1])))
        if self.adv_flag:
            if self.adv_mode:
                tl = self.cfg.tileSizeLow
                pc = cur_size                                # currentTileSizeX (:1180-1184): the fed targets' resolution
                pos = None
            else:
                pos = torch.as_tensor(y_pos, dtype=torch.float32, device=frames.device)
                pc = int(round(math.sqrt(pos.shape[1] // 2)))
            v = frames.reshape(-1, cur, cur, 1)
            if cur != pc:                                   # generator output (full size) -> current size
                k = cur // pc
                v = v[:, ::k, ::k, :].contiguous()
            if pos is None:
                vel_t = xts.reshape(-1, tl, tl, self.cfg.n_inputChannels)[..., 1:4].contiguous()
                n = v.shape[0]                              # startBz = (batch // 3) * 3 = the rows of a tempo batch
                v = train_ops.advect(v, vel_t, torch.zeros_like(v), 0.5, self.adv_mode, 1.0, start_bz=n)
            else:
                v = ResampleFn.apply(v, pos.reshape(-1, pc, pc, 2), self.clamping)
            if pc != th:
                v = ResizeNearestFn.apply(v, th, th)
        else:
            v = self._to_full_res(frames).reshape(-1, th, th, 1)
        if self.cfg.useVelInTDisc:
            tl = self.cfg.tileSizeLow
            scale = float(2 ** int(math.ceil(percentage)))                      # upresFac (:1178)
            x4 = xts.detach().reshape(-1, tl, tl, self.cfg.n_inputChannels)[..., :4].contiguous()
            return TempoVelPackFn.apply(v.contiguous(), x4, scale)
        return v.reshape(-1, self.n_t, self.cfg.n_output).permute(0, 2, 1).reshape(-1, self.cfg.n_output * self.n_t)

    def _tempo_forward(self, batch_xts, batch_yts, batch_y_pos=None, percentage=3.0, gdrop_str_t=0.0):
        """the forward passes tempo_losses and evaluate share, for [3B, .] coherent frame rows
        -> (fake, real frames as channels, T(fake) logits, T(real) logits)"""
        dev = self.sess.device
        xts = torch.as_tensor(batch_xts, dtype=torch.float32, device=dev).reshape(-1, self.cfg.n_input)
        yts = torch.as_tensor(batch_yts, dtype=torch.float32, device=dev).reshape(xts.shape[0], -1)
        if batch_y_pos is not None and self.adv_flag and not self.adv_mode:
            batch_y_pos = torch.as_tensor(batch_y_pos, dtype=torch.float32, device=dev).reshape(xts.shape[0], -1)
        if self.y_t2 is None:
            gen_ts = self.sess.run([self.gen_ts], {self.x_t: xts, self.percentage: percentage})[0]
        else:       # rows of (target, previous pass) pairs: the real frames are channel 0 (:1218-1219)
            gen_ts = self.sess.run([self.gen_ts], {self.x_t: xts, self.y_t2: yts, self.percentage: percentage})[0]
            yts = yts.reshape(-1, self.cfg.n_output, 2)[:, :, 0].contiguous()
        # resolution of the current growing stage = that of the fed targets (tileSizeLow * 2^ceil(percentage), :1180-1181)
        cur_size = int(round(math.sqrt(yts.shape[1]))) if self.cfg.upsampling_mode == 2 else self.cfg.tileSizeHigh
        fake = self._frames_as_channels(gen_ts, batch_y_pos, xts, cur_size, percentage)
        real = self._frames_as_channels(yts, batch_y_pos, xts, cur_size, percentage)
        feeds = self._gdrop_feeds({self.t_fake: fake, self.t_real: real, self.percentage: percentage}, gdrop_str_t=gdrop_str_t)
        gen_s, disc_s = self.sess.run([self.gen_s, self.disc_s], feeds)
        return fake, real, gen_s, disc_s

    def tempo_losses(self, batch_xts, batch_yts, batch_y_pos=None, percentage=3.0, lerp_factor=None, need_gp=True,
                     gdrop_str_t=0.0):
        """t_disc_loss / g_loss_t of multipassGAN-8x.py:1216-1300 for [3B, .] coherent frame rows (final stage)"""
        dev = self.sess.device
        fake, real, gen_s, disc_s = self._tempo_forward(batch_xts, batch_yts, batch_y_pos, percentage, gdrop_str_t)
        L = {"t_loss_y": self._adv(disc_s, True), "t_loss_g": self._adv(gen_s, False)}
        t_disc_loss = L["t_loss_y"] * self.weight_dld + L["t_loss_g"]
        if self.use_wgan_gp and need_gp:
            # useVelInTDisc: t_lerp_factor is [4B, 1, 1] on the [4B, P, 3] tensor (:1281-1283), one factor per third of a row
            rows = fake.shape[0] * (4 if self.cfg.useVelInTDisc else 1)
            if lerp_factor is None:
                lerp_factor = torch.rand((rows, 1), generator=self.rng)
            lf = torch.as_tensor(lerp_factor, dtype=torch.float32, device=dev).reshape(rows, 1)
            y_gp = (lf * real.reshape(rows, -1) + (1.0 - lf) * fake.detach().reshape(rows, -1)).reshape(fake.shape)
            y_gp = y_gp.requires_grad_(True)
            t_out = self.sess.run([self.t_out], {self.t_gp: y_gp, self.percentage: percentage})[0]
            (grads_t,) = torch.autograd.grad(t_out.mean(), y_gp, create_graph=True)
            # [B, n_output, n_t] ([4B, n_output, n_t] with useVelInTDisc): the norm runs over the pixels of each frame
            # (reduce_sum(axis=1), :1287)
            gt = grads_t.reshape(-1, self.cfg.n_output, self.n_t)
            norm = torch.sqrt(((gt + 1e-4) ** 2).sum(dim=1))
            L["grad_penalty_t"] = (self.wgan_lambda * (norm - self.wgan_target) ** 2).mean()
            L["epsilon_penalty_t"] = (disc_s ** 2).mean()
            t_disc_loss = t_disc_loss + L["epsilon_penalty_t"] * self.wgan_epsilon + L["grad_penalty_t"]
        L["t_disc_loss"] = t_disc_loss
        L["g_loss_t"] = self._adv(gen_s, True)
        if self.gdrop:
            L["t_sig_g"] = gen_s.detach().mean()                                 # (:2091)
        return L

    @property
    def ema(self):
        """moving averages of the generator variables as the last stage's optimiser keeps them (the model_ema checkpoint)"""
        return list(self.opt_g.ema_params().values())

    # ------------------------------------------------------------------ held-out evaluation (_HeldOutMixin)
    @property
    def tileSizeHigh(self):
        return self.cfg.tileSizeHigh

    _eval_gdrop = (0.0, 0.0)

    def evaluate(self, x, y, x_test, y_test, tempo=None, tempo_test=None, percentage=None, stage=None, gdrop_str_d=0.0,
                 gdrop_str_t=0.0):
        """_HeldOutMixin.evaluate; gdrop_str_d / gdrop_str_t: the gDrop noise strengths the test section feeds where it
        feeds them (multipassGAN-8x.py:2086-2092), the end-of-iteration values"""
        self._eval_gdrop = (gdrop_str_d, gdrop_str_t)
        try:
            return _HeldOutMixin.evaluate(self, x, y, x_test, y_test, tempo, tempo_test, percentage, stage)
        finally:
            self._eval_gdrop = (0.0, 0.0)

    def _adv_stat(self, st, real):
        """_adv out of the mpg_logit_stats vector: LSGAN 0.5 (l - target)^2, WGAN -l / +l, else sigmoid cross entropy"""
        if self.use_LSGAN:
            return 0.5 * (st[4] if real else st[5])
        if self.use_wgan_gp:
            return -st[0] if real else st[0]
        return st[2] if real else st[3]

    def _eval_spatial(self, bx, by, percentage=None):
        dev = self.sess.device
        percentage = float(self.currentUpres) if percentage is None else percentage
        xs = torch.as_tensor(bx, dtype=torch.float32, device=dev).reshape(-1, self.cfg.n_input)
        ys = torch.as_tensor(by, dtype=torch.float32, device=dev).reshape(xs.shape[0], -1)
        if self.y2 is None:
            feeds = {self.x: xs, self.x_disc: xs, self.y_in: self._to_full_res(ys), self.percentage: percentage}
        else:
            feeds = {self.x: xs, self.x_disc: xs, self.y2: ys, self.percentage: percentage}
        disc, gen = self.sess.run([self.disc, self.gen], self._gdrop_feeds(feeds, gdrop_str_d=self._eval_gdrop[0]))
        return train_ops.logit_stats(disc), train_ops.logit_stats(gen)

    def _eval_tempo(self, tempo, percentage=None):
        """-> (stats of T(real), stats of T(fake), None) for [3B, .] coherent rows"""
        percentage = float(self.currentUpres) if percentage is None else percentage
        _, _, gen_s, disc_s = self._tempo_forward(tempo[0], tempo[1], tempo[2] if len(tempo) > 2 else None, percentage,
                                                  self._eval_gdrop[1])
        return train_ops.logit_stats(disc_s), train_ops.logit_stats(gen_s), None

    def _sample(self, low, high, percentage=None):
        """the sampler on one tile; the later networks read the previous pass from channel 1 of `high` (later_network_input)"""
        percentage = float(self.currentUpres) if percentage is None else percentage
        feeds = {self.x: low, self.percentage: percentage}
        if self.y2 is not None:
            feeds[self.y2] = high
        return self.sess.run([self.gen_y], feeds)[0]

    def _update(self, opt, loss, stage):
        """calc_gradients + apply_updates (:510-541): d(loss * 2^ls_var) for ALL of the network's variables; the stage's
        mask selects the ones its optimiser owns (unconnected ones count as zeros, :516)"""
        scale = opt.loss_scale(opt.levels - 1 if stage is None else stage)
        grads = torch.autograd.grad(loss if scale is None else loss * scale, opt.params, allow_unused=True)
        opt.step(grads, stage=stage)

    def tempo_disc_step(self, batch_xts, batch_yts, batch_y_pos=None, percentage=3.0, lerp_factor=None, stage=None,
                        gdrop_str_t=0.0):
        L = self.tempo_losses(batch_xts, batch_yts, batch_y_pos, percentage, lerp_factor, gdrop_str_t=gdrop_str_t)
        self._update(self.opt_t, L["t_disc_loss"], stage)
        return L

    def disc_step(self, batch_xs, batch_ys, percentage=3.0, lerp_factor=None, stage=None, gdrop_str_d=0.0):
        L = self.losses(batch_xs, batch_ys, percentage, lerp_factor, gdrop_str_d=gdrop_str_d)
        self._update(self.opt_d, L["disc_loss"], stage)
        return L

    def gen_step(self, batch_xs, batch_ys, percentage=3.0, tempo=None, stage=None, gdrop_str_d=0.0, gdrop_str_t=0.0):
        """the reference feeds the generator step the strengths it has just set to 0 (:2013-2014,2022-2023)"""
        L = self.losses(batch_xs, batch_ys, percentage, need_gp=False, gdrop_str_d=gdrop_str_d)
        if tempo is not None:
            Lt = self.tempo_losses(tempo[0], tempo[1], tempo[2], percentage, need_gp=False, gdrop_str_t=gdrop_str_t)
            L.update(Lt)
            L["gen_loss_complete"] = L["gen_loss_complete"] + self.kt * Lt["g_loss_t"]        # :1302
        self._update(self.opt_g, L["gen_loss_complete"], stage)     # the moving averages move inside the optimiser call
        return L

    def train_step(self, batch_xs, batch_ys, percentage=3.0, discRuns=1, genRuns=1, tempo=None, stage=None,
                   gdrop_str_d=0.0, gdrop_str_t=0.0):
        """stage: index of the growing stage's optimisers, log2(currentUpres) - 1 (:1978); None = the last one.
        gdrop_str_d / gdrop_str_t: the gDrop noise strengths of the critic steps; the generator step runs at 0 (:2013-2014)"""
        for _ in range(discRuns):
            Ld = self.disc_step(batch_xs, batch_ys, percentage, stage=stage, gdrop_str_d=gdrop_str_d)
        if tempo is not None:
            for _ in range(discRuns):
                self.tempo_disc_step(tempo[0], tempo[1], tempo[2], percentage, stage=stage, gdrop_str_t=gdrop_str_t)
        for _ in range(genRuns):
            Lg = self.gen_step(batch_xs, batch_ys, percentage, tempo, stage=stage)
        return Ld["disc_loss"].detach(), Lg["gen_loss_complete"].detach()
