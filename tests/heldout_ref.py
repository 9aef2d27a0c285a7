"""Float64 restatements of the held-out evaluation quantities (Trainer4x.evaluate / Trainer8x.evaluate): the networks
of oracle/train_ref.py and oracle/train_ref8x.py called in evaluation mode, i.e. batch norm on the moving averages
(tf.contrib.layers.batch_norm(is_training=False), GAN.py:108-110), and the six means of mpg_logit_stats."""
import contextlib
import math

import numpy as np
import torch

from oracle import train_ref as TR
from oracle import train_ref8x as TR8

DT = torch.float64


def logit_stats(logits):
    """[mean l, mean sigmoid, mean CE(label 1), mean CE(label 0), mean (l-1)^2, mean l^2] in float64, the cross entropy in
    TensorFlow's form max(l,0) - l z + log1p(exp(-|l|))"""
    l = np.asarray(logits, np.float64).reshape(-1)
    soft = np.log1p(np.exp(-np.abs(l)))
    pos = np.maximum(l, 0.0)
    sig = np.where(l >= 0, 1.0 / (1.0 + np.exp(-np.abs(l))), np.exp(-np.abs(l)) / (1.0 + np.exp(-np.abs(l))))
    return np.array([l.mean(), sig.mean(), (pos - l + soft).mean(), (pos + soft).mean(), ((l - 1.0) ** 2).mean(),
                     (l * l).mean()])


@contextlib.contextmanager
def moving_average_batch_norm(enabled=True):
    """inside, oracle.train_ref.conv_layer normalises with <scope>/moving_mean and <scope>/moving_variance instead of the
    batch moments; the module is restored on exit"""
    if not enabled:
        yield
        return
    orig = TR.conv_layer

    def conv_layer(p, scope, x, act=None, stride=1, batch_norm=False, gain=math.sqrt(2.0), stats=None):
        if not batch_norm:
            return orig(p, scope, x, act, stride, False, gain, stats)
        _, lin = orig(p, scope, x, None, stride, False, gain)
        v = lambda k: p[scope + "/" + k].view(1, -1, 1, 1)       # noqa: E731
        y = (lin - v("moving_mean")) / torch.sqrt(v("moving_variance") + 1e-3) * v("gamma") + v("beta")
        if act == "relu":
            return torch.relu(y), y
        if act == "lrelu":
            return TR.lrelu(y), y
        return y, y

    TR.conv_layer = conv_layer
    try:
        yield
    finally:
        TR.conv_layer = orig


def _adv(st, real, mode):
    if mode == "lsgan":
        return 0.5 * (st[4] if real else st[5])
    if mode == "wgan":
        return -st[0] if real else st[0]
    return st[2] if real else st[3]


def _fill(out, sd, sg, split, mode, prefix=""):
    out[prefix + "out_disc_" + split], out[prefix + "out_gen_" + split] = sd[1], sg[1]
    if split == "test":
        names = ("t_loss_y", "t_loss_g", "g_loss_t") if prefix else ("d_loss_y", "d_loss_g", "g_loss_d")
        out[names[0]], out[names[1]], out[names[2]] = _adv(sd, True, mode), _adv(sg, False, mode), _adv(sg, True, mode)


def evaluate_4x(p, train, test, tile_low, up_res, channels, batch_norm=True, moving=True, tempo=None, tempo_test=None,
                tempo_l2=False, tempo_critic=True):
    """the dict of Trainer4x.evaluate in float64; moving False = batch statistics (what `train: True` would give)"""
    th = tile_low * up_res
    out = {}
    with torch.no_grad(), moving_average_batch_norm(moving):
        for split, (bx, by) in (("train", train), ("test", test)):
            x_nhwc = torch.tensor(np.asarray(bx), dtype=DT).reshape(-1, tile_low, tile_low, channels)
            y = torch.tensor(np.asarray(by), dtype=DT).reshape(-1, 1, th, th)
            gen_part = TR.gen_resnet(p, x_nhwc.permute(0, 3, 1, 2), up_res, 2, batch_norm)
            low = x_nhwc.reshape(x_nhwc.shape[0], -1)[:, :tile_low * tile_low].reshape(-1, 1, tile_low, tile_low)
            disc = TR.disc_binclass(p, low, y, up_res, batch_norm)[0]
            gen = TR.disc_binclass(p, low, gen_part, up_res, batch_norm)[0]
            _fill(out, logit_stats(disc.numpy()), logit_stats(gen.numpy()), split, "ce")
        for split, tp in (("train", tempo), ("test", tempo_test)):
            if tp is None:
                continue
            xts, yts, ypos = tp
            x = torch.tensor(np.asarray(xts), dtype=DT).reshape(-1, tile_low, tile_low, channels).permute(0, 3, 1, 2)
            gen_t = TR.gen_resnet(p, x, up_res, 2, batch_norm)

            def pack(frames_nhwc):
                v = TR.tensor_resample(frames_nhwc, ypos, True)
                v = v.reshape(-1, 3, th * th).permute(0, 2, 1)
                return v.reshape(-1, th, th, 3).permute(0, 3, 1, 2)

            fake = pack(gen_t.permute(0, 2, 3, 1))
            if tempo_critic:
                real = pack(torch.tensor(np.asarray(yts), dtype=DT).reshape(-1, th, th, 1))
                g_t, d_t = TR.disc_tempo(p, fake, batch_norm), TR.disc_tempo(p, real, batch_norm)
                _fill(out, logit_stats(d_t.numpy()), logit_stats(g_t.numpy()), split, "ce", "t_")
            if tempo_l2 and split == "test":
                fr = fake.reshape(-1, 3, th * th)
                out["tl_gen_loss"] = float(sum(torch.mean((fr[:, i] - fr[:, i + 1]) ** 2) for i in range(2)))
    return out


def evaluate_8x(p, train, test, tile_low, channels, percentage, mode="wgan", later=False):
    """the dict of Trainer8x.evaluate (spatial critic) in float64; later: the second / third network on two-channel y"""
    th = tile_low * 8
    out = {}
    with torch.no_grad():
        for split, (bx, by) in (("train", train), ("test", test)):
            xs = np.asarray(bx, np.float32).reshape(-1, tile_low, tile_low, channels)
            if later:
                gen_y, target = TR8.later_gen(p, bx, by, tile_low, channels, percentage)
                low = torch.tensor(TR8.O.resize_nearest_tf1(xs[..., :1], th, th), dtype=DT).permute(0, 3, 1, 2)
                disc = TR8.later_critic(p, "spatial-disc/", "d", torch.cat([low, target], dim=1), percentage)
                gen = TR8.later_critic(p, "spatial-disc/", "d", torch.cat([low, gen_y], dim=1), percentage)
            else:
                y = torch.tensor(np.asarray(by), dtype=DT).reshape(-1, 1, th, th)
                gen_y = TR8.growing_gen(p, xs, percentage, True)
                disc, _ = TR8.growing_disc(p, y, xs[..., :1], percentage)
                gen, _ = TR8.growing_disc(p, gen_y, xs[..., :1], percentage)
            _fill(out, logit_stats(disc.numpy()), logit_stats(gen.numpy()), split, mode)
    return out


@contextlib.contextmanager
def _recorded(module, name, keep):
    """inside, every result of module.name is appended to `keep`; the module is restored on exit"""
    orig = getattr(module, name)

    def wrapped(*a, **kw):
        out = orig(*a, **kw)
        keep.append(out)
        return out

    setattr(module, name, wrapped)
    try:
        yield
    finally:
        setattr(module, name, orig)


def tempo_logit_stats_8x(p, tempo, tile_low, channels, percentage, later=False, adv_mode=0):
    """(stats of T(real), stats of T(fake)) of the 8x temporal critic on one coherent batch: the logits are the results of
    the critic calls inside oracle.train_ref8x.tempo_losses_8x / tempo_later_nets_losses_8x (fake first, then real)"""
    xts, yts, ypos = tempo
    keep = []
    with torch.no_grad():
        if later:
            with _recorded(TR8, "later_critic", keep):
                TR8.tempo_later_nets_losses_8x(p, xts, yts, ypos, tile_low, channels, percentage, None)
        else:
            with _recorded(TR8, "growing_disc_tempo", keep):
                TR8.tempo_losses_8x(p, xts, yts, ypos, tile_low, channels, percentage, None, adv_mode=adv_mode)
    assert len(keep) == 2
    gen_s, disc_s = keep
    return logit_stats(disc_s.numpy()), logit_stats(gen_s.numpy())


def evaluate_8x_tempo(p, tempo, tempo_test, tile_low, channels, percentage, mode="wgan", later=False, adv_mode=0):
    """the temporal entries of Trainer8x.evaluate in float64"""
    out = {}
    for split, tp in (("train", tempo), ("test", tempo_test)):
        sd, sg = tempo_logit_stats_8x(p, tp, tile_low, channels, percentage, later, adv_mode)
        _fill(out, sd, sg, split, mode, "t_")
    return out


def logit_terms(logits):
    """the six per-logit terms whose means logit_stats returns, [6, n] float64"""
    l = np.asarray(logits, np.float64).reshape(-1)
    e = np.exp(-np.abs(l))
    soft, pos = np.log1p(e), np.maximum(l, 0.0)
    return np.stack([l, np.where(l >= 0, 1.0, e) / (1.0 + e), pos - l + soft, pos + soft, (l - 1.0) ** 2, l * l])
