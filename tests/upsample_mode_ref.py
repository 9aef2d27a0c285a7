"""Mode-aware stand-ins for oracle.train_ref8x.growing_gen / growing_disc: the float64 autograd restatement of the first 8x
network with upsampleMode 0 (legacy bilinear), 1 (nearest) or 2 (bicubic) instead of the nearest resize that oracle/ spells
out.  A test swaps them in with monkeypatch.setattr(oracle.train_ref8x, ...) for its own duration; oracle/ stays as it is.

What the option touches (arch.py:272, 348; multipassGAN-8x.py:629, 797-809):
  * growing_gen: the feature maps entering a genBlock are upsampled as R_h x R_w^T with the axis matrices of the method, read
    off oracle.ops.resize_images_tf1 on unit impulses.  The faded `old` branch stays nearest (arch.py:282) and the bicubic
    residual of the density stays as it is.
  * growing_disc: the low-res condition is resized with resize_images_tf1(..., mode)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops as O
from oracle import train_ref8x as TR8

DT = torch.float64

# The Trainer8x parity cases of test_resize_bwd_gpu.py: (upsampleMode, percentage, data seed).  The configuration is the
# make() of test_train8x_gpu.py (tile 8, C 6, batch 3, 32 feature maps, parameter seed 9, default_rng(3) data), with one
# exception.  The gradient of disc_loss with respect to spatial-disc/d_l61/bias is -1/B per real and +1/B per generated sample,
# which cancel, plus what the 1e-3 epsilon penalty leaves: -2e-3 d_loss_y.  The device forms it in float32 from partial sums
# of size 1, so it carries an absolute error of about 2^-24 whatever is left, and the per-tensor tolerance of 5e-3 can only
# be met where |d_loss_y| >= BIAS_GRADIENT_FLOOR = 2^-24 / (5e-3 * 2e-3) = 6e-3.  With default_rng(3) data at upsampleMode 0
# and percentage 2.3 the float64 reference has d_loss_y = 1.50e-3 (the critic's mean score on the targets all but vanishes;
# every other case has 1.6e-2 .. 3.9e-1), and the device's gradient, right to 2.5e-8 in absolute terms, was 8.3e-3 off in
# relative ones.  That case takes default_rng(4) data (d_loss_y = -5.9e-2); the tolerance stays.
# test_resize_bwd_host.py checks the condition for every case on the CPU.
PARITY_CASES = [(0, 3.0, 3), (0, 2.3, 4), (2, 3.0, 3), (2, 2.3, 3)]
BIAS_GRADIENT_FLOOR = 2.0 ** -24 / (5e-3 * 2e-3)
TILE, CHANNELS, BATCH = 8, 6, 3


def parity_data(data_seed):
    rng = np.random.default_rng(data_seed)
    xs = rng.random((BATCH, TILE * TILE * CHANNELS)).astype(np.float32)
    ys = rng.random((BATCH, (TILE * 8) ** 2)).astype(np.float32)
    lf = rng.random((BATCH, 1)).astype(np.float32)
    return xs, ys, lf


@functools.lru_cache(maxsize=None)
def axis_matrix(in_size, out_size, mode):
    """R [out, in] of one axis: column i is the resize of the unit impulse at i (float32 entries, as the oracle returns them)"""
    eye = np.eye(in_size, dtype=np.float32).reshape(in_size, in_size, 1, 1)          # [n = i, h = in, w = 1, c = 1]
    cols = O.resize_images_tf1(eye, out_size, 1, mode)[:, :, 0, 0]                    # [i, out]
    return torch.tensor(cols.T.astype(np.float64), dtype=DT)


def upsample2(x_nchw, mode):
    """[N, C, H, W] -> [N, C, 2H, 2W], differentiable"""
    rh = axis_matrix(x_nchw.shape[2], 2 * x_nchw.shape[2], mode)
    rw = axis_matrix(x_nchw.shape[3], 2 * x_nchw.shape[3], mode)
    return torch.einsum("ph,nchw,qw->ncpq", rh, x_nchw, rw)


def growing_gen_for(mode):
    def growing_gen(p, x_nhwc_np, percentage, first_nn_arch=True, current_upres=3, pn=True):
        x_in = torch.tensor(np.asarray(x_nhwc_np), dtype=DT).permute(0, 3, 1, 2)
        g = "generator/"
        x_g = x_in
        if not first_nn_arch:
            x_g = TR8.res_block(p, g, x_g, "1", pn=pn)
            x_g = TR8.res_block(p, g, x_g, "2", pn=pn)
        old = TR8.conv(p, g + "g_cdensOut1", x_g, None, gain=1)
        names = ["first", "second", "third", "fourth", "fifth"]
        for j in range(1, current_upres + 1):
            up = 2 ** j
            sc = g + "genBlock%d/" % up
            h = upsample2(x_g, mode)
            n_res = {2: 5, 4: 3, 8: 2}[up] if first_nn_arch else 2
            for i in range(n_res):
                h = TR8.res_block(p, sc, h, names[i], pn=pn)
            x_g = h
            dens = TR8.conv(p, sc + "g_cdensOut%d" % up, x_g, None, gain=1)
            hh = x_nhwc_np.shape[1]
            bic = O.resize_bicubic_tf1(np.asarray(x_nhwc_np[..., :1], np.float32), hh * up, hh * up)
            dens = dens + torch.tensor(bic, dtype=DT).permute(0, 3, 1, 2)
            old = TR8.lerp(TR8.up2(old), dens, percentage - (j - 1))
        return old
    return growing_gen


def growing_disc_for(mode):
    def growing_disc(p, high_nchw, low_density_np, percentage, up_res=8, current_upres=3):
        d = "spatial-disc/"
        low = np.asarray(low_density_np, np.float32)
        low = torch.tensor(O.resize_images_tf1(low, low.shape[1] * up_res, low.shape[2] * up_res, mode), dtype=DT).permute(0, 3, 1, 2)
        inp = torch.cat([low, high_nchw], dim=1)
        x = TR8.conv(p, d + "d_cfromDensity%d" % up_res, inp)
        feats = [TR8.lerp(torch.zeros_like(x), x, percentage - (current_upres - 1))]
        in_high = inp
        pooled = None
        for j in range(current_upres, 0, -1):
            in_high = F.avg_pool2d(in_high, 2)
            pooled, x1, x2 = TR8.grow_block_disc(p, d + "dBlock%d/" % (2 ** j), "d", x, 2 ** j)
            old = TR8.conv(p, d + "d_cfromDensity%d" % (2 ** (j - 1)), in_high)
            x = TR8.lerp(old, pooled, percentage - (j - 1))
            feats.append(TR8.lerp(torch.zeros_like(x1), x1, percentage - (j - 1)))
            feats.append(TR8.lerp(torch.zeros_like(x2), x2, percentage - (j - 1)))
        feats.append(TR8.lerp(torch.zeros_like(x), x, percentage))
        flat = pooled.permute(0, 2, 3, 1).reshape(pooled.shape[0], -1)
        w = p[d + "d_l61/weight"]
        score = flat @ (w * TR8._ws(w, 1.0)) + p[d + "d_l61/bias"]
        return score, feats
    return growing_disc
