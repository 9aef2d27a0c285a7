"""Restatements for the `useVelInTDisc` input of the 8x temporal critic (multipassGAN-8x.py:1185,1204-1208, read at :878)
and for the `gDrop` schedule (:2086-2092), shared by test_tempo_vel_host.py and test_tempo_vel_gpu.py:

* index_map(B, P): the closed form of the reference's reshape [-1, 3, P] / transpose (0, 2, 1) of the [3B, th, th, 4]
  tensor F as a permutation of flat indices;
* pack_ref(frames, x_t, scale): the literal concat / reshape / transpose over the float32 legacy bilinear resize of
  elem_ref (every operation rounded to float32, in the kernel's order);
* tempo_losses_8x_vel: float64 torch, t_disc_loss / g_loss_t with the velocity channels, on the helpers of
  oracle/train_ref8x.py; the critic is written here because the not-firstNNArch pooling critic has no restatement there.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_triad_ref as CT
import elem_ref as ER
from oracle import advect as ADV
from oracle import train_ref8x as TR8
from oracle.train_ref import tensor_resample

DT = torch.float64


# the growing blocks of the temporal critic with useVelInTDisc convolve with [filterSize + 2, filterSize] filters (:754-755):
# kh != kw with kw > 1 on ConvFn / ConvDgradFn / ConvWgradFn.  MFMA forward and data gradient; the weight gradient of a
# non-square filter runs on the one-filter-row matrix-core kernel ("row").  The 12 -> 8 case is the critic's first block
# on the 12-channel input; the ragged 9x11 image and 8x10 put the tall pad (2 rows) and the narrow one (1 column) on
# different sizes; 7x5 is filterSize 5.
TALL_CASES = [
    CT.C("5x3 16->16 9x11", 2, 9, 11, 16, 16, 5, 3, wgrad="row"),
    CT.C("5x3 12->8 8x8", 2, 8, 8, 12, 8, 5, 3, wgrad="row"),
    CT.C("7x5 8->8 8x10", 2, 8, 10, 8, 8, 7, 5, wgrad="row"),
]


# ------------------------------------------------------------------------------------------------ the permutation
def index_map(B, P):
    """-> (f, n, p, c) per output flat index o in [0, 12 B P): the flat index into F and its frame row, pixel, channel"""
    o = np.arange(12 * B * P, dtype=np.int64)
    m, q, t = o // (3 * P), (o % (3 * P)) // 3, o % 3
    f = (3 * m + t) * P + q
    return f, f // (4 * P), (f % (4 * P)) // 4, f % 4


def literal_pack(F4):
    """:1207-1208 and :878 as written: [3B, th, th, 4] -> [B, 12 P]"""
    n, th = F4.shape[0], F4.shape[1]
    P = th * th
    return np.transpose(F4.reshape(-1, 3, P), (0, 2, 1)).reshape(n // 3, 12 * P)


def pack_ref(frames, x_t, scale):
    """frames [3B, th, th, 1], x_t [3B, tl, tl, 4] float32 -> [B, 12 th th] float32 (:1185,1205-1208,:878)"""
    frames, x_t = np.asarray(frames, np.float32), np.asarray(x_t, np.float32)
    th = frames.shape[1]
    vel = np.float32(scale) * ER.resize_bilinear(x_t[..., 1:4], th, th, np.float32)
    return literal_pack(np.concatenate([frames, vel.astype(np.float32)], axis=-1))


# ------------------------------------------------------------------------------------------------ gDrop schedule
def gdrop_by_hand(curr_fakes):
    """the recurrence of :2086-2092 written out: -> [(score, strength)] after every iteration, from score 0"""
    out, score = [], 0.0
    for cf in curr_fakes:
        score = score * 0.9 + (1.0 - cf) * 0.1
        excess = score - 0.5
        out.append((score, 0.2 * excess * excess if excess > 0.0 else 0.0))
    return out


# ------------------------------------------------------------------------------------------------ float64 losses
def critic_tempo_vel(p, x_nchw, percentage, first_nn_arch, up_res=8, levels=3):
    """growing_disc_tempo of the first network on a [N, 12, H, W] input; the filter shapes come with the weights
    ([filterSize + 2, filterSize] in the blocks).  firstNNArch: the head reads the pooled x2 of the last block; otherwise
    t_cA1 / t_cB1 follow on the blended tensor and the head reads t_cB1 (:905-918)"""
    t = "tempo-disc/"
    x = TR8.conv(p, t + "t_cfromDensity%d" % up_res, x_nchw)
    in_high, pooled = x_nchw, None
    for j in range(levels, 0, -1):
        in_high = F.avg_pool2d(in_high, 2)
        pooled, _, _ = TR8.grow_block_disc(p, t + "tBlock%d/" % (2 ** j), "t", x, 2 ** j)
        old = TR8.conv(p, t + "t_cfromDensity%d" % (2 ** (j - 1)), in_high)
        x = TR8.lerp(old, pooled, percentage - (j - 1))
    if first_nn_arch:
        last = pooled
    else:
        last = TR8.conv(p, t + "t_cB1", TR8.conv(p, t + "t_cA1", x, "lrelu"))
    flat = last.permute(0, 2, 3, 1).reshape(last.shape[0], -1)
    w = p[t + "t_l61/weight"]
    return flat @ (w * TR8._ws(w, 1.0)) + p[t + "t_l61/bias"]


def tempo_losses_8x_vel(p, batch_xts, batch_yts, batch_y_pos, tile_low, percentage=3.0, lerp_factor=None,
                        wgan_lambda=10.0, wgan_target=1.0, wgan_epsilon=1e-3, weight_dld=1.0, first_nn_arch=True, adv_mode=0):
    """t_disc_loss / g_loss_t (WGAN-GP) of multipassGAN-8x.py:1178-1300 with useVelInTDisc, 4-channel low-res tiles.
    The advection runs at the current stage's size tile_low * 2^ceil(percentage) (generated frames nearest-downsampled
    to it, :1180-1200), the result is nearest-resized to tileSizeHigh and joined by upresFac * bilinear(vel_t);
    lerp_factor is [4B, 1] (:1281)"""
    th = tile_low * 8
    up_fac = 2 ** int(math.ceil(percentage))
    cur = tile_low * up_fac
    P = th * th
    xs = np.asarray(batch_xts, np.float32).reshape(-1, tile_low, tile_low, 4)
    n = xs.shape[0]
    gen_ts = TR8.growing_gen(p, xs, percentage, first_nn_arch)                  # [3B, 1, th, th]
    vel = torch.tensor(float(up_fac) * ER.resize_bilinear(xs[..., 1:4], th, th, np.float64), dtype=DT)

    def pack(frames_nhwc):
        v = frames_nhwc
        k = v.shape[1] // cur
        if k > 1:
            v = v[:, ::k, ::k, :]
        if adv_mode:
            v = ADV.advect_torch(v, xs[..., 1:4], np.zeros((n, cur, cur, 1), np.float32), 0.5, adv_mode, 1.0, n)
        else:
            v = tensor_resample(v, batch_y_pos, True)
        if cur != th:
            v = v.repeat_interleave(th // cur, 1).repeat_interleave(th // cur, 2)
        f4 = torch.cat([v, vel], dim=-1)                                        # [3B, th, th, 4]
        return f4.reshape(-1, 3, P).permute(0, 2, 1)                            # [4B, P, 3]

    fake = pack(gen_ts.permute(0, 2, 3, 1))
    real = pack(torch.tensor(np.asarray(batch_yts), dtype=DT).reshape(n, cur, cur, 1))
    to_img = lambda v: v.reshape(-1, th, th, 12).permute(0, 3, 1, 2)            # noqa: E731
    gen_s = critic_tempo_vel(p, to_img(fake), percentage, first_nn_arch)
    disc_s = critic_tempo_vel(p, to_img(real), percentage, first_nn_arch)
    t_disc_loss = (-disc_s).mean() * weight_dld + gen_s.mean()
    if lerp_factor is not None:
        lf = torch.tensor(np.asarray(lerp_factor), dtype=DT).reshape(-1, 1, 1)
        y_gp = (lf * real + (1 - lf) * fake.detach()).requires_grad_(True)
        t_out = critic_tempo_vel(p, to_img(y_gp), percentage, first_nn_arch)
        (g,) = torch.autograd.grad(t_out.mean(), y_gp, create_graph=True)
        norm = torch.sqrt(((g + 1e-4) ** 2).sum(dim=1))
        t_disc_loss = t_disc_loss + (disc_s ** 2).mean() * wgan_epsilon + (wgan_lambda * (norm - wgan_target) ** 2).mean()
    return {"t_disc_loss": t_disc_loss, "g_loss_t": (-gen_s).mean()}
