"""numpy restatement of the 8x pipeline in which nothing is zoomed along z (upsamplingMode 2 with upsampleFirst 0, then
upsamplingMode 0: multipass.plane_pass_8x / upsample_pass_8x / two_pass_8x_axis), of the mode-0 growing generator
(arch.growing_gen with Cfg8x(upsampling_mode=0), output form) and of its residual term (mpg_bicubic_cols_add), written
with the primitives of oracle.ops / oracle.nets / oracle.multipass.  float64 arithmetic on float32 inputs.

Volumes are [z, y, x, c] as stored in .uni files; the low-res array is (density, vx, vy, vz) with the velocities already
scaled by velScale.

  generator: input [N, H, L, C + 1]; optional stem (resBlock "1", "2") at [H, L]; block j = 1..3: nearest repeat of the
             COLUMNS by 2 (max_depool(1, 2)) in front of the block's units; the last block's 1x1 density head; plus the
             bicubic resize to [H, 8 L] of input channel 4 (the reference's index, multipassGAN-8x.py:721).
  pass 1:    the first generator (oracle.nets.growing_gen, first_gen) over the z_low slices as they are -> [z_low, Y, X].
  pass 2:    planes [x][y][z_low] of (pass-1 density, ALL low-res channels zoomed along y and x), channels 1 and 2 times
             upRes, channels 1 and 3 swapped: (prev, vy, vx * upRes, d * upRes, vz); the mode-0 generator; the stack
             [x][y][z] through the transposeAxis restore of multipassGAN-8x.py:1720-1725.
"""
import math

import numpy as np

from oracle import multipass as OM
from oracle import nets as ON
from oracle import ops as O

F32 = np.float32
BACK = {0: (0, 1, 2), 1: (1, 0, 2), 2: (2, 1, 0), 3: (1, 2, 0)}          # multipassGAN-8x.py:1720-1725


def bicubic_cols(plane, f):
    """[N, H, Wl] -> float64 [N, H, Wl * f]: the TF1 bicubic resize along the columns alone -- four taps of the same row,
    the table's float32 weights, summed in float64 in tap order"""
    plane = np.asarray(plane, dtype=F32)
    wl = plane.shape[2]
    ix, wx = O.bicubic_taps_tf1(wl * f, wl)
    x64 = plane.astype(np.float64)
    out = np.zeros(plane.shape[:2] + (wl * f,))
    for t in range(4):
        out += x64[:, :, ix[:, t]] * wx[:, t].astype(np.float64)[None, None, :]
    return out


def bicubic_cols_add(src, c_src, f, dens):
    """float64 [N, H, Wl * f, 1]: dens + bicubic_cols(src[..., c_src])"""
    n, h, wl, _ = src.shape
    return np.asarray(dens, dtype=F32).astype(np.float64).reshape(n, h, wl * f, 1) + bicubic_cols(src[..., c_src], f)[..., None]


def growing_gen_mode0(ps, x, up_res=8, filter_size=3, start_fms=256, max_fms=256, use_res_net=True, pixel_norm=True,
                      add_bicubic_upsample=True, prefix="generator/"):
    """growing_gen(output=True) of multipassGAN-8x.py:671-744 with upsampling_mode 0 (not first_nn_arch): x [N, H, L, C + 1]
    -> [N, H, L * up_res, 1].  gan_layer is what GAN.layer holds: max_depool resizes that (GAN.py:517)."""
    k = filter_size
    cur = int(round(math.log(up_res, 2)))
    if add_bicubic_upsample and x.shape[-1] < 5:
        raise ValueError("the residual reads input channel 4: %d channels" % x.shape[-1])
    if use_res_net:
        half = min(max_fms, start_fms // 2)
        x_g, gan_layer = ON.res_block_8x(ps, prefix, x, 16, half // 8, "1", k, pixel_norm, False)              # :693
        x_g, gan_layer = ON.res_block_8x(ps, prefix, x_g, half // 4, half // 2, "2", k, pixel_norm, False)      # :694
    else:
        x_g, _ = ON.conv_layer(ps, prefix + "g_cA1", x, 32, k, "lrelu")                                         # :696
        x_g = O.pixel_norm(x_g) if pixel_norm else x_g
        x_g, _ = ON.conv_layer(ps, prefix + "g_cB1", x_g, min(start_fms // 2, max_fms), k, "lrelu")             # :699
        x_g = O.pixel_norm(x_g) if pixel_norm else x_g
        gan_layer = x_g
    dens = None
    for j in range(1, cur + 1):
        fms = min(int(start_fms / (2 ** j)), max_fms)
        upres = 2 ** j
        scope = prefix + "genBlock%d/" % upres
        in_depool = O.max_depool(gan_layer, 1, 2)                                                               # :635
        if use_res_net:
            outp, gan_layer = ON.res_block_8x(ps, scope, in_depool, fms, fms, "first", k, pixel_norm, False)    # :655
            outp, gan_layer = ON.res_block_8x(ps, scope, outp, fms // 2, fms // 2, "second", k, pixel_norm, False)
        else:
            a, _ = ON.conv_layer(ps, scope + "g_cA%d" % upres, in_depool, fms, k, "lrelu")                      # :658
            a = O.pixel_norm(a) if pixel_norm else a
            outp, _ = ON.conv_layer(ps, scope + "g_cB%d" % upres, a, fms, k, "lrelu")                           # :661
            outp = O.pixel_norm(outp) if pixel_norm else outp
            gan_layer = outp
        if j == cur:
            dens, _ = ON.conv_layer(ps, scope + "g_cdensOut%d" % upres, outp, 1, 1, None, 1, False, gain=1.0)   # :666
            if add_bicubic_upsample:
                dens = bicubic_cols_add(x, 4, upres, dens).astype(F32)                                          # :721
    return dens


def pass1(ps, cfg, low, up_res=8, apply_cutoff=True):
    """[z_low, Y, X]: the first generator over the low-res slices as they are (multipassGAN-8x.py:1617,1633,1714)"""
    xs = np.asarray(low, dtype=F32)
    if cfg.get("add_adj", False):
        xs = OM.add_adjacent(xs, xs.shape[-1])
    out = ON.growing_gen(ps, xs, up_res, True, cfg["filter_size"], cfg["start_fms"], cfg["max_fms"],
                         cfg.get("first_nn_arch", False), cfg.get("use_res_net", True), cfg.get("pixel_norm", True))[..., 0]
    return OM.cutoff(out) if apply_cutoff else out.astype(F32)


def pass2_input(prev, low, up_res=8):
    """[X, Y, z_low, C + 1] (multipassGAN-8x.py:1615,1635-1639): plane i holds column x = i of every (z, y) -- rows y,
    columns z_low"""
    zl = low.shape[0]
    s = zl * up_res
    tile = np.asarray(low, dtype=F32)
    for ax in (1, 2):
        tile = O.zoom_axis_linear(tile, ax, up_res).astype(F32)                  # :1615, every channel
    vol = np.concatenate([np.asarray(prev, dtype=F32).reshape(zl, s, s, 1), tile], axis=3)
    xs = np.ascontiguousarray(vol.transpose(2, 1, 0, 3))                          # :1635
    xs[..., 1:3] = xs[..., 1:3] * F32(up_res)                                    # :1636
    OM.swap_channels(xs, 1, 3)                                                   # :1637-1639
    return xs


def pass2(ps, cfg, prev, low, up_res=8, transpose_axis=0, apply_cutoff=True):
    s = low.shape[0] * up_res
    out = growing_gen_mode0(ps, pass2_input(prev, low, up_res), up_res, cfg["filter_size"], cfg["start_fms"], cfg["max_fms"],
                            cfg.get("use_res_net", True), cfg.get("pixel_norm", True))[..., 0]
    out = np.ascontiguousarray(out.reshape(s, s, s).transpose(BACK[transpose_axis]))   # [x][y][z], :1716-1725
    return OM.cutoff(out) if apply_cutoff else out.astype(F32)


def two_pass(ps1, ps0, cfg1, cfg0, low, up_res=8, transpose_axis=0):
    """(final, pass-1 volume), both with the storage cutoff"""
    v1 = pass1(ps1, cfg1, low, up_res)
    return pass2(ps0, cfg0, v1, low, up_res, transpose_axis), v1
