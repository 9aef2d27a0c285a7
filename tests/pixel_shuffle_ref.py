"""Restatements of the pixel-shuffle 8x generator (usePixelShuffle 1: growBlockGen of multipassGAN-out.py:239-247 and
multipassGAN-8x.py:625-633 with gan.pixel_shuffle, tools_wscale/GAN.py:554-560) built from the oracle's pieces: the numpy
output-mode network of oracle.nets and the float64 autograd training wiring of oracle.train_ref8x.  Shared by
test_pixel_shuffle_host.py and test_pixel_shuffle_gpu.py."""
import numpy as np
import torch

from oracle import nets as ON
from oracle import ops as OO
from oracle import train_ref8x as TR8

F32 = np.float32


def d2s_nhwc(x, r=2):
    """tf.depth_to_space: out[n, r h + i, r w + j, c] = x[n, h, w, (r i + j) C + c]"""
    n, h, w, c4 = x.shape
    c = c4 // (r * r)
    return x.reshape(n, h, w, r, r, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h * r, w * r, c)


def growing_gen(ps, x, up_res=8, filter_size=3, start_fms=256, max_fms=256, first_nn_arch=False, use_res_net=True,
                pixel_norm=True, upsample_mode=1, add_bicubic_upsample=True, pixel_shuffle=True, prefix="generator/"):
    """oracle.nets.growing_gen (output mode, first network) with the block's upsampling replaced by
    depth_to_space(g_cPS<2^j>(x_g), 2) when pixel_shuffle is set; nearest / bicubic depool of GAN.layer otherwise"""
    k = filter_size
    cur = int(round(np.log2(up_res)))
    gan_layer = x
    if first_nn_arch:
        x_g = x
    elif use_res_net:
        half = min(max_fms, start_fms // 2)
        x_g, gan_layer = ON.res_block_8x(ps, prefix, x, 16, half // 8, "1", k, pixel_norm, False)
        x_g, gan_layer = ON.res_block_8x(ps, prefix, x_g, half // 4, half // 2, "2", k, pixel_norm, False)
    else:
        x_g, _ = ON.conv_layer(ps, prefix + "g_cA1", x, 32, k, "lrelu", 1, False)
        if pixel_norm:
            x_g = OO.pixel_norm(x_g)
        x_g, _ = ON.conv_layer(ps, prefix + "g_cB1", x_g, min(start_fms // 2, max_fms), k, "lrelu", 1, False)
        if pixel_norm:
            x_g = OO.pixel_norm(x_g)
        gan_layer = x_g
    dens = None
    for j in range(1, cur + 1):
        fms = min(int(start_fms / (2 ** j)), max_fms)
        upres = 2 ** j
        scope = prefix + "genBlock%d/" % upres
        if pixel_shuffle:       # the shuffle reads the block input x_g (GAN.py:554-560), the depool GAN.layer
            lin, _ = ON.conv_layer(ps, scope + "g_cPS%d" % upres, x_g, 4 * x_g.shape[-1], 1, None, 1, False)
            inp = d2s_nhwc(lin)
        else:
            inp = OO.avg_depool(gan_layer, mode=upsample_mode, scale=(2,))
        if first_nn_arch:
            if upres == 2:
                names, widths = ["first", "second", "third", "fourth", "fifth"], [(fms, fms)] * 5
            elif upres == 4:
                names, widths = ["first", "second", "third"], [(fms * 2, fms), (fms, fms), (fms, fms)]
            else:
                names, widths = ["first", "second"], [(fms * 2, fms), (fms, fms)]
            outp = inp
            for nm, (s1, s2) in zip(names, widths):
                outp, gan_layer = ON.res_block_8x(ps, scope, outp, s1, s2, nm, k, pixel_norm, False)
        elif use_res_net:
            outp, gan_layer = ON.res_block_8x(ps, scope, inp, fms, fms, "first", k, pixel_norm, False)
            outp, gan_layer = ON.res_block_8x(ps, scope, outp, fms // 2, fms // 2, "second", k, pixel_norm, False)
        else:
            a, _ = ON.conv_layer(ps, scope + "g_cA%d" % upres, inp, fms, k, "lrelu", 1, False)
            if pixel_norm:
                a = OO.pixel_norm(a)
            outp, _ = ON.conv_layer(ps, scope + "g_cB%d" % upres, a, fms, k, "lrelu", 1, False)
            if pixel_norm:
                outp = OO.pixel_norm(outp)
            gan_layer = outp
        x_g = outp
        if j == cur:
            dens, _ = ON.conv_layer(ps, scope + "g_cdensOut%d" % upres, outp, 1, 1, None, 1, False, gain=1.0)
            if add_bicubic_upsample:
                dens = (dens.astype(np.float64) + OO.avg_depool(x[..., 0:1], mode=2, scale=(2 ** j,))).astype(F32)
    return dens


# ---------------------------------------------------------------------------------------------- training (float64)
def d2s_nchw(x, r=2):
    n, c4, h, w = x.shape
    c = c4 // (r * r)
    return x.reshape(n, r, r, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, h * r, w * r)


def growing_gen_train(p, x_nhwc_np, percentage, first_nn_arch=True, current_upres=3, pn=True):
    """oracle.train_ref8x.growing_gen (training wiring: density heads, fade-in) with depth_to_space(g_cPS(x_g)) in place
    of the nearest upsampling of x_g; the faded-in old head keeps its nearest upsampling (-8x.py:718-725)"""
    x_in = torch.tensor(np.asarray(x_nhwc_np), dtype=TR8.DT).permute(0, 3, 1, 2)
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
        h = d2s_nchw(TR8.conv(p, sc + "g_cPS%d" % up, x_g, None))
        n_res = {2: 5, 4: 3, 8: 2}[up] if first_nn_arch else 2
        for i in range(n_res):
            h = TR8.res_block(p, sc, h, names[i], pn=pn)
        x_g = h
        dens = TR8.conv(p, sc + "g_cdensOut%d" % up, x_g, None, gain=1)
        hh = x_nhwc_np.shape[1]
        bic = OO.resize_bicubic_tf1(np.asarray(x_nhwc_np[..., :1], np.float32), hh * up, hh * up)
        dens = dens + torch.tensor(bic, dtype=TR8.DT).permute(0, 3, 1, 2)
        old = TR8.lerp(TR8.up2(old), dens, percentage - (j - 1))
    return old


def losses_8x(p, *args, **kw):
    """oracle.train_ref8x.losses_8x with the pixel-shuffle generator"""
    keep = TR8.growing_gen
    TR8.growing_gen = growing_gen_train
    try:
        return TR8.losses_8x(p, *args, **kw)
    finally:
        TR8.growing_gen = keep
