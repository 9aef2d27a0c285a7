"""Timing probe of the WGAN-GP discriminator step through batch norm and minibatch stddev (run under
``rocprofv3 --kernel-trace --stats -- python tools/probe_gp_norm.py step|bn``).

  step: the second network's example size (tileSizeLow 8 -> 64^2, batch 16, startFms 192, filterSize 5, batchNorm 1,
        use_mb_stddev 1, use_wgan_gp 1): two warm-up discriminator steps, then STEPS timed ones (event timing printed)
  bn:   mpg_bn_train_bwd2_ordered at the largest shapes of tests/test_gp_norm_gpu.py, REPS calls each, with the bytes one
        call moves (reduction pass: dz, x, gdx read; elementwise pass: dz, x, gdx read, g_dz, g_x written)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, REPS = 3, 20


def step():
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(tileSizeLow=8, upRes=8, n_inputChannels=4, upsampling_mode=1, first_nn_arch=False, filterSize=5,
                start_fms=192, max_fms=192, use_mb_stddev=True)
    tr = Trainer8x(cfg, batch_norm=True, use_wgan_gp=True)
    rng = np.random.default_rng(0)
    xs = rng.random((16, 8 * 8 * 4)).astype(np.float32)
    ys = rng.random((16, 64 * 64 * 2)).astype(np.float32)
    for _ in range(2):
        tr.disc_step(xs, ys)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        L = tr.disc_step(xs, ys)
    b.record()
    torch.cuda.synchronize()
    print("gp disc step: %.3f ms/step over %d steps, disc_loss %.4f" % (a.elapsed_time(b) / STEPS, STEPS,
                                                                       float(L["disc_loss"].detach())))


def bn():
    from mpgan_amd import train_ops
    for m, c in ((16 * 128 * 128, 32), (16 * 64 * 64, 130), (16 * 128 * 128, 4)):
        g = torch.Generator(device="cuda:0").manual_seed(c)
        x, dz, gdx = (torch.randn((m, c), device="cuda:0", generator=g) for _ in range(3))
        gamma, gdg, gdb = (torch.randn((c,), device="cuda:0", generator=g) for _ in range(3))
        _, mean, var = train_ops.bn_train_fwd(x, gamma, gdb)
        train_ops.bn_train_bwd2(dz, x, mean, var, gamma, 1e-3, gdx, gdg, gdb)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            train_ops.bn_train_bwd2(dz, x, mean, var, gamma, 1e-3, gdx, gdg, gdb)
        b.record()
        torch.cuda.synchronize()
        nbytes = 4 * m * c
        print("bn_train_bwd2 M=%d C=%d: %.1f us/call (reduction reads %.1f MB, elementwise moves %.1f MB)"
              % (m, c, 1e3 * a.elapsed_time(b) / REPS, 3 * nbytes / 1e6, 5 * nbytes / 1e6))


if __name__ == "__main__":
    {"step": step, "bn": bn}[sys.argv[1] if len(sys.argv) > 1 else "step"]()
