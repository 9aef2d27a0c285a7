"""Timing probe of the useVelInTDisc input of the 8x temporal critic: Trainer8x.tempo_losses with the fused pack
(mpg_tempo_vel_pack, train.TempoVelPackFn) against the same call with the unfused composition
concat(frames, scale * mpg_resize_bilinear(vel)) / reshape / transpose, and the two forms of the pack alone.

One process, the two variants alternating (A B A B ...), after warm-up of both; per variant the median with min..max of
the REPS event timings.  Shapes: the C5-style one (tileSizeLow 16 -> 128^2, startFms 256, 3 x 5 coherent rows) and
tileSizeLow 8 (-> 64^2, startFms 32, 3 x 2 rows: the size of the tests).

  python tools/probe_tempo_vel.py [out.txt]
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 9, 2


class UnfusedPack(object):
    """stands in for train.TempoVelPackFn: the composition the kernel replaces, on torch ops and mpg_resize_bilinear"""

    @staticmethod
    def apply(frames, x_t, scale):
        from mpgan_amd import ops
        th = frames.shape[1]
        vel = ops.resize_bilinear(x_t[..., 1:4].contiguous(), th, th)
        f4 = torch.cat([frames, scale * vel], -1)
        return f4.reshape(-1, 3, th * th).permute(0, 2, 1).reshape(frames.shape[0] // 3, -1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(variants):
    """variants: name -> callable; -> name -> list of REPS times (ms), taken in alternation after WARMUP calls each"""
    for _ in range(WARMUP):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(REPS):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    return times


def line(what, t):
    return "%-46s median %9.3f ms  (min %9.3f .. max %9.3f, %d reps)" % (what, statistics.median(t), min(t), max(t), len(t))


def shape(tile, fms, triples, say):
    from mpgan_amd import train
    from mpgan_amd.arch import Cfg8x
    cfg = Cfg8x(tileSizeLow=tile, upRes=8, n_inputChannels=4, start_fms=fms, max_fms=fms, useVelInTDisc=True)
    tr = train.Trainer8x(cfg, use_tempo=True, adv_mode=1, seed=3)
    rng = np.random.default_rng(0)
    n, th = 3 * triples, tile * 8
    xts = torch.as_tensor(rng.random((n, cfg.n_input)).astype(np.float32), device="cuda:0")
    yts = torch.as_tensor(rng.random((n, cfg.n_output)).astype(np.float32), device="cuda:0")
    lf = rng.random((4 * triples, 1)).astype(np.float32)
    fused = train.TempoVelPackFn

    def losses(pack):
        def run():
            train.TempoVelPackFn = pack
            try:
                return tr.tempo_losses(xts, yts, None, 3.0, lf)
            finally:
                train.TempoVelPackFn = fused
        return run

    a = float(losses(fused)()["t_disc_loss"].detach())
    b = float(losses(UnfusedPack)()["t_disc_loss"].detach())
    say("tileSizeLow %d -> %d^2, startFms %d, %d rows; t_disc_loss fused %.9g unfused %.9g (equal: %s)"
        % (tile, th, fms, n, a, b, a == b))
    t = alternate({"fused": losses(fused), "unfused": losses(UnfusedPack)})
    say(line("  tempo_losses, fused pack", t["fused"]))
    say(line("  tempo_losses, unfused composition", t["unfused"]))
    frames = torch.as_tensor(rng.random((n, th, th, 1)).astype(np.float32), device="cuda:0")
    x_t = xts.reshape(n, tile, tile, 4)
    with torch.no_grad():
        t = alternate({"fused": lambda: fused.apply(frames, x_t, 8.0), "unfused": lambda: UnfusedPack.apply(frames, x_t, 8.0)})
    moved = 4 * (frames.numel() + x_t.numel() + 12 * triples * th * th)
    say(line("  pack alone, mpg_tempo_vel_pack (%.2f MB moved)" % (moved / 1e6), t["fused"]))
    say(line("  pack alone, unfused composition", t["unfused"]))


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("useVelInTDisc pack, fused against unfused; %s; event timings, variants alternating in one process"
        % torch.cuda.get_device_name(0))
    shape(16, 256, 5, say)
    shape(8, 32, 2, say)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
