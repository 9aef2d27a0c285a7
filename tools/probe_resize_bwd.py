"""Launches for a kernel trace of the three resize adjoints at the first 8x network's training shape: 16 tiles, 64^2 -> 128^2
at 256 channels (dy [16, 128, 128, 256], 268 MB; dx 67 MB), REPS calls each of train_ops.resize_bwd with method 1 (nearest,
resize_nearest_bwd_kernel), 0 (bilinear) and 2 (bicubic; both resize_axis_bwd_kernel, two launches a call: along H, then
along W), after one warm-up call each.  Run it under a kernel trace, in a process of its own:

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/probe_resize_bwd.py

and read the per-kernel averages from the stats file.  Without a profiler it prints event timings per call (median,
min .. max), which include the launch gaps.
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 10
N, H, OH, C = 16, 64, 128, 256


def main():
    import mpgan_amd  # noqa: F401
    from mpgan_amd import train_ops
    dy = torch.as_tensor(np.random.default_rng(1).standard_normal((N, OH, OH, C)).astype(np.float32), device="cuda:0")
    for method, name in ((1, "nearest"), (0, "bilinear"), (2, "bicubic")):
        train_ops.resize_bwd(dy, H, H, method)
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            train_ops.resize_bwd(dy, H, H, method)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        print("resize_bwd %-8s [%d,%d,%d,%d] -> [%d,%d,%d,%d]: %.3f ms (%.3f .. %.3f), events around one call" % (
            name, N, OH, OH, C, N, H, H, C, statistics.median(ms), min(ms), max(ms)))


if __name__ == "__main__":
    main()
