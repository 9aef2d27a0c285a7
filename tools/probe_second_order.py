"""Times mpg_pixel_norm_bwd2 beside mpg_pixel_norm_bwd and a device-to-device copy that moves the same bytes, at
[16, 128, 128, 128] (262144 pixels of 128 channels, 134 MB a tensor): device events around every call, WARM warm-up calls and
REPS timed ones each, the three candidates interleaved call by call so that they share whatever else the machine is doing.
Bytes by the algorithm's count: the second-order kernel reads dy, x and g and writes d_x (4 tensors), the first-order one
reads dy and x and writes dx (3 tensors); the second read of the inputs, for the output, is expected from cache and is not
counted.  A copy of n bytes counts 2 n (read and written).

  python tools/probe_second_order.py [--out FILE]        prints the table in markdown; --out also writes it

For per-kernel times without launch gaps run it under `rocprofv3 --kernel-trace --stats -d <dir> --`, in a run of its own.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 20
SHAPE = (16, 128, 128, 128)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mpgan_amd  # noqa: F401
    from mpgan_amd import train_ops
    if not torch.cuda.is_available():
        raise SystemExit("probe_second_order: no GPU, nothing to measure")
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    dy, x, g = (torch.randn(SHAPE, device="cuda:0", generator=gen) for _ in range(3))
    tensor_bytes = x.numel() * 4
    src4, dst4 = torch.empty(2 * x.numel(), device="cuda:0"), torch.empty(2 * x.numel(), device="cuda:0")
    src3, dst3 = src4[:3 * x.numel() // 2], dst4[:3 * x.numel() // 2]
    src4.normal_(generator=gen)
    cands = [
        ("mpg_pixel_norm_bwd2", 4 * tensor_bytes, lambda: train_ops.pixel_norm_bwd2(dy, x, g, 1e-8)),
        ("copy of 4 tensors' bytes", 4 * tensor_bytes, lambda: dst4.copy_(src4)),
        ("mpg_pixel_norm_bwd", 3 * tensor_bytes, lambda: train_ops.pixel_norm_bwd(dy, x, 1e-8)),
        ("copy of 3 tensors' bytes", 3 * tensor_bytes, lambda: dst3.copy_(src3)),
    ]
    ms = {name: [] for name, _, _ in cands}
    for rep in range(WARM + REPS):
        for name, _, fn in cands:
            t = _timed(fn)
            if rep >= WARM:
                ms[name].append(t)
    lines = ["| call at [%d, %d, %d, %d] | bytes | ms, median (min .. max) of %d | GB/s at the median |" % (SHAPE + (REPS,)),
             "|---|---|---|---|"]
    for name, nbytes, _ in cands:
        med = statistics.median(ms[name])
        lines.append("| %s | %.1f MB | %.4f (%.4f .. %.4f) | %.0f |" % (name, nbytes / 1e6, med, min(ms[name]), max(ms[name]),
                                                                  nbytes / med / 1e6))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
