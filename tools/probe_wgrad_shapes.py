"""development probe: mpg_conv2d_wgrad_g8 on the convolution shapes of the training steps (16 tiles), us per call; run once
per library (MPGAN_LIB_OVERRIDE) to compare two builds.  SHAPES are the square filters (ring form, F16X3); ROW_SHAPES reach
the one-filter-row kernel: the 1x1 convolutions of the training nets (arch.py: the resBlock shortcuts of the 4x generator,
the cfromDensity layers of the 8x critics) at F16X3 and F16X1, and the tall filter of the velocity critic.
usage: probe_wgrad_shapes.py [seconds timed per shape, default 0.02]"""
import sys
import torch
sys.path.insert(0, ".")
import mpgan_amd  # noqa: F401
from mpgan_amd import ops, train_ops
dev = "cuda:0"
WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 0.02
SHAPES = [  # k, cin, cout, tile
    (5, 8, 128, 256), (5, 128, 128, 256), (5, 128, 32, 256), (5, 32, 8, 256), (5, 128, 128, 64), (5, 8, 128, 64), (5, 128, 32, 64),
    (4, 32, 64, 128), (4, 64, 128, 64), (4, 128, 128, 64), (3, 64, 64, 128), (3, 128, 128, 64), (3, 32, 32, 256), (3, 256, 256, 32),
]
ROW_SHAPES = [  # kh, kw, cin, cout, tile, prec
    (1, 1, 4, 32, 64, 3), (1, 1, 32, 128, 64, 3), (1, 1, 128, 8, 64, 3), (1, 1, 8, 1, 64, 3), (1, 1, 32, 128, 256, 3),
    (1, 1, 2, 32, 128, 3), (1, 1, 32, 128, 64, 1), (1, 1, 128, 8, 64, 1), (1, 1, 32, 128, 256, 1), (1, 1, 2, 32, 128, 1),
    (5, 3, 32, 64, 64, 3),
]
out = []
for kh, kw, cin, cout, t, prec in [(k, k, ci, co, t, 3) for k, ci, co, t in SHAPES] + ROW_SHAPES:
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((16, t, t, cin), device=dev, generator=g).relu_()
    dy = torch.randn((16, t, t, cout), device=dev, generator=g) * 1e-4
    am = ops.absmax(dy)
    xg, dg = ops.to_g8(x), ops.to_g8(dy, amax=am)
    f = lambda: train_ops.conv2d_wgrad_g8(xg, dg, kh, kw, 0.025, prec, None, am)

    def timed(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(reps):
            f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    for _ in range(2):
        f()
    reps = max(8, int(WINDOW * 1e6 / timed(8)))
    out.append("%dx%d %d->%d @%d x%d: %.1f" % (kh, kw, cin, cout, t, prec, timed(reps)))
print(" | ".join(out))
