"""Times the g_cPS layers of the C4 first network (startFms 256, firstNNArch 1, 64^2 -> 512^2 slices; j = 2: 128 -> 512
channels at 128^2, j = 3: 64 -> 256 channels at 256^2) three ways, 2 slices per call:
  fused   one mpg_conv2d_fused_d2s launch per 128 outputs (G8 out, what the planner runs)
  split   mpg_conv2d_fused per 128 outputs (fp32 out), concatenation, mpg_depth_to_space, G8 conversion for the consumer
  direct  what the planner ran before the fused store: mpg_conv2d_direct (cout > 128), mpg_depth_to_space, G8 conversion
and, for scale, the whole first network with usePixelShuffle 0 and 1.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/probe_pixel_shuffle.py` for per-kernel times; the script itself
prints CUDA-event medians."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpgan_amd  # noqa: E402,F401
from mpgan_amd import multipass as MP  # noqa: E402
from mpgan_amd import ops  # noqa: E402

DEV = "cuda:0"
REPS = int(os.environ.get("REPS", "20"))


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    res = {}
    g = torch.Generator(device=DEV).manual_seed(0)
    for j, (c, hw) in ((2, (128, 128)), (3, (64, 256))):
        x = torch.randn((2, hw, hw, c), generator=g, device=DEV)
        w = torch.randn((1, 1, c, 4 * c), generator=g, device=DEV)
        b = torch.randn((4 * c,), generator=g, device=DEV)
        xg = ops.to_g8(x)
        ws = 2 ** 0.5 / c ** 0.5
        chunks = []
        for co in range(0, 4 * c, 128):
            pk = ops.pack_conv_weights(w[..., co:co + 128].contiguous(), wscale=ws, prec=ops.PREC_F16X3)
            chunks.append(([ops.Segment(xg, pk)], co))

        def fused():
            return ops.conv2d_fused_d2s(chunks, (hw, hw), 4 * c, bias=b, want_f32=False, want_g8=True)

        def split():
            ys = [ops.conv2d_fused(s, (hw, hw), bias=b[co:co + 128].contiguous()) for s, co in chunks]
            return ops.to_g8(ops.depth_to_space(torch.cat(ys, dim=3).contiguous(), 2))

        def direct():
            return ops.to_g8(ops.depth_to_space(ops.conv2d_direct(x, w, (1, 1), ws, None, b), 2))

        ref = ops.from_g8(split())
        assert torch.equal(ops.from_g8(fused()), ref)
        res["g_cPS%d" % 2 ** j] = {k: round(timed(f), 1) for k, f in (("fused_us", fused), ("split_us", split),
                                                                       ("direct_us", direct))}
    cfg = dict(tile_low=64, up_res=8, channels=4, first_gen=True, filter_size=3, start_fms=256, max_fms=256,
               first_nn_arch=True)
    xin = torch.rand((2, 64, 64, 4), generator=g, device=DEV)
    for flag in (False, True):
        gen = MP.Generator("growing_gen", dict(cfg, pixel_shuffle=flag), None, None, device=DEV)
        res["network_pixel_shuffle_%d_us" % flag] = round(timed(lambda: gen(xin), 10), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
