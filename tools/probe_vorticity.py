"""Vorticity input channels, timing (profiles/vorticity/timing.md).  usage: python tools/probe_vorticity.py [what]
  kernel    mpg_vorticity_append on a training batch [16,1,16,16,4], a batch of second-network tiles [48,1,128,128,4] and
            a 4x pass-2 slice batch [256,256,256,4]: three warm-up calls, ten timed ones, device events; beside it the
            host restatement of multi-pass-gan_amd/vorticity.py on the same batch (host clock, the two smaller shapes
            with the copies a device-tile batch would need: download and upload), and the kernel's byte count
            4 n h w (2c + 3) over the copy bandwidth of this machine (a device-to-device copy of 1 GiB, timed the same way)
  counters  three calls on [256,256,256,4] and nothing else: the run to put under a counter collection of its own"""
import statistics, sys, time
sys.path.insert(0, ".")
import numpy as np, torch
import mpgan_amd
from mpgan_amd import ops, vorticity

SHAPES = [(16, 1, 16, 16, 4), (48, 1, 128, 128, 4), (256, 256, 256, 4)]


def med(ts):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(ts), min(ts), max(ts))


def events(fn, warm=3, runs=10):
    ts = []
    for r in range(warm + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(a.elapsed_time(b))
    return ts


def copy_bandwidth():
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    t = statistics.median(events(lambda: dst.copy_(src)))
    return 2 * src.numel() * 4 / (t * 1e-3)          # bytes read + written per second


def kernel():
    bw = copy_bandwidth()
    print("device-to-device copy of 1 GiB: %.2f TB/s (read + written)" % (bw / 1e12))
    g = torch.Generator(device="cuda").manual_seed(1)
    for shape in SHAPES:
        x = torch.rand(shape, device="cuda", generator=g)
        c = shape[-1]
        moved = 4 * (x.numel() // c) * (2 * c + 3)
        ts = events(lambda: ops.vorticity_append(x))
        t = statistics.median(ts)
        print("%s: %.2f MB moved" % (list(shape), moved / 1e6))
        print("  kernel            %s ms: %.2f TB/s; the bytes over the copy bandwidth: %.4f ms" % (med(ts), moved / (t * 1e-3) / 1e12,
                                                                                                   moved / bw * 1e3))
        if x.numel() > (1 << 24):
            xs = x[:8].cpu().numpy()                                        # the restatement on 8 of the 256 slices, scaled
            t0 = time.perf_counter(); vorticity.append(xs); th = (time.perf_counter() - t0) * shape[0] / 8
            print("  host restatement  %.1f ms (8 slices timed, times %d)" % (th * 1e3, shape[0] // 8))
            continue
        hs, rt = [], []
        for r in range(8):
            xn = x.cpu().numpy()
            t0 = time.perf_counter(); y = vorticity.append(xn); hs.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            y = torch.as_tensor(vorticity.append(x.cpu().numpy())).cuda(); torch.cuda.synchronize()
            rt.append((time.perf_counter() - t0) * 1e3)
        print("  host restatement  %s ms; with download and upload of a device batch %s ms" % (med(hs[3:]), med(rt[3:])))
        assert torch.equal(y, ops.vorticity_append(x))


def counters():
    x = torch.rand(SHAPES[-1], device="cuda")
    for _ in range(3):
        ops.vorticity_append(x)
    torch.cuda.synchronize()


{"kernel": kernel, "counters": counters}[sys.argv[1] if len(sys.argv) > 1 else "kernel"]()
