"""8x upsamplingMode 0, timing (profiles/mode0_8x/timing.md).  usage: python tools/probe_mode0_8x.py [what] [sim]
  kernel    mpg_bicubic_cols_add at factor 8 on a batch of two planes [2,512,64,5] and on the planes of a whole volume
            [512,512,64,5]: three warm-up calls, ten timed ones, device events; beside it the unfused composition (channel
            slice, mpg_resize_bicubic, mpg_add_act) on the same tensors, both as GB/s of the fused kernel's byte count
            4 (2 + c / f) per output pixel, and that count over the copy bandwidth of this machine (a device-to-device copy
            of 1 GiB, timed the same way, as tools/probe_vorticity.py does)
  volume    seconds per sim^3 -> (8 sim)^3 volume (sim 64 unless given) in one process, one warm-up volume and three timed
            ones (host clock around a synchronised call), the same synthetic weights and prec in both pairs:
              axis pair   upsamplingMode 2 with upsampleFirst 0 (sim slices), then upsamplingMode 0 (8 sim planes of 8 sim x sim)
              zoom pair   upsamplingMode 2 on the volume zoomed along z (8 sim slices), then upsamplingMode 1 (8 sim slices
                          of (8 sim)^2)
            first network: startFms 256, maxFms 256, firstNNArch, add_adj_idcs; second: startFms 512, maxFms 256, filter 3"""
import statistics, sys, time
sys.path.insert(0, ".")
import torch
import mpgan_amd
from mpgan_amd import multipass as MP, ops
from mpgan_amd.synthetic import synthetic_volume

NET1 = dict(first_gen=True, filter_size=3, start_fms=256, max_fms=256, add_adj=True, first_nn_arch=True, use_res_net=True)
NET2 = dict(filter_size=3, start_fms=512, max_fms=256, use_res_net=True)


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
    c, f = 5, 8
    for n, h, wl in ((2, 512, 64), (512, 512, 64)):
        src = torch.rand((n, h, wl, c), device="cuda", generator=g)
        dens = torch.rand((n, h, wl * f, 1), device="cuda", generator=g)
        out = torch.empty_like(dens)
        moved = 4 * dens.numel() * (2 + c / f)
        tk = events(lambda: ops.bicubic_cols_add(src, 4, f, dens, out=out))
        tu = events(lambda: ops.add_act(ops.resize_bicubic(src[..., 4:5].contiguous(), h, wl * f), dens))
        print("[%d,%d,%d,%d] x %d: %.2f MB by the fused kernel's count" % (n, h, wl, c, f, moved / 1e6))
        for name, ts in (("mpg_bicubic_cols_add", tk), ("slice, resize_bicubic, add", tu)):
            t = statistics.median(ts)
            print("  %-28s %s ms: %.1f GB/s of that count" % (name, med(ts), moved / (t * 1e-3) / 1e9))
        print("  the count over the copy bandwidth: %.4f ms" % (moved / bw * 1e3))


def volume():
    sim = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    prec = ops.INFERENCE_PREC
    low = torch.as_tensor(synthetic_volume(sim, 4, 0)).cuda()
    g1 = MP.Generator("growing_gen", dict(tile_low=sim, up_res=8, channels=4, **NET1), None, prec, seed=1)
    g0 = MP.Generator("growing_gen", dict(tile_low=sim, up_res=8, channels=4, upsampling_mode=0, **NET2), None, prec, seed=2)
    g2 = MP.Generator("growing_gen", dict(tile_low=sim, up_res=8, channels=4, first_gen=False, **NET2), g0.params(), prec)

    def axis_pair():
        return MP.two_pass_8x_axis(g1, g0, low, 8, batches=(2, 2))[0]

    def zoom_pair():
        v1 = MP.single_pass_8x(g1, low, None, 8, 0, batch=2)
        return MP.single_pass_8x(g2, low, v1, 8, 2, batch=2)

    print("%d^3 -> %d^3, prec %d, lanes %d" % (sim, sim * 8, prec, MP.PASS_LANES[0]))
    for name, fn in (("axis pair (mode 2 upsampleFirst 0, mode 0)", axis_pair), ("zoom pair (mode 2, mode 1)", zoom_pair)):
        ts = []
        for r in range(4):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            v = fn(); torch.cuda.synchronize()
            if r:
                ts.append(time.perf_counter() - t0)
        print("  %-44s %s s per volume; %d of %d voxels above the cutoff" % (name, med(ts), int((v > 0).sum()), v.numel()))
        del v


{"kernel": kernel, "volume": volume}[sys.argv[1] if len(sys.argv) > 1 else "kernel"]()
