"""Preview images, timing (profiles/preview/timing.md).  usage: python tools/probe_preview.py <what> [n]
  kernel    mpg_volume_projections on one n^3 volume (default 512) against the same three planes from (vol / 80).sum(k) in
            torch, alternating in one process: three warm-up rounds, ten timed ones, device events; results compared
  counters  three calls of mpg_volume_projections and nothing else: the run to put under a counter collection of its own
  frame     one frame of the multi-network 8x driver at sim n / 8 (default 64 -> 512^3, three synthetic-weight networks):
            "time for network(s)" without a sink, the same frame with a sink (kernels, download, PNG encoding, file
            writes), and the frame-110 dump of tileSizeHigh = n planes per axis on its own"""
import os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, ".")
import numpy as np, torch
import mpgan_amd
from mpgan_amd import _lib, multipass as MP, ops, preview
from mpgan_amd.synthetic import synthetic_volume


def volume(n):
    g = torch.Generator(device="cuda").manual_seed(1)
    return torch.rand((n, n, n), device="cuda", generator=g) ** 3


def med(ts):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(ts), min(ts), max(ts))


def kernel(n):
    vol = volume(n)
    div = torch.tensor(80.0, device="cuda")

    def ours():
        return ops.volume_projections(vol, 80.0)

    def baseline():
        q = vol / div
        return q.sum(0), q.sum(1), q.sum(2)

    times = {"hip": [], "torch": []}
    for r in range(13):
        for name, fn in (("hip", ours), ("torch", baseline)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); res = fn(); b.record()
            torch.cuda.synchronize()
            if r >= 3:
                times[name].append(a.elapsed_time(b))
    got, want = ours(), baseline()
    err = max(float(((g - w).abs().max() / w.abs().max())) for g, w in zip(got, want))
    mb = vol.numel() * 4 / 1e6
    print("%d^3 volume, %.0f MB; planes agree to %.2e of their largest value" % (n, mb, err))
    for name in ("hip", "torch"):
        t = statistics.median(times[name])
        print("  %-5s %s ms: %.0f GB/s of the volume's bytes" % (name, med(times[name]), mb / t))
    ws = int(_lib.load().mpg_volume_projections_ws_bytes(n, n, n))
    print("  workspace of partial sums: %.1f MB" % (ws / 1e6))


def counters(n):
    vol = volume(n)
    for _ in range(3):
        ops.volume_projections(vol, 80.0)
    torch.cuda.synchronize()


CFG = [dict(first_gen=True, filter_size=3, start_fms=256, max_fms=256, add_adj=True, first_nn_arch=True, use_res_net=True),
       dict(first_gen=False, filter_size=5, start_fms=192, max_fms=192, use_res_net=True),
       dict(first_gen=False, filter_size=5, start_fms=192, max_fms=96, use_res_net=False)]


def frame(n):
    sim = n // 8
    low = torch.as_tensor(synthetic_volume(sim, 4, 0)).cuda()
    gens = [MP.Generator("growing_gen", dict(tile_low=sim, up_res=8, channels=4, **c), None, seed=100 + i) for i, c in enumerate(CFG)]
    d = tempfile.mkdtemp()

    def run(frame_no):
        sink = None if frame_no is None else preview.PreviewSink(d, frame_no, n)
        torch.cuda.synchronize(); t = time.perf_counter()
        MP.multipass_8x(gens, low, 8, previews=sink)
        torch.cuda.synchronize()
        return time.perf_counter() - t, sink

    run(None), run(7)                                      # warm-up: code objects, workspaces, the sink's kernels
    plain, with_sink = [], []
    for _ in range(3):
        plain.append(run(None)[0])
        dt, sink = run(7)
        with_sink.append(dt)
    files = len(set(sink.written))
    size = sum(os.path.getsize(os.path.join(d, f)) for f in set(sink.written))
    print("sim %d -> %d^3, three networks, one frame" % (sim, n))
    print("  time for 3 network(s), no sink:   %s s" % med(plain))
    print("  the same frame with a sink:       %s s  (%d files, %.2f MB of PNG)" % (med(with_sink), files, size / 1e6))
    print("  preview step (difference of the medians): %.3f s" % (statistics.median(with_sink) - statistics.median(plain)))
    # the parts of the preview step on a volume of the same size, each ended by a synchronise
    vol = volume(n)
    for what, fn in (("projection_image + download", lambda: preview.projection_image(vol).cpu()),
                     ("slice_images of the two mid planes + download",
                      lambda: [i.cpu() for v in preview.slice_images(vol, (1, 0, 2), [n // 2 - 1, n // 2]).values() for _, i in v])):
        fn(); ts = []
        for _ in range(5):
            torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
        print("  %-48s %s ms" % (what, med([x * 1e3 for x in ts])))
    img = preview.projection_image(vol).cpu().numpy()
    ts = []
    for _ in range(5):
        t = time.perf_counter(); preview.heldout.encode_gray_png(img); ts.append(time.perf_counter() - t)
    print("  %-48s %s ms" % ("encode_gray_png of one %d x %d picture" % img.shape, med([x * 1e3 for x in ts])))
    # frame 110: every plane along every axis
    d110 = tempfile.mkdtemp()
    sink = preview.PreviewSink(d110, 110, n)
    torch.cuda.synchronize(); t = time.perf_counter()
    kinds = preview.slice_images(vol, (1, 0, 2), range(n))
    torch.cuda.synchronize(); t_dev = time.perf_counter() - t
    t = time.perf_counter()
    sink.slices(vol, (1, 0, 2))
    t_all = time.perf_counter() - t
    print("  frame-110 dump: %d planes on the device %.3f s; whole step (kernels, download, encoding, %d files) %.2f s"
          % (sum(len(v) for v in kinds.values()), t_dev, len(set(sink.written)), t_all))
    shutil.rmtree(d), shutil.rmtree(d110)


what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
{"kernel": kernel, "counters": counters, "frame": frame}[what](n)
