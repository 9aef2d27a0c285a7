"""Wall clock and peak host memory of the training-set loaders of the second 4x network (GAN/multipassGAN-4x.py,
upsamplingMode 1): the host FluidDataLoader against fluiddataloader_device.DeviceFluidDataLoader, on synthetic entries.

  python tools/probe_loader.py [--sim 64] [--up 4] [--entries 4] [--out profiles/loader_device/timing.md]

Both loaders of that network are built, as the driver does: `fl` (density + velocity of three frames, 12 channels, zoomed
by upRes on all three axes; y the three high-resolution frames) and `fl2` (density only; y the previous pass's output).
Each path runs once, in a process of its own under its own time limit; the clock covers the constructor -- .uni decoding,
upload, kernels and download included -- and the start of the HIP runtime is reported separately.  Peak memory is the
child's ru_maxrss, read before the loaders (what the interpreter, the imports and the HIP runtime hold) and after."""
import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_data(folder, sim, up, frames):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import uniio
    from mpgan_amd.synthetic import synthetic_volume
    d = os.path.join(folder, "sim_1000")
    os.makedirs(d)
    hs = sim * up
    for f in range(frames):
        v = synthetic_volume(sim, 4, f)
        uniio.writeUni(os.path.join(d, "density_low_%04d.uni" % f), uniio.make_header(sim, sim, sim), v[..., 0:1], level=1)
        uniio.writeUni(os.path.join(d, "velocity_low_%04d.uni" % f), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4],
                       level=1)
        # content does not matter to the clock: the low density repeated, twice with different gains
        hi = np.repeat(np.repeat(np.repeat(v[..., 0:1], up, 0), up, 1), up, 2)
        uniio.writeUni(os.path.join(d, "density_high_%04d.uni" % f), uniio.make_header(hs, hs, hs), hi, level=1)
        uniio.writeUni(os.path.join(d, "density_low_2x2_%04d.uni" % f), uniio.make_header(hs, hs, hs), 0.9 * hi, level=1)


def child(kind, folder, up, frames):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import fluiddataloader as FDL
    base = folder + os.sep
    common = dict(print_info=0, base_path=base, base_path_y=base, numpy_seed=42, conv_slices=True, conv_axis=2,
                  select_random=0.1, density_threshold=0.002, axis_scaling_y=[1, 1, 1, 1], axis_scaling=[up, up, up, 1],
                  filename="density_low_%04d.uni", oldNamingScheme=False, filename_index_max=frames, filename_index_min=0,
                  indices=[1000], data_fraction=1.0, multi_file_list_y=["density"] * 3, multi_file_idxOff_y=[0, 1, 2])
    res = {"kind": kind}
    if kind == "device":
        import torch
        from mpgan_amd import _lib
        from mpgan_amd.fluiddataloader_device import DeviceFluidDataLoader
        t0 = time.perf_counter()
        torch.zeros(1, device="cuda:0")
        _lib.load()
        torch.cuda.synchronize()
        res["runtime_start_s"] = time.perf_counter() - t0

        def Loader(**kw):
            return DeviceFluidDataLoader(device="cuda:0", **kw)
    else:
        Loader = FDL.FluidDataLoader
    res["rss_start_mb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
    t0 = time.perf_counter()
    fl = Loader(filename_y="density_high_%04d.uni", multi_file_list=["density", "velocity"] * 3,
                multi_file_idxOff=[0, 0, 1, 1, 2, 2], **common)
    t1 = time.perf_counter()
    fl2 = Loader(filename_y="density_low_2x2_%04d.uni", multi_file_list=["density"] * 3, multi_file_idxOff=[0, 1, 2], **common)
    t2 = time.perf_counter()
    peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
    # what neither path can avoid: reading the files
    for e in fl._entries:
        fl._assemble(e.x, fl.multi_file_list, fl.multi_file_idxOff, "arr_0")
        fl._assemble(e.y, fl.multi_file_list_y, fl.multi_file_idxOff_y, "arr_0")
    t3 = time.perf_counter()
    x, y, _ = fl.get()
    res.update(fl_s=t1 - t0, fl2_s=t2 - t1, decode_fl_s=t3 - t2, entries=len(fl._entries), x_shape=list(x.shape),
               y_shape=list(y.shape), x_sum=float(np.sum(x, dtype=np.float64)), y_sum=float(np.sum(y, dtype=np.float64)),
               x2_sum=float(np.sum(fl2.get()[0], dtype=np.float64)), peak_rss_mb=peak)
    print("RESULT " + json.dumps(res))


def run_child(kind, folder, args, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--data", folder, "--up", str(args.up),
           "--entries", str(args.entries)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError("%s child failed (%d): %s" % (kind, r.returncode, (r.stdout + r.stderr)[-2000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sim", type=int, default=64)
    ap.add_argument("--up", type=int, default=4)
    ap.add_argument("--entries", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-limit", type=int, default=900)
    ap.add_argument("--device-limit", type=int, default=300)
    ap.add_argument("--child", default=None)
    ap.add_argument("--data", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.data, args.up, args.entries)
    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        write_data(folder, args.sim, args.up, args.entries)
        print("wrote %d frames at simSize %d upRes %d in %.1f s" % (args.entries, args.sim, args.up, time.perf_counter() - t0))
        dev = run_child("device", folder, args, args.device_limit)
        print(json.dumps(dev))
        host = run_child("host", folder, args, args.host_limit)
        print(json.dumps(host))
    same = host["x_shape"] == dev["x_shape"] and host["y_shape"] == dev["y_shape"]
    lines = [
        "# Training-set loaders of the second 4x network: host against device",
        "",
        "`python tools/probe_loader.py --sim %d --up %d --entries %d`: %d entries, x [%d^3 x 12] -> [%d^3 x 12] "
        "(conv_axis 2, select_random 0.1, density_threshold 0.002), one run each, a process each; the clock covers the "
        "constructors (file decoding, upload, kernels, download)." % (args.sim, args.up, args.entries, host["entries"],
                                                                      args.sim, args.sim * args.up),
        "",
        "| | host FluidDataLoader | DeviceFluidDataLoader |",
        "|---|---|---|",
        "| `fl` (12 channels + three high-res y frames), s | %.2f | %.2f |" % (host["fl_s"], dev["fl_s"]),
        "| `fl2` (3 channels + three previous-pass y frames), s | %.2f | %.2f |" % (host["fl2_s"], dev["fl2_s"]),
        "| both, s | %.2f | %.2f |" % (host["fl_s"] + host["fl2_s"], dev["fl_s"] + dev["fl2_s"]),
        "| of `fl`: reading and decoding its .uni files again, s | %.2f | %.2f |" % (host["decode_fl_s"], dev["decode_fl_s"]),
        "| HIP runtime and library start, before the clock, s | - | %.2f |" % dev["runtime_start_s"],
        "| host memory before the loaders (interpreter, imports, HIP runtime), MB | %.0f | %.0f |"
        % (host["rss_start_mb"], dev["rss_start_mb"]),
        "| peak host memory (ru_maxrss), MB | %.0f | %.0f |" % (host["peak_rss_mb"], dev["peak_rss_mb"]),
        "| growth during the loaders, MB | %.0f | %.0f |"
        % (host["peak_rss_mb"] - host["rss_start_mb"], dev["peak_rss_mb"] - dev["rss_start_mb"]),
        "| x, y shapes | %s, %s | %s, %s |" % (host["x_shape"], host["y_shape"], dev["x_shape"], dev["y_shape"]),
        "| sum x, sum y, sum x of `fl2` | %.6g, %.6g, %.6g | %.6g, %.6g, %.6g |"
        % (host["x_sum"], host["y_sum"], host["x2_sum"], dev["x_sum"], dev["y_sum"], dev["x2_sum"]),
        "",
        "Speed-up of both loaders: %.1fx.  Shapes %s." % ((host["fl_s"] + host["fl2_s"]) / (dev["fl_s"] + dev["fl2_s"]),
                                                         "agree" if same else "DIFFER"),
        "",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
