"""f3, reading back: seconds per volume through uniio.readUni + upload (the host path: zlib on the thread pool, then one
copy to the GPU) and through uniio.readUniToDevice (file bytes up, units inflated by the HIP kernel), alternating in one
process on the volumes of tools/probe_uni_device.py written once with codec "device_dynamic" and once with codec "device",
both with the unit index: two warm-up reads of each, then five timed ones; the decode call (descriptor upload and
kernel) between device events, the file read + upload share of the device path, and what the index adds to the file.
usage: python tools/probe_uni_read.py [n ...]   (volumes of n^3, default 256 512)"""
import os, statistics, sys, tempfile, time
sys.path.insert(0, ".")
import numpy as np, torch
import scipy.ndimage
import mpgan_amd
from mpgan_amd import ops, uniio
from mpgan_amd.synthetic import synthetic_volume


def fmt(ts):
    return "%.3f (%.3f .. %.3f) s" % (statistics.median(ts), min(ts), max(ts))


def host_read(path):
    """the path without the device reader: readUni, then the upload the drivers do"""
    head, a = uniio.readUni(path)
    t = torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return head, t


def device_read(path):
    info = {}
    head, t = uniio.readUniToDevice(path, "cuda:0", info=info)
    torch.cuda.synchronize()
    assert info["path"] == "device", info
    return head, t


def parts_ms(path, reps=5):
    """(file read + upload seconds, ms between device events around the decode call: descriptor upload, then the kernel)"""
    raw = open(path, "rb").read()
    plan = uniio._device_plan(memoryview(raw))
    head, dims, offsets, sizes, members = plan
    offsets, sizes = np.asarray(offsets, np.uint64), np.asarray(sizes, np.uint32)
    n_bytes = 4 * int(np.prod(dims))
    up, ker = [], []
    for r in range(reps + 2):
        torch.cuda.synchronize(); t = time.perf_counter()
        pinned = torch.empty((os.path.getsize(path) + 15) // 16 * 16, dtype=torch.uint8, pin_memory=True)
        with open(path, "rb") as f:
            f.readinto(memoryview(pinned.numpy())[:len(raw)])
        packed = pinned.to("cuda:0", non_blocking=True)
        torch.cuda.synchronize(); t_up = time.perf_counter() - t
        out = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:0")
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        _, crcs, status = ops.inflate_units(packed, offsets, sizes, n_bytes, out=out)
        e[1].record()
        torch.cuda.synchronize()
        assert not bool(status.any())
        if r >= 2:
            up.append(t_up); ker.append(e[0].elapsed_time(e[1]))
    return statistics.median(up), statistics.median(ker)


def main():
    ns = [int(a) for a in sys.argv[1:]] or [256, 512]
    d = tempfile.mkdtemp()
    print("threads available:", len(os.sched_getaffinity(0)), " unit %d bytes, %d units per member" % (uniio.UNIT, uniio.MEMBER_UNITS))
    low = synthetic_volume(64, 1, 0)[..., 0]
    for n in ns:
        vol = np.maximum(scipy.ndimage.zoom(low, n / 64.0, order=1), 0).astype(np.float32)
        vol[vol < 5e-4] = 0
        dev = torch.as_tensor(vol).cuda()
        h = uniio.make_header(n, n, n)
        print("%d^3 (%.0f MB payload, %.0f %% zero words)" % (n, vol.nbytes / 1e6, 100.0 * float((vol == 0).mean())))
        for codec in ("device_dynamic", "device"):
            path, plain = os.path.join(d, "v_%s.uni" % codec), os.path.join(d, "p_%s.uni" % codec)
            uniio.writeUniFromDevice(path, h, dev, codec=codec, unit_index=True)
            uniio.writeUniFromDevice(plain, h, dev, codec=codec)
            size, size_plain = os.path.getsize(path), os.path.getsize(plain)
            times = {"host": [], "device": []}
            for k in range(7):
                for name, fn in (("host", host_read), ("device", device_read)):
                    torch.cuda.synchronize(); t = time.perf_counter()
                    hh, got = fn(path)
                    dt = time.perf_counter() - t
                    if k >= 2:
                        times[name].append(dt)
                    if k == 0:
                        assert hh == h and np.array_equal(got.cpu().numpy()[..., 0].view(np.uint32), vol.view(np.uint32))
                    del got
            mh, md = statistics.median(times["host"]), statistics.median(times["device"])
            spread = max(max(ts) - min(ts) for ts in times.values())
            up, ker = parts_ms(path)
            print("  codec %-14s file %.2f MB, of which the unit index %.3f MB (%.3f %%)" % (codec, size / 1e6, (size - size_plain) / 1e6,
                                                                                        100.0 * (size - size_plain) / size))
            print("    readUni + upload   %s" % fmt(times["host"]))
            print("    readUniToDevice    %s   ratio %.2f x, difference %.3f s, largest spread of five runs %.3f s"
                  % (fmt(times["device"]), mh / md, mh - md, spread))
            print("    of the device path: file read + upload %.3f s, decode call %.3f ms by events (%.0f GB/s of payload)"
                  % (up, ker, vol.nbytes / ker / 1e6), flush=True)


main()
