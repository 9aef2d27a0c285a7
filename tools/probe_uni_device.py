"""f3, device codecs: seconds per volume through uniio.writeUniFromDevice with codec "host" (zlib level 6 on the thread
pool), codec "device" (HIP deflate kernels, fixed Huffman code) and codec "device_dynamic" (the same with a Huffman code
per unit), alternating in one process into one directory: two warm-up writes of each, then five timed ones; file sizes,
readUni seconds, and the encode + compaction kernels' own time from device events for both device codecs.
usage: python tools/probe_uni_device.py [n ...]   (volumes of n^3, default 256 512)"""
import os, statistics, sys, tempfile, time
sys.path.insert(0, ".")
import numpy as np, torch
import scipy.ndimage
import mpgan_amd
from mpgan_amd import ops, uniio
from mpgan_amd.synthetic import synthetic_volume


def fmt(ts):
    return "%.3f (%.3f .. %.3f) s" % (statistics.median(ts), min(ts), max(ts))


CODECS = ("host", "device", "device_dynamic")


def kernels_ms(dev, dynamic, reps=5):
    """device-event time of encode + compaction over the whole payload, slab by slab as the writer runs them"""
    flat = dev.reshape(-1)
    per = uniio.SLAB_BYTES // 4
    units = (min(flat.numel(), per) * 4 + uniio.UNIT - 1) // uniio.UNIT
    slots = torch.empty(units * uniio.SLOT, dtype=torch.uint8, device="cuda")
    packed = torch.empty_like(slots)
    sizes = torch.empty(units, dtype=torch.int32, device="cuda")
    crcs = torch.empty_like(sizes)
    enc, tot = [], []
    for r in range(reps + 2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t_enc = t_all = 0.0
        for c in range(0, flat.numel(), per):
            piece = flat[c:c + per]
            e[0].record()
            ops.deflate_encode(piece, slots, sizes, crcs, dynamic=dynamic)
            e[1].record()
            ops.deflate_compact(slots, sizes, (piece.numel() * 4 + uniio.UNIT - 1) // uniio.UNIT, packed)
            e[2].record()
            torch.cuda.synchronize()
            t_enc += e[0].elapsed_time(e[1]); t_all += e[0].elapsed_time(e[2])
        if r >= 2:
            enc.append(t_enc); tot.append(t_all)
    return statistics.median(enc), statistics.median(tot)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [256, 512]
    d = tempfile.mkdtemp()
    print("threads available:", len(os.sched_getaffinity(0)), " unit %d bytes, %d units per member" % (uniio.UNIT, uniio.MEMBER_UNITS))
    low = synthetic_volume(64, 1, 0)[..., 0]
    for n in sizes:
        vol = np.maximum(scipy.ndimage.zoom(low, n / 64.0, order=1), 0).astype(np.float32)
        vol[vol < 5e-4] = 0
        dev = torch.as_tensor(vol).cuda()
        h = uniio.make_header(n, n, n)
        paths = {c: os.path.join(d, "v_%s.uni" % c) for c in CODECS}
        times = {c: [] for c in CODECS}
        for k in range(7):
            for c in CODECS:
                torch.cuda.synchronize(); t = time.perf_counter()
                uniio.writeUniFromDevice(paths[c], h, dev, level=6, codec=c)
                if k >= 2:
                    times[c].append(time.perf_counter() - t)
        mb = {c: os.path.getsize(paths[c]) / 1e6 for c in paths}
        print("%d^3 (%.0f MB payload, %.0f %% zero words)" % (n, vol.nbytes / 1e6, 100.0 * float((vol == 0).mean())))
        for c in CODECS:
            t = time.perf_counter(); hh, a = uniio.readUni(paths[c]); tr = time.perf_counter() - t
            assert hh == h and np.array_equal(a[..., 0].view(np.uint32), vol.view(np.uint32))
            print("  codec %-14s write %s, file %.2f MB, readUni %.3f s" % (c, fmt(times[c]), mb[c], tr), flush=True)
        for c in CODECS[1:]:
            enc, tot = kernels_ms(dev, c == "device_dynamic")
            print("  %s kernels: encode %.3f ms (%.0f GB/s of payload), encode + compaction %.3f ms; file size ratio %s / host %.3f"
                  % (c, enc, vol.nbytes / enc / 1e6, tot, c, mb[c] / mb["host"]), flush=True)


main()
