"""The device .uni codec on the GPU (uniio.writeUniFromDevice(..., codec="device")): every file it writes must decode
to the source bytes through this package's reader, through gzip, and member by member through raw zlib."""
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from mpgan_amd import uniio  # noqa: E402

U = uniio.UNIT
W = U // 4                      # words per unit
RUNS = (1, 2, 63, 64, 65, 66, 128, 129)     # zero runs between islands: both sides of the 64-word (256-byte) match limit

# (dimX, dimY, dimZ, vec3)
SHAPES = [(n, 1, 1, False) for n in (1, 2, 63, 64, 65, W - 1, W, W + 1, 3 * W + 5)] + [(33, 17, 9, False), (20, 20, 20, True)]


def _patterns(n, rng):
    """name -> uint32 words of the payload"""
    out = {}
    out["zero"] = np.zeros(n, np.uint32)
    out["constant"] = np.full(n, np.float32(0.37).view(np.uint32), np.uint32)
    out["randn"] = rng.standard_normal(n).astype(np.float32).view(np.uint32)
    isl = np.zeros(n, np.float32)
    at, k = 0, 0
    while at < n:                                   # islands of 1..3 distinct values, zero runs of every length in RUNS
        width = 1 + k % 3
        isl[at:at + width] = rng.uniform(0.1, 1.0, min(width, n - at)).astype(np.float32)
        at += width + RUNS[k % len(RUNS)]
        k += 1
    out["islands"] = isl.view(np.uint32)
    span = rng.uniform(0.1, 1.0, n).astype(np.float32)
    span[max(0, min(n, W) - 100):W + 100] = 0.0     # a zero run across the first unit boundary (or up to the end)
    span[2 * W - 1:2 * W + 1] = 0.0                 # and the shortest one across the second
    out["boundary_run"] = span.view(np.uint32)
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x00000001,
                        0x807fffff, 0x00800000, 0x00000000, 0x80000000, 0x80000000, 0xffffffff, 0x90909090, 0x8f8f8f8f],
                       np.uint32)
    out["special_bits"] = np.resize(special, n)
    return out


def _check_file(path, header, words):
    """the three readers of the issue; `words`: the source payload as uint32"""
    raw = open(path, "rb").read()
    first = b"MNT3" + struct.pack(uniio._V4_FORMAT, *[header[k] for k in uniio._V4_FIELDS])
    want = first + words.tobytes()
    head, arr = uniio.readUni(path)
    assert head == header
    assert arr.dtype == np.float32 and np.array_equal(arr.reshape(-1).view(np.uint32), words)
    assert gzip.decompress(raw) == want
    sizes = uniio._member_sizes(raw)
    assert sizes is not None and len(sizes) >= 2, "every member carries the MP size subfield"
    at, got = 0, []
    for size in sizes:
        body = raw[at + uniio._MEMBER_HEAD:at + size - 8]
        crc, isize = struct.unpack_from("<II", raw, at + size - 8)
        part = zlib.decompress(body, -15)
        assert zlib.crc32(part) == crc, "stored CRC-32 of the member at %d" % at
        assert len(part) == isize
        got.append(part)
        at += size
    assert b"".join(got) == want
    return len(raw)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d%s" % (s[0], s[1], s[2], "v3" if s[3] else ""))
def test_round_trip_bit_for_bit(gpu_ops, tmp_path, shape):
    dx, dy, dz, vec3 = shape
    c = 3 if vec3 else 1
    n = dx * dy * dz * c
    header = uniio.make_header(dx, dy, dz, vec3=vec3)
    rng = np.random.default_rng(n)
    for name, words in _patterns(n, rng).items():
        vol = torch.as_tensor(words.view(np.float32).reshape(dz, dy, dx, c)).cuda()
        path = str(tmp_path / (name + ".uni"))
        uniio.writeUniFromDevice(path, header, vol, codec="device")
        _check_file(path, header, words)


def test_more_units_than_one_member_and_unaligned_source(gpu_ops, tmp_path):
    """members of MEMBER_UNITS units: the CRCs of several units combined, a second member, and a source that does not
    start on a 16-byte boundary"""
    n = (uniio.MEMBER_UNITS + 2) * W + 3
    rng = np.random.default_rng(5)
    vals = rng.standard_normal(n + 1).astype(np.float32)
    vals[rng.random(n + 1) < 0.6] = 0.0
    vol = torch.as_tensor(vals).cuda()[1:]
    assert vol.data_ptr() % 16 != 0
    header = uniio.make_header(n, 1, 1)
    path = str(tmp_path / "two_members.uni")
    uniio.writeUniFromDevice(path, header, vol, codec="device")
    _check_file(path, header, vals[1:].view(np.uint32))
    assert len(uniio._member_sizes(open(path, "rb").read())) == 3


def test_unit_streams_and_crcs_of_the_encoder(gpu_ops):
    """the operator layer below the writer: every slot inflates to its unit, sizes and CRCs are per unit, and the
    compaction is the slots back to back"""
    n = 2 * W + 7
    rng = np.random.default_rng(9)
    vals = rng.standard_normal(n).astype(np.float32)
    vals[W // 2:W + 300] = 0.0
    src = torch.as_tensor(vals).cuda()
    slots, sizes, crcs = gpu_ops.deflate_encode(src)
    packed = gpu_ops.deflate_compact(slots, sizes, 3)
    torch.cuda.synchronize()
    assert gpu_ops.deflate_ws_bytes(n * 4) == 3 * uniio.SLOT == slots.numel()
    slots, packed = slots.cpu().numpy(), packed.cpu().numpy()
    sizes, crcs = sizes.cpu().numpy().view(np.uint32), crcs.cpu().numpy().view(np.uint32)
    raw = vals.tobytes()
    at = 0
    for u in range(3):
        piece = raw[u * U:(u + 1) * U]
        body = slots[u * uniio.SLOT:u * uniio.SLOT + sizes[u]].tobytes()
        assert zlib.decompress(body + uniio._FINAL_BLOCK, -15) == piece
        assert int(crcs[u]) == zlib.crc32(piece)
        assert sizes[u] <= len(piece) + 5, "never longer than the stored form"
        assert packed[at:at + sizes[u]].tobytes() == body
        at += int(sizes[u])


def test_size_conditions(gpu_ops, tmp_path):
    n = (1 << 20) // 4
    header = uniio.make_header(n, 1, 1)
    zero = str(tmp_path / "zero.uni")
    uniio.writeUniFromDevice(zero, header, torch.zeros(n, device="cuda"), codec="device")
    print("all-zero 1 MiB -> %d bytes" % os.path.getsize(zero))
    assert os.path.getsize(zero) < (1 << 20) / 50          # a 256-byte match costs 18 bits
    dense = str(tmp_path / "dense.uni")
    vals = np.random.default_rng(2).standard_normal(n).astype(np.float32)
    uniio.writeUniFromDevice(dense, header, torch.as_tensor(vals).cuda(), codec="device")
    print("dense randn 1 MiB -> %d bytes" % os.path.getsize(dense))
    assert os.path.getsize(dense) <= 1.01 * (1 << 20)      # the stored-block bound
    _check_file(dense, header, vals.view(np.uint32))


def test_same_volume_gives_identical_files(gpu_ops, tmp_path):
    n = 3 * W + 11
    vals = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    vals[vals < 0.3] = 0.0
    vol = torch.as_tensor(vals).cuda()
    header = uniio.make_header(n, 1, 1)
    files = []
    for k in range(2):
        path = str(tmp_path / ("run%d.uni" % k))
        uniio.writeUniFromDevice(path, header, vol, codec="device")
        files.append(open(path, "rb").read())
    assert files[0] == files[1]


def test_write_follows_the_current_stream(gpu_ops, tmp_path):
    """the encode is ordered behind the kernel that produces the volume: the file holds the cut-off values"""
    n = 96
    vals = np.random.default_rng(6).uniform(0.0, 1e-3, (n, n, n, 1)).astype(np.float32)
    vol = torch.as_tensor(vals).cuda()
    torch.cuda.synchronize()
    out = torch.empty_like(vol)
    header = uniio.make_header(n, n, n)
    path = str(tmp_path / "cut.uni")
    gpu_ops.cutoff(vol, 5e-4, out=out)
    uniio.writeUniFromDevice(path, header, out, codec="device")
    want = np.where(vals < np.float32(5e-4), np.float32(0), vals)
    _, arr = uniio.readUni(path)
    assert np.array_equal(arr.view(np.uint32), want.view(np.uint32))


def _run_4x(tmp, codec):
    from mpgan_amd.synthetic import synthetic_volume
    sim = 8
    d = tmp / ("codec%d" % codec) / "data" / "sim_1005"
    d.mkdir(parents=True)
    uniio.writeUni(str(d / "density_low_0000.uni"), uniio.make_header(sim, sim, sim), synthetic_volume(sim, 4, 0)[..., 0:1])
    models = tmp / ("codec%d" % codec) / "models"
    (models / "test_0004").mkdir(parents=True)
    args = ["out", 1, "genUni", 1, "synthWeights", 1, "prec", 3, "uniCodec", codec, "upRes", 4, "tileSize", sim, "simSize", sim,
            "fromSim", 1005, "toSim", 1005, "dataDim", 2, "useVelocities", 0, "basePath", str(models) + "/",
            "packedSimPath", str(d.parent) + "/", "frame_min", 0, "frame_max", 1, "velScale", 1.0, "genModel", "gen_resnet",
            "randSeed", 101, "load_model_test", 4, "load_model_no", 1199, "upsamplingMode", 2, "upsampledData", 0]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "GAN", "multipassGAN-4x.py")] + [str(a) for a in args],
                       cwd=str(tmp / ("codec%d" % codec)), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return str(d / "density_low_2x2_0000.uni")


def test_driver_switch(gpu_ops, tmp_path):
    host, device = _run_4x(tmp_path, 0), _run_4x(tmp_path, 1)
    h0, v0 = uniio.readUni(host)
    h1, v1 = uniio.readUni(device)
    assert h0 == h1
    assert v0.shape == v1.shape and np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
    # the two codecs frame different deflate streams: the device one ends every member with the empty final block
    raw = open(device, "rb").read()
    assert raw[-10:-8] == uniio._FINAL_BLOCK and open(host, "rb").read() != raw
    assert gzip.decompress(raw) == gzip.decompress(open(host, "rb").read())
