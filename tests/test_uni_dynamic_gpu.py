"""The per-unit Huffman mode of the device .uni codec on the GPU (ops.deflate_encode(dynamic=True),
uniio.writeUniFromDevice(codec="device_dynamic"), the drivers' uniCodec 2): the kernel's unit streams are those of
tests/deflate_dynamic_ref.py byte for byte, and every file decodes to the source bytes through this package's reader,
through gzip, and member by member through raw zlib."""
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

import deflate_dynamic_ref as R  # noqa: E402

U = uniio.UNIT
W = U // 4


def _payloads():
    out = dict(R.cases())
    rng = np.random.default_rng(1)
    for nbytes in (4, U - 4, U, U + 4, 3 * U + 20):
        v = rng.standard_normal(nbytes // 4).astype(np.float32)
        v[rng.random(nbytes // 4) < 0.4] = 0.0
        out["bytes_%d" % nbytes] = v.view(np.uint32)
    return out


PAYLOADS = _payloads()


@pytest.fixture(scope="module")
def probe():
    return R.probe_volume(128)


def _encode(ops, words, dynamic):
    src = torch.as_tensor(words.view(np.float32)).cuda()
    slots, sizes, crcs = ops.deflate_encode(src, dynamic=dynamic)
    torch.cuda.synchronize()
    slots = slots.cpu().numpy()
    sizes, crcs = sizes.cpu().numpy().view(np.uint32), crcs.cpu().numpy().view(np.uint32)
    return [slots[u * uniio.SLOT:u * uniio.SLOT + int(sizes[u])].tobytes() for u in range(len(sizes))], sizes, crcs


@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_encoder_against_the_restatement(gpu_ops, name):
    words = PAYLOADS[name]
    streams, sizes, crcs = _encode(gpu_ops, words, True)
    fixed_streams, fixed_sizes, _ = _encode(gpu_ops, words, False)
    again, _, _ = _encode(gpu_ops, words, True)
    assert len(streams) == -(-len(words) // W)
    for u, stream in enumerate(streams):
        unit = words[u * W:(u + 1) * W]
        want = R.encode_unit(unit)
        assert len(stream) == len(want), "unit %d: %d bytes, the restatement has %d" % (u, len(stream), len(want))
        assert stream == want, "unit %d differs from the restatement" % u
        assert int(crcs[u]) == zlib.crc32(unit.tobytes())
        assert int(sizes[u]) <= int(fixed_sizes[u])
        assert again[u] == stream
        assert fixed_streams[u] == R.encode_unit(unit, dynamic=False), "the fixed-code encoder's bytes"
    assert zlib.decompress(b"".join(streams) + uniio._FINAL_BLOCK, -15) == words.tobytes()


def test_compaction_takes_dynamic_units(gpu_ops):
    words = PAYLOADS["bytes_%d" % (3 * U + 20)]
    src = torch.as_tensor(words.view(np.float32)).cuda()
    slots, sizes, crcs = gpu_ops.deflate_encode(src, dynamic=True)
    packed = gpu_ops.deflate_compact(slots, sizes, 4)
    torch.cuda.synchronize()
    total = int(sizes.sum())
    assert packed[:total].cpu().numpy().tobytes() == b"".join(R.encode_payload(words))


def _check_file(path, header, words):
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


def _model_file_size(header, words, dynamic):
    """header member + unit streams of the restatement + framing of every member"""
    first = b"MNT3" + struct.pack(uniio._V4_FORMAT, *[header[k] for k in uniio._V4_FIELDS])
    units = -(-len(words) // W)
    members = -(-units // uniio.MEMBER_UNITS)
    body = sum(R.unit_size(words[a:a + W], dynamic) for a in range(0, len(words), W))
    return len(uniio._deflate_member(first, 6)) + body + members * (uniio._MEMBER_HEAD + len(uniio._FINAL_BLOCK) + 8)


def _density(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    v[v < 0.35] = 0.0
    return v


@pytest.mark.parametrize("shape", [(16, 16, 16, False), (33, 17, 9, False), (20, 20, 20, True)],
                         ids=lambda s: "%dx%dx%d%s" % (s[0], s[1], s[2], "v3" if s[3] else ""))
def test_files_round_trip_bit_for_bit(gpu_ops, tmp_path, shape):
    dx, dy, dz, vec3 = shape
    c = 3 if vec3 else 1
    vals = _density((dz, dy, dx, c), dx * dy)
    words = vals.reshape(-1).view(np.uint32)
    header = uniio.make_header(dx, dy, dz, vec3=vec3)
    vol = torch.as_tensor(vals).cuda()
    for codec, dynamic in (("device_dynamic", True), ("device", False)):
        path = str(tmp_path / (codec + ".uni"))
        uniio.writeUniFromDevice(path, header, vol, codec=codec)
        assert _check_file(path, header, words) == _model_file_size(header, words, dynamic)


def test_probe_volume_file_and_its_size(gpu_ops, tmp_path, probe):
    n = 128
    words = probe.reshape(-1).view(np.uint32)
    header = uniio.make_header(n, n, n)
    vol = torch.as_tensor(probe).cuda()
    sizes = {}
    for codec in ("host", "device", "device_dynamic"):
        path = str(tmp_path / (codec + ".uni"))
        uniio.writeUniFromDevice(path, header, vol, level=6, codec=codec)
        sizes[codec] = os.path.getsize(path)
    print("128^3: host %d B, device %d B (%.4f), device_dynamic %d B (%.4f)"
          % (sizes["host"], sizes["device"], sizes["device"] / sizes["host"], sizes["device_dynamic"],
             sizes["device_dynamic"] / sizes["host"]))
    _check_file(str(tmp_path / "device_dynamic.uni"), header, words)
    assert sizes["device_dynamic"] <= 1.03 * sizes["host"]
    assert sizes["device_dynamic"] == _model_file_size(header, words, True)
    assert sizes["device"] == _model_file_size(header, words, False), "the fixed-code codec writes what it wrote"


def test_same_volume_gives_identical_files(gpu_ops, tmp_path):
    words = PAYLOADS["boundary_run_3units"]
    vol = torch.as_tensor(words.view(np.float32)).cuda()
    header = uniio.make_header(len(words), 1, 1)
    files = []
    for k in range(2):
        path = str(tmp_path / ("run%d.uni" % k))
        uniio.writeUniFromDevice(path, header, vol, codec="device_dynamic")
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
    uniio.writeUniFromDevice(path, header, out, codec="device_dynamic")
    want = np.where(vals < np.float32(5e-4), np.float32(0), vals)
    _, arr = uniio.readUni(path)
    assert np.array_equal(arr.view(np.uint32), want.view(np.uint32))


def test_environment_switch_and_unknown_name(gpu_ops, tmp_path, monkeypatch):
    words = PAYLOADS["smooth"]
    vol = torch.as_tensor(words.view(np.float32)).cuda()
    header = uniio.make_header(len(words), 1, 1)
    named, env = str(tmp_path / "named.uni"), str(tmp_path / "env.uni")
    uniio.writeUniFromDevice(named, header, vol, codec="device_dynamic")
    monkeypatch.setenv("MPG_UNI_CODEC", "device_dynamic")
    uniio.writeUniFromDevice(env, header, vol)
    assert open(env, "rb").read() == open(named, "rb").read()
    raw = open(env, "rb").read()
    at = uniio._member_sizes(raw)[0]
    assert raw[at + uniio._MEMBER_HEAD] & 7 == 4, "the payload member opens with a dynamic block"
    monkeypatch.setenv("MPG_UNI_CODEC", "device_huffman")
    with pytest.raises(uniio.UniError):
        uniio.writeUniFromDevice(str(tmp_path / "x.uni"), header, vol)
    with pytest.raises(uniio.UniError):
        uniio.writeUniFromDevice(str(tmp_path / "y.uni"), header, vol, codec="dynamic")


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
    host, dynamic = _run_4x(tmp_path, 0), _run_4x(tmp_path, 2)
    raw_host, raw_dyn = open(host, "rb").read(), open(dynamic, "rb").read()
    assert gzip.decompress(raw_dyn) == gzip.decompress(raw_host)
    h0, v0 = uniio.readUni(host)
    h1, v1 = uniio.readUni(dynamic)
    assert h0 == h1 and np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
    # the file is the dynamic codec's: its unit streams are the restatement's
    words = v1.reshape(-1).view(np.uint32)
    assert len(raw_dyn) == _model_file_size(h1, words, True) and raw_dyn != raw_host
    assert raw_dyn[-10:-8] == uniio._FINAL_BLOCK
