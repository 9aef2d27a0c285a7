"""Reading .uni volumes on the GPU: ops.inflate_units on the encoder kernels' own streams at every alignment, on malformed
streams (after the CPU build of the same decode core has passed the sanitizers on the very same bytes),
uniio.readUniToDevice against readUni, and the deviceRead / uniIndex parameters of the 4x and 8x drivers."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_dynamic_ref as R
import uni_inflate_ref as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = R.UNIT
ZONE = 4096
FILL = 0x5A


def _mix(n_words):
    """n_words of payload with runs, smooth values and noise"""
    rng = np.random.default_rng(n_words)
    base = np.concatenate([R.smooth_unit(), R.cases()["runs_63_64_65"], rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32),
                           np.zeros(2000, np.uint32)])
    return np.resize(base, n_words).copy()


def _payloads():
    W = UNIT // 4
    out = {"4_bytes": _mix(1), "unit_minus_4": _mix(W - 1), "one_unit": _mix(W), "unit_plus_4": _mix(W + 1),
           "three_units_plus_20": _mix(3 * W + 5)}
    out.update(R.cases())
    return out


PAYLOADS = _payloads()


def _encode_on_gpu(words, dynamic):
    """the encoder kernels' own unit streams of a payload, as bytes"""
    import torch
    from mpgan_amd import ops
    src = torch.from_numpy(words.view(np.float32).copy()).cuda()
    units = (4 * len(words) + UNIT - 1) // UNIT
    slots, sizes, _ = ops.deflate_encode(src, dynamic=dynamic)
    packed = ops.deflate_compact(slots, sizes, units)
    sizes = sizes.cpu().numpy().view(np.uint32).astype(np.int64)
    raw = packed[:int(sizes.sum())].cpu().numpy().tobytes()
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    return [raw[cuts[u]:cuts[u + 1]] for u in range(units)]


def _decode(streams, n_bytes, start=0):
    """ops.inflate_units on streams laid back to back from byte `start` of packed, the output between two sentinel zones
    -> (output bytes, crcs, status)"""
    import torch
    from mpgan_amd import ops
    blob = b"\xa5" * start + b"".join(streams)
    sizes = [len(s) for s in streams]
    offsets = (start + np.concatenate([[0], np.cumsum(sizes)[:-1]])).astype(np.uint64)
    packed = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    buf = torch.full((ZONE + n_bytes + ZONE,), FILL, dtype=torch.uint8, device="cuda")
    out, crcs, status = ops.inflate_units(packed, offsets, sizes, n_bytes, out=buf[ZONE:ZONE + n_bytes])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:ZONE] == FILL).all() and (host[ZONE + n_bytes:] == FILL).all(), "a sentinel zone was written"
    assert out.data_ptr() == buf.data_ptr() + ZONE
    return host[ZONE:ZONE + n_bytes].tobytes(), crcs.cpu().numpy().view(np.uint32), status.cpu().numpy()


@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_inflate_units_on_the_encoders_own_streams(name, dynamic):
    words = PAYLOADS[name]
    src = words.tobytes()
    streams = _encode_on_gpu(words, dynamic)
    want = [zlib.crc32(src[a:a + UNIT]) for a in range(0, len(src), UNIT)]
    first = None
    for start in (0, 1, 7, 15):
        out, crcs, status = _decode(streams, len(src), start)
        assert not status.any(), (start, status)
        assert out == src, start
        assert crcs.tolist() == want, start
        if first is None:
            first = (out, crcs.tolist())
    again = _decode(streams, len(src), 0)
    assert (again[0], again[1].tolist()) == first and not again[2].any()


def test_inflate_units_refuses_streams_that_leave_packed():
    import torch
    from mpgan_amd import _lib, ops
    words = PAYLOADS["unit_plus_4"]
    streams = _encode_on_gpu(words, True)
    blob = b"".join(streams)
    packed = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    sizes = [len(s) for s in streams]
    offsets = [0, sizes[0]]
    for bad_off, bad_size in (([0, sizes[0] + 1], sizes), (offsets, [sizes[0], sizes[1] + 1]), ([0, 1 << 40], sizes),
                              (offsets, [sizes[0], 0xffffffff])):
        with pytest.raises(_lib.MpgError):
            ops.inflate_units(packed, bad_off, bad_size, 4 * len(words))
    with pytest.raises(_lib.MpgError):
        ops.inflate_units(packed, offsets[:1], sizes[:1], 4 * len(words))
    # the C entry itself: nothing is launched, the output keeps its fill
    lib = _lib.load()
    padded = torch.zeros((len(blob) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    padded[:len(blob)] = packed
    out = torch.full((4 * len(words),), FILL, dtype=torch.uint8, device="cuda")
    meta = torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    off_c = (ctypes.c_uint64 * 2)(0, sizes[0])
    size_c = (ctypes.c_uint32 * 2)(sizes[0], padded.numel() - sizes[0] + 1)
    rc = lib.mpg_inflate_units(None, padded.data_ptr(), padded.numel(), off_c, size_c, 2, out.data_ptr(), out.numel(),
                               meta[0].data_ptr(), meta[1].data_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"leaves" in lib.mpg_last_error()
    assert bool((out == FILL).all()) and bool((meta == -7).all())
    # and the same call with the true sizes decodes
    size_c[1] = sizes[1]
    rc = lib.mpg_inflate_units(None, padded.data_ptr(), padded.numel(), off_c, size_c, 2, out.data_ptr(), out.numel(),
                               meta[0].data_ptr(), meta[1].data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and out.cpu().numpy().tobytes() == words.tobytes() and not bool(meta[1].any())


def test_malformed_streams_end_with_a_status():
    bad = U.gpu_malformed()
    assert len(bad) == 12
    # the same bytes through the CPU build of the same decode core, under ASan and UBSan, first
    try:
        results, _ = U.run_program([(0, stream, n) for _, stream, n in bad])
    except (AssertionError, subprocess.CalledProcessError, OSError) as e:
        pytest.skip("the sanitizer run of the decode core did not pass on these bytes: %s" % (str(e)[-300:],))
    assert all(r[0] != 0 for r in results)
    good_words = PAYLOADS["runs_63_64_65"]
    good = [R.encode_unit(good_words, True)]
    for (label, stream, n), cpu in zip(bad, results):
        _, _, status = _decode([stream], n, start=5)
        assert status[0] != 0, label
        assert status[0] == cpu[0], label
        out, crcs, status = _decode(good, 4 * len(good_words), start=3)
        assert out == good_words.tobytes() and status[0] == 0 and crcs[0] == zlib.crc32(out), label
    # a bad unit between good ones does not touch its neighbours
    W = UNIT // 4
    three = PAYLOADS["three_units_plus_20"][:3 * W]
    streams = R.encode_payload(three, True)
    assert streams[1][0] & 7 != 0 and streams[1][-4:] == b"\0\0\xff\xff"     # a Huffman block and its closing stored block
    streams[1] = streams[1][:-3] + b"\0\0\0"
    out, crcs, status = _decode(streams, 4 * len(three), start=9)
    src = three.tobytes()
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert out[:UNIT] == src[:UNIT] and out[2 * UNIT:] == src[2 * UNIT:]


# ---------------------------------------------------------------- readUniToDevice
def _volumes():
    rng = np.random.default_rng(5)
    p64, p128 = R.probe_volume(64), R.probe_volume(128)
    vec = np.zeros((16, 20, 24, 3), np.float32)
    vec[4:12, 5:15] = rng.uniform(-1, 1, (8, 10, 24, 3)).astype(np.float32)
    return {"probe64": (p64[..., None], False), "probe128": (p128[..., None], False), "vec3": (vec, True),
            "last_unit_4_bytes": (rng.uniform(0, 1, (1, 1, UNIT // 4 + 1, 1)).astype(np.float32), False),
            "two_members": (np.concatenate([p128, p128[:32]])[..., None], False)}


@pytest.fixture(scope="module")
def volumes():
    return _volumes()


@pytest.mark.parametrize("codec", ["device", "device_dynamic"])
@pytest.mark.parametrize("name", ["probe64", "probe128", "vec3", "last_unit_4_bytes", "two_members"])
def test_readUniToDevice_decodes_indexed_files_on_the_device(tmp_path, volumes, name, codec):
    import torch
    from mpgan_amd import uniio
    vol, vec3 = volumes[name]
    z, y, x = vol.shape[:3]
    head = uniio.make_header(x, y, z, vec3=vec3, info=b"test", timestamp=3)
    path = str(tmp_path / "v.uni")
    uniio.writeUniFromDevice(path, head, torch.from_numpy(vol).cuda(), codec=codec, unit_index=True)
    raw = open(path, "rb").read()
    index = uniio.unit_index(raw)
    assert index is not None and sum(len(s) for _, s in index) == -(-vol.nbytes // UNIT)
    want_head, want = uniio.readUni(path)
    assert np.array_equal(want.view(np.uint32), vol.view(np.uint32))
    info = {}
    got_head, got = uniio.readUniToDevice(path, "cuda:0", info=info)
    assert info["path"] == "device", info
    assert got_head == want_head
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the index is all that the flag adds
    plain = str(tmp_path / "p.uni")
    uniio.writeUniFromDevice(plain, head, torch.from_numpy(vol).cuda(), codec=codec)
    assert len(raw) == os.path.getsize(plain) + sum(4 + 4 * len(s) for _, s in index)


def test_readUniToDevice_falls_back_to_the_host(tmp_path, volumes, monkeypatch):
    import torch
    from mpgan_amd import uniio
    vol, _ = volumes["probe64"]
    head = uniio.make_header(64, 64, 64)
    dev_vol = torch.from_numpy(vol).cuda()
    paths = {}
    paths["host codec"] = str(tmp_path / "host.uni")
    uniio.writeUniFromDevice(paths["host codec"], head, dev_vol, codec="host")
    paths["no index"] = str(tmp_path / "plain.uni")
    uniio.writeUniFromDevice(paths["no index"], head, dev_vol, codec="device_dynamic")
    paths["single member"] = str(tmp_path / "ref.uni")
    with gzip.open(paths["single member"], "wb") as f:                   # the reference's writer
        f.write(b"MNT3" + struct.pack(uniio._V4_FORMAT, *[head[k] for k in uniio._V4_FIELDS]) + vol.tobytes())
    for what, path in paths.items():
        info = {}
        got_head, got = uniio.readUniToDevice(path, "cuda:0", info=info)
        assert info["path"] == "host" and info["reason"], what
        assert got_head == head and got.is_cuda and tuple(got.shape) == vol.shape, what
        assert np.array_equal(got.cpu().numpy().view(np.uint32), vol.view(np.uint32)), what
    # the environment switches the index on like the argument
    monkeypatch.setenv("MPG_UNI_INDEX", "1")
    uniio.writeUniFromDevice(paths["no index"], head, dev_vol, codec="device_dynamic")
    info = {}
    uniio.readUniToDevice(paths["no index"], "cuda:0", info=info)
    assert info["path"] == "device"


def test_readUniToDevice_raises_for_a_flipped_payload_byte(tmp_path):
    import torch
    from mpgan_amd import uniio
    rng = np.random.default_rng(9)
    # random bits: stored units, in which any flipped byte decodes and changes the CRC
    vol = rng.integers(0, 1 << 32, (4, 32, 128, 1), dtype=np.uint64).astype(np.uint32).view(np.float32)
    head = uniio.make_header(128, 32, 4)
    path = str(tmp_path / "v.uni")
    uniio.writeUniFromDevice(path, head, torch.from_numpy(vol).cuda(), codec="device_dynamic", unit_index=True)
    raw = bytearray(open(path, "rb").read())
    (body, sizes), = uniio.unit_index(bytes(raw))
    assert raw[body] & 7 == 0 and sizes[0] == UNIT + 5                   # a stored block
    info = {}
    uniio.readUniToDevice(path, "cuda:0", info=info)
    assert info["path"] == "device"
    raw[body + sizes[0] + 1000] ^= 0x10                                  # inside the second unit's bytes
    with open(path, "wb") as f:
        f.write(bytes(raw))
    with pytest.raises(uniio.UniError):
        uniio.readUniToDevice(path, "cuda:0", info=info)
    assert info["path"] == "host" and "CRC" in info["reason"]
    with pytest.raises(uniio.UniError):
        uniio.readUni(path)


# ---------------------------------------------------------------- drivers
def _run(script, args, cwd, ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "GAN", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _make_sim(tmp, sim, vel):
    from mpgan_amd import uniio
    from mpgan_amd.synthetic import synthetic_volume
    d = tmp / "data" / "sim_1005"
    d.mkdir(parents=True)
    v = synthetic_volume(sim, 4, 0)
    uniio.writeUni(str(d / "density_low_0000.uni"), uniio.make_header(sim, sim, sim), v[..., 0:1])
    if vel:
        uniio.writeUni(str(d / "velocity_low_0000.uni"), uniio.make_header(sim, sim, sim, vec3=True), v[..., 1:4])
    for t in (0, 4, 9, 48):
        (tmp / "models" / ("test_%04d" % t)).mkdir(parents=True, exist_ok=True)
    return d


def _chain(tmp_path, script, first, second, in_name, out_name):
    """the first pass writes an indexed volume; the second pass gives the same bits with deviceRead 0, with deviceRead 1,
    and with deviceRead 1 over the same input without its index"""
    import torch
    from mpgan_amd import uniio
    d = tmp_path / "data" / "sim_1005"
    _run(script, first + ["uniCodec", 2, "uniIndex", 1], str(tmp_path))
    assert uniio.unit_index(open(str(d / in_name), "rb").read()) is not None
    results = {}

    def second_pass(key, device_read):
        _run(script, second + ["uniCodec", 2, "uniIndex", 1, "deviceRead", device_read], str(tmp_path))
        assert uniio.unit_index(open(str(d / out_name), "rb").read()) is not None
        results[key] = uniio.readUni(str(d / out_name))[1].copy()
        os.remove(str(d / out_name))

    second_pass("host read", 0)
    second_pass("device read", 1)
    head, vol = uniio.readUni(str(d / in_name))
    uniio.writeUniFromDevice(str(d / in_name), head, torch.from_numpy(vol.copy()).cuda(), codec="device_dynamic")
    assert uniio.unit_index(open(str(d / in_name), "rb").read()) is None
    second_pass("device read, no index", 1)
    base = results["host read"]
    assert base.shape == (32, 32, 32, 1) and float(np.abs(base).max()) > 0
    for key, vol in results.items():
        assert np.array_equal(vol.view(np.uint32), base.view(np.uint32)), key


def test_4x_chain_reads_the_previous_pass_on_the_device(tmp_path):
    sim, up = 8, 4
    _make_sim(tmp_path, sim, 0)
    common = ["upRes", up, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005, "toSim", 1005, "dataDim", 2,
              "useVelocities", 0, "basePath", str(tmp_path / "models") + "/", "packedSimPath", str(tmp_path / "data") + "/",
              "frame_min", 0, "frame_max", 1, "genUni", 1, "velScale", 1.0, "synthWeights", 1, "genModel", "gen_resnet"]
    first = common + ["randSeed", 101, "load_model_test", 4, "load_model_no", 1199, "upsamplingMode", 2, "upsampledData", 0]
    second = common + ["randSeed", 102, "load_model_test", 48, "load_model_no", 799, "upsamplingMode", 1, "upsampledData", 1]
    _chain(tmp_path, "multipassGAN-4x.py", first, second, "density_low_2x2_0000.uni", "density_low_1x1_0000.uni")
    r = _run("multipassGAN-4x.py", first + ["uniIndex", 1, "uniCodec", 0], str(tmp_path), ok=False)
    assert r.returncode == 1 and "ERROR:" in r.stdout and "uniIndex" in r.stdout


def test_8x_chain_reads_the_previous_pass_on_the_device(tmp_path):
    sim, up = 4, 8
    _make_sim(tmp_path, sim, 1)
    common = ["upRes", up, "pixelNorm", 1, "batchNorm", 0, "out", 1, "tileSize", sim, "simSize", sim, "fromSim", 1005,
              "toSim", 1005, "dataDim", 2, "useVelocities", 1, "basePath", str(tmp_path / "models") + "/",
              "packedSimPath", str(tmp_path / "data") + "/", "frame_max", 1, "frame_min", 0, "velScale", 1.0, "genUni", 1,
              "upsampleMode", 1, "addBicubicUpsample", 1, "synthWeights", 1, "prec", 3, "genModel", "gen_resnet"]
    first = common + ["randSeed", 400, "use_res_net", 1, "firstNNArch", 1, "add_adj_idcs", 1, "load_model_test", 0,
                      "load_model_no", 299, "upsampledData", 0, "upsamplingMode", 2, "maxFms", 256, "startFms", 256,
                      "filterSize", 3, "transposeAxis", 0]
    second = common + ["randSeed", 401, "use_res_net", 1, "outNNTestNo", 0, "load_model_test", 9, "load_model_no", 499,
                       "upsampledData", 1, "upsamplingMode", 1, "maxFms", 192, "startFms", 192, "filterSize", 5, "transposeAxis", 2]
    _chain(tmp_path, "multipassGAN-8x.py", first, second, "density_low_t0000_2x2_0000.uni", "density_low_t0009_1x1_0000.uni")
    r = _run("multipassGAN-8x.py", first + ["uniIndex", 1, "uniCodec", 0], str(tmp_path), ok=False)
    assert r.returncode == 1 and "ERROR:" in r.stdout and "uniIndex" in r.stdout
