"""Host side of the device .uni codec: the member assembler, the CRC combination and the codec switch of
uniio.writeUniFromDevice.  No GPU: unit bodies come from zlib."""
import gzip
import struct
import zlib

import numpy as np
import pytest
import torch

import mpgan_amd  # noqa: F401
from mpgan_amd import uniio

U = uniio.UNIT


def _unit_body(buf):
    """what the device encoder yields for one unit: a byte-aligned raw deflate stream without a final block"""
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    return co.compress(buf) + co.flush(zlib.Z_SYNC_FLUSH)


def _members(raw):
    sizes = uniio._member_sizes(raw)
    assert sizes is not None, "not a stream of size-tagged members"
    at = 0
    for size in sizes:
        yield raw[at + uniio._MEMBER_HEAD:at + size - 8], struct.unpack_from("<II", raw, at + size - 8)
        at += size


def test_unit_constants_match_the_library_header():
    from mpgan_amd import _lib
    assert (uniio.UNIT, uniio.SLOT, uniio.SLAB_BYTES) == (_lib.DEFLATE_UNIT, _lib.DEFLATE_SLOT, _lib.DEFLATE_SLAB)
    assert U % 4 == 0 and uniio.SLAB_BYTES % U == 0 and uniio.CHUNK_BYTES % U == 0


@pytest.mark.parametrize("member_units", [1, 3, 256])
def test_member_assembler_round_trip(tmp_path, member_units):
    rng = np.random.default_rng(7)
    n = (5 * U + 4 * 37) // 4                      # five full units and a short one
    data = rng.standard_normal(n).astype(np.float32)
    data[U // 8:U // 2] = 0.0
    header = uniio.make_header(n, 1, 1)
    first = b"MNT3" + struct.pack(uniio._V4_FORMAT, *[header[k] for k in uniio._V4_FIELDS])
    payload = data.tobytes()
    pieces = [payload[a:a + U] for a in range(0, len(payload), U)]
    bodies = [_unit_body(p) for p in pieces]
    path = str(tmp_path / "assembled.uni")
    with open(path, "wb") as out:
        out.write(uniio._deflate_member(first, 6))
        uniio.write_unit_members(out, b"".join(bodies), [len(b) for b in bodies], [zlib.crc32(p) for p in pieces],
                                 [len(p) for p in pieces], member_units=member_units)
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == first + payload
    head, arr = uniio.readUni(path)
    assert head == header
    assert np.array_equal(arr.reshape(-1).view(np.uint32), data.view(np.uint32))
    members = list(_members(raw))
    assert len(members) == 1 + -(-len(pieces) // member_units)
    got = b""
    for body, (crc, isize) in members:
        part = zlib.decompress(body, -15)
        assert zlib.crc32(part) == crc and len(part) == isize
        got += part
    assert got == first + payload


def test_member_assembler_rejects_inconsistent_sizes(tmp_path):
    body = _unit_body(b"\0" * 64)
    with open(str(tmp_path / "x"), "wb") as out, pytest.raises(uniio.UniError):
        uniio.write_unit_members(out, body + b"\0", [len(body)], [zlib.crc32(b"\0" * 64)], [64])


def test_crc_combination_equals_zlib():
    rng = np.random.default_rng(3)
    lengths = [1, 255, 256, U, U + 4, 0, 7]
    pieces = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]
    assert uniio.crc32_combine([zlib.crc32(p) for p in pieces], lengths) == zlib.crc32(b"".join(pieces))
    for p in pieces:                                   # a single piece is its own CRC
        assert uniio.crc32_combine([zlib.crc32(p)], [len(p)]) == zlib.crc32(p)
    zeros = [b"\0" * U, b"\0" * U, b"\0" * 4]          # all-zero pieces: the start value still has to travel
    assert uniio.crc32_combine([zlib.crc32(p) for p in zeros], [len(p) for p in zeros]) == zlib.crc32(b"".join(zeros))
    assert uniio.crc32_combine([], []) == zlib.crc32(b"")


def test_device_codec_on_a_cpu_tensor_raises(tmp_path, monkeypatch):
    vol = torch.zeros(4, 4, 4, 1)
    header = uniio.make_header(4, 4, 4)
    with pytest.raises(uniio.UniError):
        uniio.writeUniFromDevice(str(tmp_path / "a.uni"), header, vol, codec="device")
    monkeypatch.setenv("MPG_UNI_CODEC", "device")
    with pytest.raises(uniio.UniError):
        uniio.writeUniFromDevice(str(tmp_path / "b.uni"), header, vol)
    with pytest.raises(uniio.UniError):
        uniio.writeUniFromDevice(str(tmp_path / "c.uni"), header, vol, codec="gpu")


def test_host_codec_and_default_are_unchanged(tmp_path, monkeypatch):
    monkeypatch.delenv("MPG_UNI_CODEC", raising=False)
    rng = np.random.default_rng(11)
    vol = torch.as_tensor(rng.standard_normal((5, 6, 7, 1)).astype(np.float32))
    header = uniio.make_header(7, 6, 5)
    uniio.writeUniFromDevice(str(tmp_path / "default.uni"), header, vol)
    uniio.writeUniFromDevice(str(tmp_path / "host.uni"), header, vol, codec="host")
    uniio.writeUni(str(tmp_path / "plain.uni"), header, vol.numpy())
    raws = [open(str(tmp_path / n), "rb").read() for n in ("default.uni", "host.uni", "plain.uni")]
    assert raws[0] == raws[1] == raws[2]
    for name in ("default.uni", "host.uni"):
        head, arr = uniio.readUni(str(tmp_path / name))
        assert head == header and np.array_equal(arr.view(np.uint32), vol.numpy().view(np.uint32))
    monkeypatch.setenv("MPG_UNI_CODEC", "host")
    uniio.writeUniFromDevice(str(tmp_path / "env.uni"), header, vol)
    assert open(str(tmp_path / "env.uni"), "rb").read() == raws[0]
