"""The per-unit Huffman mode of the device .uni codec, host side: tests/deflate_dynamic_ref.py (the restatement the
kernel is held to byte for byte in test_uni_dynamic_gpu.py) writes valid DEFLATE, never more than the fixed or stored
form, close to the host codec's size on a density, and its units go through uniio's member framing.  No GPU."""
import gzip
import heapq
import struct
import zlib

import numpy as np
import pytest

import mpgan_amd  # noqa: F401
from mpgan_amd import uniio

import deflate_dynamic_ref as R

W = R.UNIT // 4
CASES = R.cases()


def _inflate(streams):
    """raw inflate of unit streams closed with the empty final block"""
    d = zlib.decompressobj(-15)
    out = d.decompress(b"".join(streams) + uniio._FINAL_BLOCK)
    assert d.eof and d.unused_data == b""
    return out


def _units(words):
    return [words[a:a + W] for a in range(0, len(words), W)]


def test_constants_are_the_codecs():
    assert R.UNIT == uniio.UNIT and R.UNIT + 5 <= uniio.SLOT


@pytest.mark.parametrize("name", sorted(CASES))
def test_units_inflate_and_are_never_longer_than_fixed_or_stored(name):
    words = CASES[name]
    streams = R.encode_payload(words)
    assert len(streams) == -(-len(words) // W)
    for unit, stream in zip(_units(words), streams):
        assert _inflate([stream]) == unit.tobytes()
        fixed = len(R.encode_unit(unit, dynamic=False))
        assert fixed == min(R.fixed_size(unit), 5 + 4 * len(unit))
        assert len(stream) <= min(R.fixed_size(unit), 5 + 4 * len(unit))
        assert _inflate([R.encode_unit(unit, dynamic=False)]) == unit.tobytes()
    assert _inflate(streams) == words.tobytes()


def test_each_form_wins_somewhere():
    assert R.encode_unit(CASES["random_bits"])[:1] == b"\x00" and len(R.encode_unit(CASES["random_bits"])) == 5 + R.UNIT
    assert R.encode_unit(CASES["smooth"])[0] & 7 == 4                       # BFINAL 0, BTYPE 10
    tiny = np.full(8, 0x3f800000, np.uint32)                                # a header costs more than it saves
    assert R.encode_unit(tiny)[0] & 7 == 2 and R.encode_unit(tiny) == R.encode_unit(tiny, dynamic=False)
    assert _inflate([R.encode_unit(tiny)]) == tiny.tobytes()


def _unrestricted_depth(freq):
    heap = [(int(f), s, 0) for s, f in enumerate(freq) if f > 0]           # (weight, tie, depth below)
    heapq.heapify(heap)
    tie = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tie, max(a[2], b[2]) + 1))
        tie += 1
    return heap[0][2]


def test_length_limit_is_exercised():
    unit = CASES["fibonacci"]
    assert 4 * len(unit) == 6764 and not (unit[1:] == unit[:-1]).any()
    freq = R.histogram(unit)
    assert _unrestricted_depth(freq) > 15, "the unit must need the limiter"
    lengths = R.code_lengths(freq)
    assert max(lengths) == 15
    assert sum(2.0 ** -n for n in lengths if n) == 1.0, "a complete code"
    assert [n > 0 for n in lengths] == [f > 0 for f in freq]
    assert _inflate([R.encode_unit(unit)]) == unit.tobytes()


def test_codes_are_complete_and_ordered_on_every_case():
    for name, words in CASES.items():
        for unit in _units(words):
            freq = R.histogram(unit)
            lengths = R.code_lengths(freq)
            assert 1 <= max(lengths) <= 15 and sum(2.0 ** -n for n in lengths if n) == 1.0, name
            used = sorted((int(f), s) for s, f in enumerate(freq) if f > 0)
            by_rank = [lengths[s] for _, s in used]
            assert by_rank == sorted(by_rank, reverse=True), "a rarer symbol never gets the shorter code"


def test_run_lengths_cut_at_64_words():
    words = CASES["runs_63_64_65"]
    is_lit, closes, q = R.tokenise(words)
    got = sorted(int(x) for x in q[closes])
    # runs of 63, 64, 65, 1, 2, 128, 129 repeats
    assert got == sorted([63, 64, 64, 1, 1, 2, 64, 64, 64, 64, 1])
    assert R.length_symbol(64) == (284, 5, 29) and R.length_symbol(1) == (258, 0, 0) and R.length_symbol(3) == (265, 1, 1)


@pytest.fixture(scope="module")
def probe():
    vol = R.probe_volume(128)
    return vol.reshape(-1).view(np.uint32)


def test_size_against_the_host_codec(probe, tmp_path):
    """the 128^3 volume of tools/probe_uni.py: restated units + framing against the host codec's file"""
    assert probe.nbytes == 128 ** 3 * 4
    header = uniio.make_header(128, 128, 128)
    host = str(tmp_path / "host.uni")
    uniio.writeUni(host, header, probe.view(np.float32), level=6)
    host_bytes = len(open(host, "rb").read())
    units = _units(probe)
    sizes = [R.unit_size(u) for u in units]
    first = b"MNT3" + struct.pack(uniio._V4_FORMAT, *[header[k] for k in uniio._V4_FIELDS])
    members = -(-len(units) // uniio.MEMBER_UNITS)
    total = len(uniio._deflate_member(first, 6)) + sum(sizes) + members * (uniio._MEMBER_HEAD + len(uniio._FINAL_BLOCK) + 8)
    fixed = sum(R.unit_size(u, dynamic=False) for u in units)
    print("host %d B, dynamic units + framing %d B (%.4f), fixed units %d B (%.4f)"
          % (host_bytes, total, total / host_bytes, fixed, fixed / host_bytes))
    assert total <= 1.03 * host_bytes
    for k in (0, len(units) // 2, len(units) - 1):                         # the size model is the encoder's
        assert len(R.encode_unit(units[k])) == sizes[k]


def test_framing_of_restated_units(tmp_path):
    words = np.concatenate([CASES["smooth"], CASES["boundary_run_3units"][:2 * W], CASES["fibonacci"]])
    header = uniio.make_header(len(words), 1, 1)
    first = b"MNT3" + struct.pack(uniio._V4_FORMAT, *[header[k] for k in uniio._V4_FIELDS])
    units = _units(words)
    streams = [R.encode_unit(u) for u in units]
    path = str(tmp_path / "restated.uni")
    with open(path, "wb") as out:
        out.write(uniio._deflate_member(first, 6))
        uniio.write_unit_members(out, b"".join(streams), [len(s) for s in streams], [zlib.crc32(u.tobytes()) for u in units],
                                 [4 * len(u) for u in units], member_units=3)
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == first + words.tobytes()
    head, arr = uniio.readUni(path)
    assert head == header and np.array_equal(arr.reshape(-1).view(np.uint32), words)
    assert len(uniio._member_sizes(raw)) == 1 + 2


def test_codec_names(tmp_path, monkeypatch):
    import torch
    vol = torch.zeros(4, 4, 4, 1)
    header = uniio.make_header(4, 4, 4)
    with pytest.raises(uniio.UniError, match="GPU tensor"):                # a known codec: it gets as far as the tensor
        uniio.writeUniFromDevice(str(tmp_path / "a.uni"), header, vol, codec="device_dynamic")
    monkeypatch.setenv("MPG_UNI_CODEC", "device_dynamic")
    with pytest.raises(uniio.UniError, match="GPU tensor"):
        uniio.writeUniFromDevice(str(tmp_path / "b.uni"), header, vol)
    with pytest.raises(uniio.UniError) as err:
        uniio.writeUniFromDevice(str(tmp_path / "c.uni"), header, vol, codec="dynamic")
    for name in ("host", "device", "device_dynamic"):
        assert '"%s"' % name in str(err.value)
    from mpgan_amd import _lib
    assert "mpg_deflate_encode_dynamic" in _lib.PROTOTYPES
