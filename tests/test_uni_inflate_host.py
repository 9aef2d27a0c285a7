"""The unit index of device-coded .uni files and the decode core of the device reader, host side.  The index is an opt-in
second subfield (MU) of every payload member; files without it do not change by a byte, files with it read everywhere.  The
decode core (csrc/mpgan_inflate_core.h) runs here as a stand-alone CPU program under AddressSanitizer and UBSan, on every
stream of the writer's language and on a malformed set.  No GPU."""
import gzip
import io
import struct
import zlib

import numpy as np
import pytest

import mpgan_amd  # noqa: F401
from mpgan_amd import uniio

import deflate_dynamic_ref as R
import uni_inflate_ref as U

CASES = R.cases()


def _write(tmp_path, name, blob):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(blob)
    return path


@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_indexed_file_reads_everywhere_and_costs_only_the_index(tmp_path, name, dynamic):
    words = CASES[name]
    streams, sources = U.payload_streams(words, dynamic)
    for member_units in (256, 2):
        plain = U.member_file(streams, sources, False, member_units)
        indexed = U.member_file(streams, sources, True, member_units)
        groups = [streams[a:a + member_units] for a in range(0, len(streams), member_units)]
        # the sizes that went in come out, with the offset of every member's body
        index = uniio.unit_index(indexed)
        assert [sizes for _, sizes in index] == [[len(s) for s in g] for g in groups]
        for (body, sizes), g in zip(index, groups):
            assert indexed[body:body + sum(sizes)] == b"".join(g)
        assert uniio.unit_index(plain) is None
        # exactly 4 + 4 k bytes per member, everything else as without the index
        assert len(indexed) == len(plain) + sum(4 + 4 * len(g) for g in groups)
        assert uniio._member_sizes(indexed) is not None and len(uniio._member_sizes(indexed)) == 1 + len(groups)
        at_p, at_i = uniio._member_sizes(plain)[0], uniio._member_sizes(indexed)[0]
        assert plain[:at_p] == indexed[:at_i]                       # the header member carries no index
        for g, size_p, size_i in zip(groups, uniio._member_sizes(plain)[1:], uniio._member_sizes(indexed)[1:]):
            extra = 4 + 4 * len(g)
            assert size_i == size_p + extra
            assert indexed[at_i:at_i + 10] == plain[at_p:at_p + 10]
            assert struct.unpack_from("<H", indexed, at_i + 10)[0] == 8 + extra and struct.unpack_from("<H", plain, at_p + 10)[0] == 8
            assert indexed[at_i + 12:at_i + 16] == plain[at_p + 12:at_p + 16] == b"MP\x04\x00"
            assert indexed[at_i + 20:at_i + 24] == b"MU" + struct.pack("<H", 4 * len(g))
            assert indexed[at_i + 20 + extra:at_i + size_i] == plain[at_p + 20:at_p + size_p]
            at_p, at_i = at_p + size_p, at_i + size_i
        # every reader gets the payload
        for blob in (plain, indexed):
            assert gzip.decompress(blob)[4 + uniio.HEADER_BYTES:] == words.tobytes()
            with gzip.open(io.BytesIO(blob), "rb") as f:             # the reference's reader
                assert f.read()[4 + uniio.HEADER_BYTES:] == words.tobytes()


def test_readUni_reads_an_indexed_file(tmp_path):
    words = CASES["boundary_run_3units"]                             # 16424 words: two units and a short third
    vol = words.view(np.float32).reshape(1, 8, 2053, 1)
    head = uniio.make_header(2053, 8, 1)
    for dynamic in (False, True):
        streams, sources = U.payload_streams(words, dynamic)
        first = uniio._deflate_member(b"MNT3" + struct.pack(uniio._V4_FORMAT, *[head[k] for k in uniio._V4_FIELDS]), 6)
        for flag in (False, True):
            buf = io.BytesIO()
            uniio.write_unit_members(buf, b"".join(streams), [len(s) for s in streams], [zlib.crc32(x) for x in sources],
                                     [len(x) for x in sources], member_units=2, unit_index=flag)
            path = _write(tmp_path, "v_%d_%d.uni" % (dynamic, flag), first + buf.getvalue())
            for threads in (1, 4):
                got_head, got = uniio.readUni(path, threads=threads)
                assert got_head == head and got.dtype == np.float32
                assert np.array_equal(got.view(np.uint32), vol.view(np.uint32))


def test_default_is_off_and_limits_raise():
    streams, sources = U.payload_streams(CASES["special_bits"], True)
    args = (b"".join(streams), [len(s) for s in streams], [zlib.crc32(x) for x in sources], [len(x) for x in sources])
    a, b = io.BytesIO(), io.BytesIO()
    uniio.write_unit_members(a, *args)
    uniio.write_unit_members(b, *args, unit_index=False)
    assert a.getvalue() == b.getvalue() and b"MU" not in a.getvalue()[:24]
    # 16380 units fill the extra field, one more does not fit
    n = uniio.MAX_INDEX_UNITS
    assert n == 16380
    tiny = R.encode_unit(np.zeros(1, np.uint32), False)
    ok = io.BytesIO()
    uniio.write_unit_members(ok, tiny * n, [len(tiny)] * n, [zlib.crc32(b"\0" * 4)] * n, [4] * n, member_units=n, unit_index=True)
    assert struct.unpack_from("<H", ok.getvalue(), 10)[0] == 8 + 4 + 4 * n <= 65535
    assert gzip.decompress(ok.getvalue()) == b"\0" * (4 * n)
    with pytest.raises(uniio.UniError):
        uniio.write_unit_members(io.BytesIO(), tiny * (n + 1), [len(tiny)] * (n + 1), [zlib.crc32(b"\0" * 4)] * (n + 1), [4] * (n + 1),
                                 member_units=n + 1, unit_index=True)
    # the same units without the index are no error
    uniio.write_unit_members(io.BytesIO(), tiny * (n + 1), [len(tiny)] * (n + 1), [zlib.crc32(b"\0" * 4)] * (n + 1), [4] * (n + 1),
                             member_units=n + 1)


def test_host_codec_with_index_raises(tmp_path, monkeypatch):
    import torch
    head = uniio.make_header(4, 4, 4)
    vol = torch.zeros(4, 4, 4, 1)
    with pytest.raises(uniio.UniError):
        uniio.writeUniFromDevice(str(tmp_path / "a.uni"), head, vol, codec="host", unit_index=True)
    monkeypatch.setenv("MPG_UNI_INDEX", "1")
    with pytest.raises(uniio.UniError):
        uniio.writeUniFromDevice(str(tmp_path / "b.uni"), head, vol, codec="host")
    monkeypatch.setenv("MPG_UNI_INDEX", "0")
    uniio.writeUniFromDevice(str(tmp_path / "c.uni"), head, vol, codec="host")
    monkeypatch.delenv("MPG_UNI_INDEX")
    uniio.writeUniFromDevice(str(tmp_path / "d.uni"), head, vol, codec="host")
    assert open(str(tmp_path / "c.uni"), "rb").read() == open(str(tmp_path / "d.uni"), "rb").read()


def test_unit_index_is_none_without_a_full_index(tmp_path):
    path = str(tmp_path / "host.uni")
    uniio.writeUni(path, uniio.make_header(16, 16, 16), np.arange(4096, dtype=np.float32))
    assert uniio.unit_index(open(path, "rb").read()) is None
    assert uniio.unit_index(gzip.compress(b"MNT3" + b"\0" * 400)) is None      # a foreign single-member file
    streams, sources = U.payload_streams(CASES["boundary_run_3units"], True)
    indexed = U.member_file(streams, sources, True, member_units=1)
    plain = U.member_file(streams, sources, False, member_units=1)
    assert len(uniio.unit_index(indexed)) == 3
    si, sp = uniio._member_sizes(indexed), uniio._member_sizes(plain)
    # the second payload member replaced by its twin without MU
    a_i, a_p = si[0] + si[1], sp[0] + sp[1]
    mixed = indexed[:a_i] + plain[a_p:a_p + sp[2]] + indexed[a_i + si[2]:]
    assert gzip.decompress(mixed) == gzip.decompress(indexed)
    assert uniio.unit_index(mixed) is None


# ---------------------------------------------------------------- the decode core as a CPU program under ASan + UBSan
def test_core_decodes_every_case_under_the_sanitizers():
    good = U.good_streams()
    records = [((3 * k) % 16, stream, len(src)) for k, (_, _, _, stream, src) in enumerate(good)]
    results, _ = U.run_program(records)
    forms = set()
    for (name, dynamic, unit, stream, src), (status, crc, out) in zip(good, results):
        assert status == 0, (name, dynamic, unit, status)
        assert out == src, (name, dynamic, unit)
        assert crc == zlib.crc32(src)
        forms.add(stream[0] & 7)
    assert forms == {0, 2, 4}                                        # stored, fixed and dynamic blocks all met


def test_core_on_every_lead_and_tiny_outputs():
    words = CASES["runs_63_64_65"]
    records, want = [], []
    for lead in range(16):
        for n in (1, 2, 5, len(words)):
            for dynamic in (False, True):
                records.append((lead, R.encode_unit(words[:n], dynamic), 4 * n))
                want.append(words[:n].tobytes())
    results, _ = U.run_program(records)
    for (status, crc, out), src in zip(results, want):
        assert status == 0 and out == src and crc == zlib.crc32(src)
    # the right stream with the wrong output length is an error, not an overrun
    s = R.encode_unit(words, True)
    results, _ = U.run_program([(0, s, 4 * len(words) - 4), (0, s, 4 * len(words) + 4), (5, s, 0), (5, b"", 0), (5, b"", 4)])
    assert [r[0] != 0 for r in results] == [True, True, True, False, True]


def test_core_malformed_set_under_the_sanitizers():
    bad = U.malformed_streams()
    assert len(bad) == 2 * 2 * 72 + 200 * len(CASES) + 3
    results, _ = U.run_program([((7 * k) % 16, stream, n) for k, (_, stream, n) in enumerate(bad)])
    for (label, stream, n), (status, crc, out) in zip(bad, results):
        assert len(out) <= n, label
        if status == 0:
            assert len(out) == n and out == U.zlib_view(stream), label
            assert crc == zlib.crc32(out), label
    by_label = {label: r[0] for (label, _, _), r in zip(bad, results)}
    for label, _, _ in U.gpu_malformed():
        assert by_label[label] != 0, label
    assert by_label["zlib6/smooth"] == 1 and by_label["all_ff"] != 0 and by_label["all_zero"] == 2
