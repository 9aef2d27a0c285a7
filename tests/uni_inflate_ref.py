"""Shared by test_uni_inflate_host.py and test_uni_inflate_gpu.py: the unit streams of deflate_dynamic_ref.cases() in both
modes, the malformed set, and the decode core of csrc/mpgan_inflate_core.h built as a stand-alone CPU program under
AddressSanitizer and UBSan (tools/inflate_core_host.cpp; nothing is preloaded, the program has its own main)."""
import atexit
import functools
import os
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np

import deflate_dynamic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = R.UNIT


@functools.lru_cache(maxsize=None)
def good_streams():
    """[(name, dynamic, unit number, stream bytes, source bytes)] over every case and both modes"""
    out = []
    for name, words in R.cases().items():
        for dynamic in (False, True):
            for k, a in enumerate(range(0, len(words), UNIT // 4)):
                part = words[a:a + UNIT // 4]
                out.append((name, dynamic, k, R.encode_unit(part, dynamic), part.tobytes()))
    return out


def _stream_of(name, dynamic, unit=0):
    for n, d, k, s, src in good_streams():
        if (n, d, k) == (name, dynamic, unit):
            return s, src
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def malformed_streams():
    """[(label, stream bytes, out_bytes)]: the malformed set of the decoder's tests"""
    out = []
    for name in ("fibonacci", "runs_63_64_65"):
        for dynamic in (False, True):
            s, src = _stream_of(name, dynamic)
            for cut in list(range(64)) + list(range(len(s) - 8, len(s))):
                out.append(("%s/%d/cut%d" % (name, dynamic, cut), s[:cut], len(src)))
    for name in R.cases():
        s, src = _stream_of(name, True)
        for bit in range(200):
            b = bytearray(s)
            b[bit >> 3] ^= 1 << (bit & 7)
            out.append(("%s/flip%d" % (name, bit), bytes(b), len(src)))
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    smooth = R.cases()["smooth"].tobytes()
    out.append(("zlib6/smooth", co.compress(smooth) + co.flush(zlib.Z_SYNC_FLUSH), len(smooth)))
    out.append(("all_ff", b"\xff" * 100, 4096))
    out.append(("all_zero", b"\0" * 100, 4096))
    return out


def gpu_malformed():
    """a fixed dozen of the set above for the GPU: truncations at both ends, header and token bit flips, foreign streams"""
    last = len(_stream_of("runs_63_64_65", False)[0]) - 1
    labels = ("fibonacci/1/cut10", "fibonacci/1/cut40", "fibonacci/0/cut3", "runs_63_64_65/1/cut63", "runs_63_64_65/0/cut%d" % last,
              "smooth/flip3", "smooth/flip17", "smooth/flip60", "fibonacci/flip150", "zlib6/smooth", "all_ff", "all_zero")
    table = {label: (stream, n) for label, stream, n in malformed_streams()}
    return [(label,) + table[label] for label in labels]


def zlib_view(stream):
    """what zlib makes of a raw, non-final stream: its output, or None where it objects"""
    try:
        return zlib.decompressobj(-15).decompress(stream)
    except zlib.error:
        return None


_PROGRAM = {}


def build_program():
    """path of the sanitizer build of tools/inflate_core_host.cpp (built once per process), or None without a compiler"""
    if "path" not in _PROGRAM:
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
        path = None
        if cxx:
            d = tempfile.mkdtemp(prefix="mpg_inflate_core_")
            atexit.register(shutil.rmtree, d, True)
            path = os.path.join(d, "inflate_core_host")
            # the sanitizer runtime is linked into the program (clang's default): it has to be the first thing loaded
            static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
            subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                            "-I", os.path.join(ROOT, "multi-pass-gan_amd", "csrc"), os.path.join(ROOT, "tools", "inflate_core_host.cpp"),
                "-o", path], check=True)
        _PROGRAM["path"] = path
    return _PROGRAM["path"]


def run_program(records):
    """records: [(lead, stream, out_bytes)] -> ([(status, crc, output bytes)], the program's stderr).  A sanitizer report
    ends the program with a non-zero exit status, which raises here."""
    prog = build_program()
    assert prog, "no C++ compiler"
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "streams.bin"), os.path.join(d, "results.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(records)))
            for lead, s, n in records:
                f.write(struct.pack("<III", lead, len(s), n))
                f.write(s)
        p = subprocess.run([prog, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = p.stderr.decode(errors="replace")
        assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
        raw = open(dst, "rb").read()
    out, at = [], 0
    for _ in records:
        status, crc, n = struct.unpack_from("<III", raw, at)
        out.append((status, crc, raw[at + 12:at + 12 + n]))
        at += 12 + n
    assert at == len(raw)
    return out, err


def member_file(streams, sources, unit_index, member_units=256):
    """bytes of a .uni-style file: a header member, then the streams framed by uniio.write_unit_members"""
    import io
    from mpgan_amd import uniio
    buf = io.BytesIO()
    buf.write(uniio._deflate_member(b"MNT3" + b"\0" * uniio.HEADER_BYTES, 6))
    uniio.write_unit_members(buf, b"".join(streams), [len(s) for s in streams], [zlib.crc32(x) for x in sources],
                             [len(x) for x in sources], member_units=member_units, unit_index=unit_index)
    return buf.getvalue()


def payload_streams(words, dynamic):
    words = np.asarray(words, np.uint32)
    return R.encode_payload(words, dynamic), [words[a:a + UNIT // 4].tobytes() for a in range(0, len(words), UNIT // 4)]
