"""mantaflow ``.uni`` grid files: same functions and header dictionary as the
reference's ``tools_wscale/uniio.py`` (readUni :81-88, writeUni :91-123).

File = gzip stream of: 4-byte magic (b"MNT2" or b"MNT3"), a 288-byte header,
then the raw C-order payload [dimZ, dimY, dimX, channels] of float32 (scalar:
elementType 1, 4 bytes/element; vec3: elementType 2, 12 bytes/element) or int32
(elementType 0).  Files are always written as MNT3.  Large grids stream through a chunked, multi-threaded codec
(below) whose output every gzip reader, the reference's included, decodes to the same bytes.  writeUniFromDevice can
instead deflate the payload on the GPU (codecs "device" and "device_dynamic", further below): same bytes after
inflation; the fixed-code files are larger, those with a Huffman code per unit about the host codec's size.
"""
import concurrent.futures
import gzip
import io
import os
import shutil
import struct
import zlib

import numpy as np

_V4_FIELDS = ("dimX", "dimY", "dimZ", "gridType", "elementType", "bytesPerElement", "info", "dimT", "timestamp")
_V4_FORMAT = "iiiiii252siQ"      # MNT3, uniio.py:67
_V3_FORMAT = "iiiiii256sQ"       # MNT2, uniio.py:56
HEADER_BYTES = 288


class UniError(Exception):
    pass


def _parse_header(stream):
    magic = stream.read(4)
    raw = stream.read(HEADER_BYTES)
    if len(raw) != HEADER_BYTES:
        raise UniError("truncated .uni header")
    if magic == b"MNT3":
        head = dict(zip(_V4_FIELDS, struct.unpack(_V4_FORMAT, raw)))
    elif magic == b"MNT2":
        dx, dy, dz, gt, et, bpe, info, ts = struct.unpack(_V3_FORMAT, raw)
        # re-packed as a v4 header with dimT = 0 and the info string cut to 252 bytes (uniio.py:58-62)
        head = dict(zip(_V4_FIELDS, (dx, dy, dz, gt, et, bpe, info[0:252], 0, ts)))
    elif magic in (b"M4T2", b"M4T3"):
        raise UniError("4D .uni grids are not supported (uniio.py:69-71)")
    else:
        raise UniError("unknown .uni header %r" % (magic,))
    return head


def _parse_content(stream, head):
    et, bpe = head["elementType"], head["bytesPerElement"]
    if not ((bpe == 12 and et == 2) or (bpe == 4 and et in (0, 1))):
        raise UniError("unsupported element type %d with %d bytes per element" % (et, bpe))
    data = np.frombuffer(stream.read(), dtype="int32" if et == 0 else "float32")
    channels = 3 if et == 2 else 1
    dims = [head["dimZ"], head["dimY"], head["dimX"], channels]
    if head["dimT"] > 1:
        dims = [head["dimT"]] + dims
    return data.reshape(dims)


# ----------------------------------------------------------------------------------------------
# streaming codec.  A .uni file is ONE gzip stream for the reference (gzip.open(...).read()); RFC 1952 lets such a
# stream be a sequence of members, which every gzip reader -- the reference's included -- concatenates.  Volumes are
# therefore written as independently deflated chunks (one member each, compressed on a thread pool: zlib releases
# the GIL), and each member carries its own compressed size in a gzip "extra" subfield (the BGZF idea), so that this
# reader can find the members without inflating them and inflate them in parallel.  Files from other writers (one
# member, no subfield) are read as a plain stream.  A 512^3 volume is 537 MB: single-threaded level-9 deflate (the
# reference's gzip.open default) takes tens of seconds, longer than the three network passes that produce it.
# ----------------------------------------------------------------------------------------------
CHUNK_BYTES = 8 << 20
_SUBFIELD = b"MP"                 # extra-field subfield id: uint32 member size (header + deflate data + trailer)
_MEMBER_HEAD = 10 + 2 + 4 + 4     # fixed header, XLEN, subfield header, subfield payload


def _threads(threads):
    if threads is None:
        threads = int(os.environ.get("MPG_UNI_THREADS", "0")) or min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    return max(1, int(threads))


def _deflate_member(buf, level):
    """one gzip member for `buf`, its total size recorded in the extra field"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(buf) + co.flush()
    total = _MEMBER_HEAD + len(body) + 8
    head = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 255, 8) + _SUBFIELD + struct.pack("<HI", 4, total)
    return head + body + struct.pack("<II", zlib.crc32(buf) & 0xffffffff, len(buf) & 0xffffffff)


def _member_sizes(raw):
    """sizes of the members of a file written by writeUni, or None if it is not one"""
    sizes, at = [], 0
    n = len(raw)
    while at < n:
        if n - at < _MEMBER_HEAD or raw[at:at + 4] != b"\x1f\x8b\x08\x04" or raw[at + 12:at + 14] != _SUBFIELD:
            return None
        (size,) = struct.unpack_from("<I", raw, at + 16)
        if size < _MEMBER_HEAD + 8 or at + size > n:
            return None
        sizes.append(size)
        at += size
    return sizes


def _body_start(raw, at):
    """offset of the deflate body of the member at `at`: behind the fixed header, XLEN and the extra field"""
    return at + 12 + struct.unpack_from("<H", raw, at + 10)[0]


def _inflate_member(raw, at, size):
    data = zlib.decompress(raw[_body_start(raw, at):at + size - 8], -15)
    crc, isize = struct.unpack_from("<II", raw, at + size - 8)
    if (zlib.crc32(data) & 0xffffffff) != crc or (len(data) & 0xffffffff) != isize:
        raise UniError("corrupt gzip member at offset %d" % at)
    return data


def readUni(filename, threads=None):
    """-> (header dict, ndarray [Z,Y,X,C]).  Members written by writeUni are inflated in parallel."""
    with open(filename, "rb") as f:
        raw = f.read()
    sizes = _member_sizes(raw)
    if sizes is None:                       # a foreign writer (the reference, mantaflow): plain gzip stream
        with gzip.open(io.BytesIO(raw), "rb") as stream:
            head = _parse_header(stream)
            return head, _parse_content(stream, head)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    nthreads = min(_threads(threads), len(sizes))
    if nthreads > 1:
        with concurrent.futures.ThreadPoolExecutor(nthreads) as pool:
            parts = list(pool.map(lambda a: _inflate_member(raw, a[0], a[1]), zip(offs, sizes)))
    else:
        parts = [_inflate_member(raw, o, z) for o, z in zip(offs, sizes)]
    stream = io.BytesIO(b"".join(parts))
    head = _parse_header(stream)
    return head, _parse_content(stream, head)


def writeUni(filename, header, content, level=None, threads=None, chunk_bytes=CHUNK_BYTES):
    """header: dict as returned by readUni (field order as in the file); content: array with dimX*dimY*dimZ (*3 for
    vec3) elements, converted to float32.  The decompressed bytes are those of the reference writer; the container is
    a multi-member gzip stream (see above).  level: deflate level (default MPG_UNI_LEVEL or 6; the reference's 9)."""
    if level is None:
        level = int(os.environ.get("MPG_UNI_LEVEL", "6"))
    content = np.asarray(content)
    if content.dtype != np.float32:
        content = content.astype(np.float32)
    n = header["dimX"] * header["dimY"] * header["dimZ"] * (3 if header["elementType"] == 2 else 1)
    payload = memoryview(np.ascontiguousarray(content).reshape(n)).cast("B")
    first = b"MNT3" + struct.pack(_V4_FORMAT, *[header[k] for k in _V4_FIELDS])
    cuts = list(range(0, len(payload), chunk_bytes)) or [0]
    pieces = [payload[c:c + chunk_bytes] for c in cuts]

    def member(i):
        return _deflate_member(first + bytes(pieces[0]) if i == 0 else pieces[i], level)

    nthreads = min(_threads(threads), len(pieces))
    with open(filename, "wb") as out:
        if nthreads > 1:
            with concurrent.futures.ThreadPoolExecutor(nthreads) as pool:
                for blob in pool.map(member, range(len(pieces))):       # in order; members stream out as they finish
                    out.write(blob)
        else:
            for i in range(len(pieces)):
                out.write(member(i))


def writeUniFromDevice(filename, header, volume, level=None, threads=None, chunk_bytes=CHUNK_BYTES, codec=None, unit_index=None):
    """writeUni for a float32 CUDA tensor: the volume is copied to pinned host memory chunk by chunk on a side stream
    while the previous chunks are being deflated, so neither the 537 MB device-to-host copy of a 512^3 volume nor its
    compression waits for the other.  codec: "host" (zlib on the thread pool, the default), "device" (deflated by
    HIP kernels with the fixed Huffman code, only compressed bytes cross to the host; larger files, see _write_device)
    or "device_dynamic" (the same with a Huffman code per unit: files about as small as the host's);
    None = MPG_UNI_CODEC.  unit_index (device codecs only): record the unit sizes in every member, see write_unit_members;
    None = MPG_UNI_INDEX ("1" = on), off when unset."""
    import torch
    if level is None:
        level = int(os.environ.get("MPG_UNI_LEVEL", "6"))
    if codec is None:
        codec = os.environ.get("MPG_UNI_CODEC", "") or "host"
    if codec not in ("host", "device", "device_dynamic"):
        raise UniError("unknown codec %r: expected \"host\", \"device\" or \"device_dynamic\"" % (codec,))
    if unit_index is None:
        unit_index = os.environ.get("MPG_UNI_INDEX", "") == "1"
    if codec != "host":
        return _write_device(filename, header, volume, level, dynamic=codec == "device_dynamic", unit_index=bool(unit_index))
    if unit_index:
        raise UniError("the unit index needs a device codec: codec \"host\" writes no units")
    flat = volume.contiguous().reshape(-1)
    if flat.dtype != torch.float32:
        flat = flat.float()
    n = header["dimX"] * header["dimY"] * header["dimZ"] * (3 if header["elementType"] == 2 else 1)
    if flat.numel() != n:
        raise UniError("volume has %d elements, header describes %d" % (flat.numel(), n))
    per = max(1, chunk_bytes // 4)
    cuts = list(range(0, n, per)) or [0]
    host = torch.empty(n, dtype=torch.float32, pin_memory=flat.is_cuda)
    side = torch.cuda.Stream(device=flat.device) if flat.is_cuda else None
    events = []
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(flat.device))
        with torch.cuda.stream(side):
            for c in cuts:
                host[c:c + per].copy_(flat[c:c + per], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
                events.append(ev)
    else:
        host.copy_(flat)
    view = memoryview(host.numpy()).cast("B")
    first = b"MNT3" + struct.pack(_V4_FORMAT, *[header[k] for k in _V4_FIELDS])

    def member(i):
        if events:
            events[i].synchronize()
        piece = view[cuts[i] * 4:(cuts[i] + per) * 4]
        return _deflate_member(first + bytes(piece) if i == 0 else piece, level)

    nthreads = min(_threads(threads), len(cuts))
    with open(filename, "wb") as out, concurrent.futures.ThreadPoolExecutor(nthreads) as pool:
        for blob in pool.map(member, range(len(cuts))):
            out.write(blob)


# ----------------------------------------------------------------------------------------------
# device codec.  ops.deflate_encode turns every UNIT bytes of the payload into a byte-aligned, non-final raw DEFLATE
# stream (fixed Huffman code over word-granular runs, or a stored block; codec "device_dynamic": or the same tokens under
# a Huffman code of the unit's own, whichever of the three is shortest) and the CRC-32 of those bytes; the streams of
# consecutive units concatenate into a valid deflate body, which an empty final block closes.  The host only frames
# members around bodies it never inflates: MEMBER_UNITS units each, the CRCs of their units combined.
# ----------------------------------------------------------------------------------------------
UNIT = 32768                      # payload bytes per device-encoded unit (MPG_DEFLATE_UNIT)
SLOT = UNIT + 16                  # workspace bytes per unit (MPG_DEFLATE_SLOT)
SLAB_BYTES = 64 << 20             # payload bytes per encode call (MPG_DEFLATE_SLAB): bounds the workspace
MEMBER_UNITS = CHUNK_BYTES // UNIT    # units per gzip member: members as large as the host codec's, so readUni's
#                                       thread pool gets the same work items either way
_FINAL_BLOCK = b"\x03\x00"        # BFINAL 1, BTYPE 01, end-of-block: an empty last block
_UNIT_SUBFIELD = b"MU"            # second extra-field subfield, opt-in: uint32 stream length of every unit of the member
MAX_INDEX_UNITS = 16380           # 8 + 4 + 4 * k <= 65535, the most an extra field holds
_CRC_POLY = 0xEDB88320


def _gf_mul(a, b):
    """a * b mod the CRC-32 polynomial, bit-reflected (bit 31 is x^0), as zlib's multmodp"""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (_CRC_POLY if b & 1 else 0)
    return p


_SHIFT_TABLES = {}


def _crc_shift_tables(nbytes):
    """four 256-entry tables: the CRC register `c` moved past nbytes zero bytes is T0[c & 255] ^ T1[c >> 8 & 255] ^ ..."""
    tabs = _SHIFT_TABLES.get(nbytes)
    if tabs is None:
        xp, sq, n = 0x80000000, 0x00800000, nbytes          # x^0; x^8
        while n:
            if n & 1:
                xp = _gf_mul(xp, sq)
            sq = _gf_mul(sq, sq)
            n >>= 1
        basis = [_gf_mul(1 << k, xp) for k in range(32)]
        tabs = []
        for byte in range(4):
            t = [0] * 256
            for v in range(1, 256):
                low = v & -v
                t[v] = t[v ^ low] ^ basis[8 * byte + low.bit_length() - 1]
            tabs.append(t)
        if len(_SHIFT_TABLES) < 64:
            _SHIFT_TABLES[nbytes] = tabs
    return tabs


def crc32_combine(crcs, lengths):
    """zlib.crc32 of the concatenation of pieces, from the pieces' own CRC-32s and byte lengths"""
    crc = 0
    for c, n in zip(crcs, lengths):
        if n:
            t0, t1, t2, t3 = _crc_shift_tables(int(n))
            crc = t0[crc & 255] ^ t1[(crc >> 8) & 255] ^ t2[(crc >> 16) & 255] ^ t3[crc >> 24]
        crc ^= int(c) & 0xffffffff
    return crc


def _frame_member(body_len, crc, isize, unit_sizes=None):
    """(head, tail) of a gzip member around a deflate body of body_len bytes that lacks its final block.  unit_sizes:
    the stream lengths of the member's units, recorded in an MU subfield behind the MP one (the unit index)"""
    index = b""
    if unit_sizes is not None:
        if len(unit_sizes) > MAX_INDEX_UNITS:
            raise UniError("%d units in one member: the unit index holds at most %d" % (len(unit_sizes), MAX_INDEX_UNITS))
        index = _UNIT_SUBFIELD + struct.pack("<H%dI" % len(unit_sizes), 4 * len(unit_sizes), *unit_sizes)
    total = _MEMBER_HEAD + len(index) + body_len + len(_FINAL_BLOCK) + 8
    head = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 255, 8 + len(index)) + _SUBFIELD + struct.pack("<HI", 4, total) + index
    return head, _FINAL_BLOCK + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def write_unit_members(out, bodies, sizes, crcs, lengths, member_units=MEMBER_UNITS, unit_index=False):
    """Write gzip members for device-encoded units to the file object `out`.  bodies: the unit streams back to back
    (bytes-like), sizes[u] the stream length of unit u, crcs[u] / lengths[u] the CRC-32 and byte count of its input.
    Every member holds up to member_units units and carries the MP size subfield and a CRC-32 / ISIZE trailer.
    unit_index: every member also records the stream lengths of its units (MU subfield, 4 + 4 * units bytes), which lets
    readUniToDevice inflate the units in parallel on the GPU; every gzip reader skips the subfield."""
    bodies = memoryview(bodies).cast("B")
    sizes = [int(x) for x in sizes]
    lengths = [int(x) for x in lengths]
    at = 0
    for a in range(0, len(sizes), member_units):
        b = min(a + member_units, len(sizes))
        body_len = sum(sizes[a:b])
        head, tail = _frame_member(body_len, crc32_combine(crcs[a:b], lengths[a:b]), sum(lengths[a:b]),
                                   sizes[a:b] if unit_index else None)
        out.write(head)
        out.write(bodies[at:at + body_len])
        out.write(tail)
        at += body_len
    if at != len(bodies):
        raise UniError("unit sizes describe %d bytes, %d were given" % (at, len(bodies)))


def _write_device(filename, header, volume, level, dynamic=False, unit_index=False):
    """The device codecs of writeUniFromDevice (dynamic: a Huffman code per unit).  The payload is encoded in slabs of SLAB_BYTES on the caller's current
    stream (one slot workspace, reused in stream order); each slab's compacted streams go to pinned memory on a side
    stream while the next slab is being encoded, so only compressed bytes cross to the host."""
    import torch
    if not (isinstance(volume, torch.Tensor) and volume.is_cuda):
        raise UniError("codec \"%s\" needs a GPU tensor" % ("device_dynamic" if dynamic else "device"))
    from . import ops
    flat = volume.contiguous().reshape(-1)
    if flat.dtype != torch.float32:
        flat = flat.float()
    n = header["dimX"] * header["dimY"] * header["dimZ"] * (3 if header["elementType"] == 2 else 1)
    if flat.numel() != n:
        raise UniError("volume has %d elements, header describes %d" % (flat.numel(), n))
    if flat.data_ptr() % 16:
        flat = flat.clone()
    dev = flat.device
    per = SLAB_BYTES // 4
    cuts = list(range(0, n, per))
    first = b"MNT3" + struct.pack(_V4_FORMAT, *[header[k] for k in _V4_FIELDS])
    with open(filename, "wb") as out, torch.cuda.device(dev):
        out.write(_deflate_member(first, level))
        if not cuts:
            return
        main = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        cap_units = (min(n, per) * 4 + UNIT - 1) // UNIT
        slots = torch.empty(cap_units * SLOT, dtype=torch.uint8, device=dev)
        bufs = []
        for _ in range(min(2, len(cuts))):
            bufs.append(dict(
                packed=torch.empty(cap_units * SLOT, dtype=torch.uint8, device=dev),
                meta=torch.empty(2, cap_units, dtype=torch.int32, device=dev),
                host_meta=torch.empty(2, cap_units, dtype=torch.int32, pin_memory=True),
                host=torch.empty(cap_units * SLOT, dtype=torch.uint8, pin_memory=True),
                done=torch.cuda.Event()))

        def launch(k):
            buf = bufs[k % 2]
            piece = flat[cuts[k]:cuts[k] + per]
            units = (piece.numel() * 4 + UNIT - 1) // UNIT
            ops.deflate_encode(piece, slots, buf["meta"][0], buf["meta"][1], dynamic=dynamic)
            ops.deflate_compact(slots, buf["meta"][0], units, buf["packed"])
            buf["done"].record(main)
            return units

        pending = launch(0)
        for k in range(len(cuts)):
            units, buf = pending, bufs[k % 2]
            if k + 1 < len(cuts):
                pending = launch(k + 1)         # the other buffer: its previous slab has been written out below
            with torch.cuda.stream(side):
                side.wait_event(buf["done"])
                buf["host_meta"].copy_(buf["meta"], non_blocking=True)
                side.synchronize()
                meta = buf["host_meta"][:, :units].numpy().view(np.uint32)
                total = int(meta[0].sum(dtype=np.int64))
                buf["host"][:total].copy_(buf["packed"][:total], non_blocking=True)
                side.synchronize()
            nbytes = min(per, n - cuts[k]) * 4
            lengths = [UNIT] * (units - 1) + [nbytes - UNIT * (units - 1)]
            write_unit_members(out, buf["host"][:total].numpy(), meta[0], meta[1], lengths, unit_index=unit_index)
        # `flat`, the workspace and the pinned buffers are released only now: every copy has completed


# ----------------------------------------------------------------------------------------------
# device reader.  With the unit index a reader knows where every unit stream starts without inflating anything, and the
# streams are independent, so ops.inflate_units decodes all units of a file in one launch.  The host keeps what it is good
# at: the member walk, the 292-byte header member, and the trailer check (unit CRCs combined per member).
# ----------------------------------------------------------------------------------------------
def unit_index(raw):
    """[(body offset, [unit stream sizes])] for the payload members (all but the first) of the bytes of a .uni file written
    with unit_index=True; None if the file has no member sizes or any payload member lacks the MU subfield"""
    raw = memoryview(raw).cast("B")
    sizes = _member_sizes(raw)
    if sizes is None or len(sizes) < 2:
        return None
    out, at = [], sizes[0]
    for size in sizes[1:]:
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        if xlen < 12 or bytes(raw[at + 20:at + 22]) != _UNIT_SUBFIELD:
            return None
        (nbytes,) = struct.unpack_from("<H", raw, at + 22)
        if nbytes % 4 or 12 + nbytes != xlen or at + 12 + xlen + len(_FINAL_BLOCK) + 8 > at + size:
            return None
        out.append((at + 12 + xlen, list(struct.unpack_from("<%dI" % (nbytes // 4), raw, at + 24))))
        at += size
    return out


def _device_plan(raw):
    """(header, dims, offsets, sizes, members) for the device path of readUniToDevice, or a string: why it does not apply.
    members: (first unit, one past the last, CRC-32, ISIZE) of every payload member"""
    member_sizes = _member_sizes(raw)
    if member_sizes is None:
        return "no member sizes: not written by this package"
    index = unit_index(raw)
    if index is None:
        return "no unit index"
    first_xlen = struct.unpack_from("<H", raw, 10)[0]
    if first_xlen != 8:
        return "the first member is not a plain header member"
    try:
        first = _inflate_member(raw, 0, member_sizes[0])
    except (UniError, zlib.error):
        return "the header member does not inflate"
    if len(first) != 4 + HEADER_BYTES:
        return "the first member is not exactly the header"
    try:
        head = _parse_header(io.BytesIO(first))
    except UniError:
        return "unreadable header"
    et, bpe = head["elementType"], head["bytesPerElement"]
    if not ((bpe == 12 and et == 2) or (bpe == 4 and et == 1)):
        return "element type %d with %d bytes per element" % (et, bpe)
    dims = [head["dimZ"], head["dimY"], head["dimX"], 3 if et == 2 else 1]
    if head["dimT"] > 1:
        dims = [head["dimT"]] + dims
    n_bytes = 4 * int(np.prod(dims, dtype=np.int64))
    offsets, sizes, members = [], [], []
    at = member_sizes[0]
    for (body, units), msize in zip(index, member_sizes[1:]):
        if body + sum(units) + len(_FINAL_BLOCK) + 8 != at + msize:
            return "a unit index disagrees with its member's size"
        crc, isize = struct.unpack_from("<II", raw, at + msize - 8)
        members.append((len(sizes), len(sizes) + len(units), crc, isize))
        for n in units:
            offsets.append(body)
            body += n
        sizes += units
        at += msize
    if n_bytes < 4 or len(sizes) != (n_bytes + UNIT - 1) // UNIT:
        return "%d units for %d payload bytes" % (len(sizes), n_bytes)
    return head, dims, offsets, sizes, members


def readUniToDevice(filename, device="cuda:0", info=None):
    """readUni with the volume left on the GPU -> (header dict, float32 CUDA tensor [Z,Y,X,C]).  A file written with
    unit_index=True goes up as it is and ops.inflate_units decodes its units in parallel; the member trailers (CRC-32, ISIZE)
    are checked on the host against the unit CRCs the kernel returns.  Every other file, and every file for which the device
    decode reports anything but success, is read by readUni (which raises UniError for a corrupt one) and uploaded.
    info: a dict that receives "path" ("device" or "host") and "reason"."""
    import torch
    dev = torch.device(device)

    def note(path, reason):
        if isinstance(info, dict):
            info["path"], info["reason"] = path, reason

    nbytes = os.path.getsize(filename)
    pinned = torch.empty((nbytes + 15) // 16 * 16, dtype=torch.uint8, pin_memory=True)   # whole 16-byte lines for the kernel
    with open(filename, "rb") as f:
        got = f.readinto(memoryview(pinned.numpy())[:nbytes])
    raw = memoryview(pinned.numpy())[:got]
    pinned[got:] = 0
    plan = _device_plan(raw)
    reason = plan if isinstance(plan, str) else None
    if reason is None:
        head, dims, offsets, sizes, members = plan
        from . import ops
        with torch.cuda.device(dev):
            packed = pinned.to(dev, non_blocking=True)
            n_bytes = 4 * int(np.prod(dims, dtype=np.int64))
            out, crcs, status = ops.inflate_units(packed, offsets, sizes, n_bytes)
            meta = torch.stack([crcs, status]).cpu().numpy().view(np.uint32)        # waits for the decode
        if meta[1].any():
            reason = "unit %d: decode status %d" % (int(np.flatnonzero(meta[1])[0]), int(meta[1][np.flatnonzero(meta[1])[0]]))
        else:
            lengths = [UNIT] * (len(sizes) - 1) + [n_bytes - UNIT * (len(sizes) - 1)]
            for a, b, crc, isize in members:
                if crc32_combine(meta[0][a:b], lengths[a:b]) != crc or (sum(lengths[a:b]) & 0xffffffff) != isize:
                    reason = "member of units %d..%d: CRC-32 or ISIZE mismatch" % (a, b - 1)
                    break
        if reason is None:
            note("device", "")
            return head, out.view(torch.float32).reshape(dims)
    note("host", reason)
    try:
        head, content = readUni(filename)
    except zlib.error as e:
        raise UniError("corrupt deflate data in %s: %s" % (filename, e))
    host = torch.empty(content.shape, dtype=torch.int32 if content.dtype == np.int32 else torch.float32, pin_memory=True)
    np.copyto(host.numpy(), content)
    return head, host.to(dev)


def make_header(dim_x, dim_y, dim_z, vec3=False, info=b"", timestamp=0, grid_type=1):
    """a fresh v4 header (the reference always copies one from an existing file, multipassGAN-out.py:629)"""
    return {
        "dimX": int(dim_x), "dimY": int(dim_y), "dimZ": int(dim_z), "gridType": int(grid_type),
        "elementType": 2 if vec3 else 1, "bytesPerElement": 12 if vec3 else 4,
        "info": bytes(info).ljust(252, b"\0")[:252], "dimT": 0, "timestamp": int(timestamp),
    }


def backupFile(name, test_path):
    """copy a source file into the run directory (uniio.py:126-130)"""
    shutil.copy(name if os.path.dirname(name) else "./" + name, test_path + os.path.basename(name))


# numpy array helpers (uniio.py:168-206)
def writeNumpySingle(filename, content):
    np.savez_compressed(filename, content)


def readNumpy(filename):
    return np.load(filename)
