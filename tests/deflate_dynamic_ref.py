"""Plain Python restatement of the device .uni encoder for ONE unit (csrc/mpgan_deflate.hip), in both modes: the
fixed-code unit of codec "device" and the unit of codec "device_dynamic", whose literal/length symbols get a Huffman
code of their own.  encode_unit returns the unit's bytes, the kernel is held to them byte for byte.

The unit (at most UNIT bytes, a whole number of 32-bit words) becomes a byte-aligned, non-final raw DEFLATE stream:
  tokens   word i equal to word i-1 extends a run; a run is cut into matches of distance 4 and length 4 * min(r, 64),
           every other word is four literal bytes, lowest byte first;
  fixed    one BTYPE 01 block + the empty stored block (00 00 FF FF behind the padding);
  stored   one BTYPE 00 block;
  dynamic  one BTYPE 10 block + the empty stored block.  Code lengths: symbols in use ranked by (count, symbol);
           two-queue Huffman tree (of two equal weights the leaf goes before the internal node); leaves counted per depth
           with everything deeper than 15 on 15; while that over-subscribes the code one leaf leaves level 15 and a leaf
           of the deepest shorter level moves one level down with it; the counts are handed out in rank order, the
           longest to the rarest symbol; canonical codes (RFC 1951 3.2.2).  Header: HLIT = highest symbol in use + 1,
           four distance codes with lengths 1 0 0 1 (distance symbol 3 is the bit 1), all nineteen lengths of one
           constant code-length code (4 bits for 0, 4..12, 16, 17, 18; 5 bits for 1, 2, 3, 13, 14, 15), the HLIT + 4
           lengths as one sequence, run-length coded greedily.
  choice   stored where the fixed form is longer than it, dynamic where strictly shorter than both.
"""
import numpy as np

UNIT = 32768
MAXBITS = 15
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_LEN = [4, 5, 5, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 4, 4, 4]


def _reverse(code, n):
    return int(format(code, "0%db" % n)[::-1], 2)


def canonical(lengths):
    """symbol -> (bit-reversed code, length) for the lengths > 0, RFC 1951 3.2.2"""
    count = [0] * (max(lengths) + 2)
    for n in lengths:
        if n:
            count[n] += 1
    nxt, code = {}, 0
    for bits in range(1, len(count)):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (_reverse(nxt[n], n), n)
            nxt[n] += 1
    return out


CL_CODE = canonical(CL_LEN)


def tokenise(words):
    """-> (is_literal[nw], closes[nw], q[nw]): word k is four literals, or the last word of a match of q[k] words"""
    w = np.asarray(words, np.uint32)
    nw = len(w)
    eq = np.zeros(nw, bool)
    eq[1:] = w[1:] == w[:-1]
    idx = np.arange(nw)
    lit = np.maximum.accumulate(np.where(~eq, idx, -1))
    p = (idx - lit - 1) & 63
    nxt = np.zeros(nw, bool)
    nxt[:-1] = eq[1:]
    closes = eq & ((p == 63) | ~nxt)
    return ~eq, closes, p + 1


def length_symbol(q):
    """match of q words -> (length symbol, extra bits, their value)"""
    n = 4 * q
    if n <= 10:
        return 254 + n, 0, 0
    x = n - 3
    e = x.bit_length() - 1 - 2
    return 261 + 4 * e + ((x >> e) & 3), e, x & ((1 << e) - 1)


def histogram(words):
    """counts of the symbols 0..285: literal bytes, one length symbol per match, one end of block"""
    w = np.asarray(words, np.uint32)
    is_lit, closes, q = tokenise(w)
    freq = np.bincount(w[is_lit].view(np.uint8), minlength=286).astype(np.int64)
    for qq, c in zip(*np.unique(q[closes], return_counts=True)):
        freq[length_symbol(int(qq))[0]] += int(c)
    freq[256] += 1
    return freq


def code_lengths(freq):
    """lengths of at most 15 bits for the symbols with freq > 0 (at least two of them)"""
    used = sorted((int(f), s) for s, f in enumerate(freq) if f > 0)
    n = len(used)
    assert n >= 2
    w = [f for f, _ in used] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    li, ni, nn = 0, n, n
    for _ in range(n - 1):
        total = 0
        for _ in range(2):
            if li < n and (ni >= nn or w[li] <= w[ni]):
                a, li = li, li + 1
            else:
                a, ni = ni, ni + 1
            total += w[a]
            parent[a] = nn
        w[nn] = total
        nn += 1
    count = [0] * (MAXBITS + 1)
    for r in range(n):
        node, d = r, 0
        while node != 2 * n - 2:
            node, d = parent[node], d + 1
        count[min(d, MAXBITS)] += 1
    total = sum(count[i] << (MAXBITS - i) for i in range(1, MAXBITS + 1))
    while total > 1 << MAXBITS:
        count[MAXBITS] -= 1
        for i in range(MAXBITS - 1, 0, -1):
            if count[i]:
                count[i] -= 1
                count[i + 1] += 2
                break
        total -= 1
    lengths = [0] * len(freq)
    r = 0
    for bits in range(MAXBITS, 0, -1):
        for _ in range(count[bits]):
            lengths[used[r][1]] = bits
            r += 1
    assert r == n
    return lengths


def header_tokens(lengths):
    """the dynamic block header as (value, bits) pairs, first bit lowest"""
    hlit = max(257, max(s for s, n in enumerate(lengths) if n) + 1)
    out = [(4, 3), (hlit - 257, 5), (3, 5), (15, 4)]           # BFINAL 0 BTYPE 10, HLIT, HDIST, HCLEN
    out += [(CL_LEN[s], 3) for s in CL_ORDER]
    seq = list(lengths[:hlit]) + [1, 0, 0, 1]
    i = 0
    while i < len(seq):
        v, j = seq[i], i + 1
        while j < len(seq) and seq[j] == v:
            j += 1
        r = j - i
        if v == 0:
            while r >= 11:
                c = min(r, 138)
                out += [CL_CODE[18], (c - 11, 7)]
                r -= c
            if r >= 3:
                out += [CL_CODE[17], (r - 3, 3)]
                r = 0
        else:
            out.append(CL_CODE[v])
            r -= 1
            while r >= 3:
                c = min(r, 6)
                out += [CL_CODE[16], (c - 3, 2)]
                r -= c
        out += [CL_CODE[v]] * r
        i = j
    return out


def _fixed_table():
    lengths = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    return canonical(lengths)


FIXED = _fixed_table()


def _token_arrays(words, table, dist_value, dist_bits):
    """(values, bits) of the unit's tokens in stream order under `table` (symbol -> (reversed code, length))"""
    w = np.asarray(words, np.uint32)
    nw = len(w)
    is_lit, closes, q = tokenise(w)
    code = np.zeros(286, np.uint64)
    size = np.zeros(286, np.int64)
    for s, (c, n) in table.items():
        if s < 286:
            code[s], size[s] = c, n
    vals = np.zeros((nw, 4), np.uint64)
    bits = np.zeros((nw, 4), np.int64)
    b = w[is_lit].view(np.uint8).reshape(-1, 4)
    vals[is_lit] = code[b]
    bits[is_lit] = size[b]
    for k in np.flatnonzero(closes):
        s, e, x = length_symbol(int(q[k]))
        n = int(size[s])
        assert n > 0
        vals[k, 0] = int(code[s]) | (x << n) | (dist_value << (n + e))
        bits[k, 0] = n + e + dist_bits
    keep = bits.reshape(-1) > 0
    return vals.reshape(-1)[keep], bits.reshape(-1)[keep]


def _pack(vals, bits):
    """LSB-first bit string of the (value, bits) tokens -> (bytes zero-padded to a byte, bit count)"""
    vals = np.asarray(vals, np.uint64)
    bits = np.asarray(bits, np.int64)
    total = int(bits.sum())
    start = np.cumsum(bits) - bits
    pos = np.arange(total) - np.repeat(start, bits)
    stream = ((np.repeat(vals, bits) >> pos.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(stream, bitorder="little").tobytes(), total


def _close(vals, bits):
    """block bits + the empty stored block: header 000, padding, 00 00 FF FF"""
    body, total = _pack(vals, bits)
    n = (total + 3 + 7) >> 3
    return body.ljust(n, b"\0") + b"\x00\x00\xff\xff"


def fixed_size(words):
    w = np.asarray(words, np.uint32)
    is_lit, closes, q = tokenise(w)
    b = w[is_lit].view(np.uint8)
    total = 3 + 8 * len(b) + int((b >= 144).sum())
    for qq, c in zip(*np.unique(q[closes], return_counts=True)):
        s, e, _ = length_symbol(int(qq))
        total += int(c) * (FIXED[s][1] + e + 5)
    return ((total + 7 + 3 + 7) >> 3) + 4


def stored_size(words):
    return 5 + 4 * len(words)


def dynamic_size(words, freq=None, lengths=None):
    freq = histogram(words) if freq is None else freq
    lengths = code_lengths(freq) if lengths is None else lengths
    total = sum(n for _, n in header_tokens(lengths)) + sum(int(f) * n for f, n in zip(freq, lengths))
    for s in range(257, 286):
        if freq[s]:
            total += int(freq[s]) * (max(0, (s - 261) // 4) + 1)       # extra bits of the symbol, one distance bit
    return ((total + 3 + 7) >> 3) + 4


def unit_size(words, dynamic=True):
    """size of the unit's stream without building it"""
    fixed, stored = fixed_size(words), stored_size(words)
    size = stored if fixed > stored else fixed
    return min(size, dynamic_size(words)) if dynamic else size


def encode_fixed(words):
    vals, bits = _token_arrays(words, FIXED, 3 << 3, 5)         # distance code 00011, first bit lowest: 11000
    vals = np.concatenate([[2], vals, [0]]).astype(np.uint64)   # BFINAL 0 BTYPE 01 ... end of block 0000000
    bits = np.concatenate([[3], bits, [7]])
    return _close(vals, bits)


def encode_stored(words):
    raw = np.asarray(words, np.uint32).tobytes()
    n = len(raw)
    return bytes([0, n & 255, n >> 8, (~n) & 255, ((~n) >> 8) & 255]) + raw


def encode_dynamic(words):
    lengths = code_lengths(histogram(words))
    table = canonical(lengths)
    head = header_tokens(lengths)
    vals, bits = _token_arrays(words, table, 1, 1)
    vals = np.concatenate([[v for v, _ in head], vals, [table[256][0]]]).astype(np.uint64)
    bits = np.concatenate([[n for _, n in head], bits, [table[256][1]]]).astype(np.int64)
    return _close(vals, bits)


def encode_unit(words, dynamic=True):
    """the bytes of one unit; dynamic=False: what codec "device" writes"""
    words = np.asarray(words, np.uint32)
    assert 1 <= len(words) <= UNIT // 4
    fixed, stored = fixed_size(words), stored_size(words)
    size = stored if fixed > stored else fixed
    if dynamic and dynamic_size(words) < size:
        out = encode_dynamic(words)
    elif fixed > stored:
        out = encode_stored(words)
    else:
        out = encode_fixed(words)
    assert len(out) == unit_size(words, dynamic)
    return out


def encode_payload(words, dynamic=True):
    """list of the unit streams of a payload of 32-bit words"""
    words = np.asarray(words, np.uint32)
    return [encode_unit(words[a:a + UNIT // 4], dynamic) for a in range(0, len(words), UNIT // 4)]


# ---------------------------------------------------------------- the test payloads, shared by the host and the GPU tests
def fibonacci_unit():
    """a short unit (6764 bytes) in which the end of block (1) and 17 literal byte values (1, 2, 3, 5, ... 1597, 2585:
    Fibonacci numbers, the last one raised by one to fill the last word) leave Huffman no choice: every merge joins the
    single internal node with the next leaf, whatever the order among equal weights, so the tree is 17 levels deep.
    Consecutive words differ, so every word is literals."""
    fib = [1, 2]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    fib[-1] += 1
    data = np.repeat(np.arange(17, dtype=np.uint8) * 13 + 7, fib)
    assert len(data) == 6764
    rng = np.random.default_rng(18)
    while True:
        words = rng.permutation(data).view(np.uint32)
        if not (words[1:] == words[:-1]).any():
            return words.copy()


def smooth_unit(n=UNIT // 4):
    x = np.arange(n, dtype=np.float32)
    v = (0.4 + 0.3 * np.sin(x / 97.0) + 0.05 * np.cos(x / 7.0)).astype(np.float32)
    v[(x % 1024) < 300] = 0.0                       # cut-off regions as in a density
    return v.view(np.uint32).copy()


def cases():
    """name -> payload as uint32 words (one unit, or several where the name says so)"""
    W = UNIT // 4
    rng = np.random.default_rng(2024)
    out = {}
    out["zero"] = np.zeros(W, np.uint32)
    out["constant"] = np.full(W, np.float32(0.37).view(np.uint32), np.uint32)
    out["random_bits"] = rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)
    out["smooth"] = smooth_unit()
    out["fibonacci"] = fibonacci_unit()
    runs = rng.uniform(0.1, 1.0, 1024).astype(np.float32)
    at = 3
    for r in (63, 64, 65, 1, 2, 128, 129):          # a literal word and r repeats of it, both sides of the 64-word match
        runs[at:at + r + 1] = runs[at]
        at += r + 7
    out["runs_63_64_65"] = runs.view(np.uint32).copy()
    span = rng.uniform(0.1, 1.0, 2 * W + 40).astype(np.float32)
    span[W - 100:W + 100] = 0.0                     # a run across the first unit boundary
    span[2 * W - 1:2 * W + 1] = 0.25                # and the shortest one across the second
    out["boundary_run_3units"] = span.view(np.uint32).copy()
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x00000001,
                        0x807fffff, 0x00800000, 0x00000000, 0x80000000, 0x80000000, 0xffffffff, 0xffffffff, 0x007fffff],
                       np.uint32)
    out["special_bits"] = np.resize(special, 5000)
    return out


def probe_volume(n=128):
    """the volume of tools/probe_uni.py at n^3: synthetic_volume(64) zoomed linearly, 5e-4 cutoff"""
    import scipy.ndimage
    from mpgan_amd.synthetic import synthetic_volume
    low = synthetic_volume(64, 1, 0)[..., 0]
    vol = np.maximum(scipy.ndimage.zoom(low, n / 64.0, order=1), 0).astype(np.float32)
    vol[vol < 5e-4] = 0
    return vol
