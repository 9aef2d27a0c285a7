// Bounded decode core of the device .uni reader (mpg_inflate_units): bit reader, Huffman table build and token loop for ONE
// unit stream of the device codecs (mpgan_deflate.hip; tests/deflate_dynamic_ref.py states the language).  The same source
// is the body of the HIP kernel (mpgan_inflate.hip) and of a stand-alone CPU program (tools/inflate_core_host.cpp), which
// is where it meets a sanitizer.
//
// A unit stream is a byte-aligned, NON-final raw DEFLATE stream: blocks of BTYPE 00, 01 or 10 until the input is used up.
// Tokens are word-granular: literals come four at a time and every match has distance 4 and a length that is a multiple
// of 4, so the decoder keeps the last 32-bit word in a register and never reads its own output.  Anything else that is
// valid DEFLATE ends with UNSUPPORTED, anything that is not with CORRUPT.
//
// The core is written for a group of `io.lanes()` threads in lockstep (one wave; one thread on the CPU).  Every thread runs
// the whole decode on the same values and writes the same values to the shared tables; only the fast table is filled
// cooperatively, one entry per thread and step.  What is outside the core is behind `IO`:
//   uint32_t word(uint32_t i)      32-bit word i of the input, counted from the stream's start aligned down to 16 bytes;
//                                  the core never asks for a word at or beyond the stream's end rounded up to 16 bytes
//   void put(uint32_t w)           the next output word; the core never puts more than out_bytes / 4 of them
//   int lane(), int lanes(), void sync()
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MPG_INFLATE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MPG_INFLATE_HD inline
#endif

namespace mpg_inflate {

constexpr int OK = 0;            // status values of mpg_inflate_units
constexpr int UNSUPPORTED = 1;   // valid DEFLATE outside the writer's token language
constexpr int CORRUPT = 2;

constexpr int MAXBITS = 15;
constexpr int FAST_BITS = 9;     // codes up to 9 bits decode with one table read
constexpr int NLIT = 288, NDIST = 32, NCL = 19;

// 2 KiB (with a 1 KiB input window and a 2 KiB output piece: 5 KiB a wave), shared by the threads of one decode
struct Tables {
    uint16_t fast[1 << FAST_BITS];   // next FAST_BITS stream bits -> symbol | length << 9, 0: the code is longer
    uint16_t lsym[NLIT];             // literal/length symbols in canonical order
    uint8_t dsym[NDIST];             // distance symbols; the code-length code before them
    uint16_t lcount[16], dcount[16]; // codes per length
    uint16_t offs[16];
    uint8_t lens[NLIT + NDIST];
};

// Canonical code of lens[0..n): count[] per length and sym[] sorted by (length, symbol).  0 = complete, -1 = over-subscribed,
// 1 = incomplete.
template <class Sym>
MPG_INFLATE_HD int build_code(const uint8_t* lens, int n, uint16_t* count, Sym* sym, uint16_t* offs) {
    for (int b = 0; b <= MAXBITS; ++b) count[b] = 0;
    for (int s = 0; s < n; ++s) count[lens[s] & 15] = (uint16_t)(count[lens[s] & 15] + 1);
    int left = 1;
    for (int b = 1; b <= MAXBITS; ++b) {
        left = 2 * left - (int)count[b];
        if (left < 0) return -1;
    }
    offs[1] = 0;
    for (int b = 1; b < MAXBITS; ++b) offs[b + 1] = (uint16_t)(offs[b] + count[b]);
    for (int s = 0; s < n; ++s) {
        const int b = lens[s] & 15;
        if (b) {
            sym[offs[b]] = (Sym)s;
            offs[b] = (uint16_t)(offs[b] + 1);
        }
    }
    return left > 0 ? 1 : 0;
}

// The symbol whose code starts `bits` (first stream bit lowest), looking at no more than maxlen of them; len = its length.
// -1: no code of at most maxlen bits matches.
template <class Sym>
MPG_INFLATE_HD int decode_bits(uint32_t bits, int maxlen, const uint16_t* count, const Sym* sym, int& len) {
    int code = 0, first = 0, index = 0;
    for (int b = 1; b <= maxlen; ++b) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = (int)count[b];
        if (code - c < first) {
            len = b;
            return (int)sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    len = 0;
    return -1;
}

template <class IO>
struct BitReader {
    IO& io;
    unsigned long long acc;
    uint32_t nbits, widx, lead_bits, total_bits, wend;

    // the stream starts `lead` bytes into word (lead / 4) and is `size` bytes long
    MPG_INFLATE_HD BitReader(IO& io_, uint32_t lead, uint32_t size) : io(io_) {
        wend = ((lead + size + 15u) >> 4) << 2;
        widx = lead >> 2;
        lead_bits = 8u * lead;
        total_bits = 8u * size;
        acc = 0;
        nbits = 0;
        const uint32_t skip = 8u * (lead & 3u);
        acc = (unsigned long long)(fetch() >> skip);
        nbits = 32u - skip;
    }
    // the next input word; zeros behind the end of the stream's last 16-byte line
    MPG_INFLATE_HD uint32_t fetch() {
        const uint32_t w = widx < wend ? io.word(widx) : 0u;
        ++widx;
        return w;
    }
    MPG_INFLATE_HD void refill() {           // afterwards at least 33 bits
        if (nbits <= 32u) {
            acc |= (unsigned long long)fetch() << nbits;
            nbits += 32u;
        }
    }
    MPG_INFLATE_HD uint32_t peek(int n) const { return (uint32_t)acc & ((1u << n) - 1u); }
    MPG_INFLATE_HD void drop(int n) {
        acc >>= n;
        nbits -= (uint32_t)n;
    }
    MPG_INFLATE_HD uint32_t take(int n) {    // n <= 16
        refill();
        const uint32_t v = peek(n);
        drop(n);
        return v;
    }
    MPG_INFLATE_HD uint32_t used() const { return 32u * widx - lead_bits - nbits; }
    MPG_INFLATE_HD bool over() const { return used() > total_bits; }
};

// Decode one unit stream: `size` bytes that start `lead` (< 16) bytes into io.word(0), into exactly out_bytes (a multiple
// of 4) of output.  size <= MAX_STREAM.  Every loop is bounded by size or out_bytes.
constexpr uint32_t MAX_STREAM = 1u << 20;

template <class IO>
MPG_INFLATE_HD int inflate_unit(IO& io, Tables& t, uint32_t lead, uint32_t size, uint32_t out_bytes) {
    if (size > MAX_STREAM || lead >= 16u || (out_bytes & 3u)) return CORRUPT;
    BitReader<IO> r(io, lead, size);
    const uint32_t out_words = out_bytes >> 2;
    uint32_t done = 0;               // words put
    uint32_t prev = 0;               // the last of them

    // a block takes at least 3 bits
    for (uint32_t blocks = 0; blocks <= (8u * size) / 3u; ++blocks) {
        if (r.over()) return CORRUPT;
        if (r.used() == r.total_bits) return done == out_words ? OK : CORRUPT;
        const uint32_t head = r.take(3);
        if (head & 1u) return UNSUPPORTED;                                   // BFINAL: the writer leaves that to the member
        const uint32_t btype = head >> 1;
        if (btype == 3u) return CORRUPT;

        if (btype == 0u) {
            r.drop((int)(r.nbits & 7u));                                     // to the byte boundary
            const uint32_t len = r.take(16), nlen = r.take(16);
            if ((len ^ nlen) != 0xffffu) return CORRUPT;
            if (len & 3u) return UNSUPPORTED;
            if ((len >> 2) > out_words - done) return CORRUPT;
            if (r.used() + 8u * len > r.total_bits) return CORRUPT;
            for (uint32_t k = 0; k < (len >> 2); ++k) {
                const uint32_t lo = r.take(16);
                prev = lo | (r.take(16) << 16);
                io.put(prev);
            }
            done += len >> 2;
            continue;
        }

        // ---- code lengths: the fixed code, or the block's own
        int nlen, ndist;
        if (btype == 1u) {
            nlen = NLIT;
            ndist = NDIST;
            for (int s = 0; s < NLIT; ++s) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (int s = 0; s < NDIST; ++s) t.lens[NLIT + s] = 5;
        } else {
            nlen = (int)r.take(5) + 257;
            ndist = (int)r.take(5) + 1;
            const int ncode = (int)r.take(4) + 4;
            if (nlen > 286 || ndist > 30) return CORRUPT;
            for (int k = 0; k < NCL; ++k) {
                // order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (RFC 1951 3.2.7)
                const int s = k < 3 ? 16 + k : k == 3 ? 0 : (k & 1) ? 10 - ((k + 1) >> 1) : 6 + (k >> 1);
                t.lens[s] = (uint8_t)(k < ncode ? r.take(3) : 0u);
            }
            if (build_code(t.lens, NCL, t.dcount, t.dsym, t.offs) != 0) return CORRUPT;
            int at = 0;
            // every step writes at least one length
            while (at < nlen + ndist) {
                if (r.over()) return CORRUPT;
                r.refill();
                int n;
                const int s = decode_bits(r.peek(7), 7, t.dcount, t.dsym, n);
                if (s < 0) return CORRUPT;
                r.drop(n);
                if (s < 16) {
                    t.lens[at++] = (uint8_t)s;
                    continue;
                }
                int v = 0, rep;
                if (s == 16) {
                    if (at == 0) return CORRUPT;
                    v = t.lens[at - 1];
                    rep = 3 + (int)r.take(2);
                } else if (s == 17) {
                    rep = 3 + (int)r.take(3);
                } else {
                    rep = 11 + (int)r.take(7);
                }
                if (at + rep > nlen + ndist) return CORRUPT;
                for (; rep > 0; --rep) t.lens[at++] = (uint8_t)v;
            }
            if (t.lens[256] == 0) return CORRUPT;                            // no end of block
        }
        // the distance lengths follow the nlen literal/length ones; the distance code first, the other one then owns t.offs
        if (build_code(t.lens + nlen, ndist, t.dcount, t.dsym, t.offs) != 0) return CORRUPT;
        if (build_code(t.lens, nlen, t.lcount, t.lsym, t.offs) != 0) return CORRUPT;
        io.sync();
        for (int i = io.lane(); i < (1 << FAST_BITS); i += io.lanes()) {
            int n;
            const int s = decode_bits((uint32_t)i, FAST_BITS, t.lcount, t.lsym, n);
            t.fast[i] = s < 0 ? (uint16_t)0 : (uint16_t)(s | (n << 9));
        }
        io.sync();

        // ---- tokens: every step but the last puts at least one byte
        uint32_t cur = 0, nlit = 0;
        bool ended = false;
        for (uint32_t step = 0; step <= out_bytes; ++step) {
            if (r.over()) return CORRUPT;
            r.refill();
            int sym, n;
            const uint32_t e = t.fast[r.peek(FAST_BITS)];
            if (e) {
                sym = (int)(e & 511u);
                n = (int)(e >> 9);
            } else {
                sym = decode_bits(r.peek(MAXBITS), MAXBITS, t.lcount, t.lsym, n);
                if (sym < 0) return CORRUPT;
            }
            r.drop(n);
            if (sym < 256) {
                if (done >= out_words) return CORRUPT;
                cur |= (uint32_t)sym << (8u * nlit);
                if (++nlit == 4u) {
                    io.put(cur);
                    prev = cur;
                    ++done;
                    cur = 0;
                    nlit = 0;
                }
                continue;
            }
            if (sym == 256) {
                ended = true;
                break;
            }
            if (sym > 285) return CORRUPT;
            // length 3..258: symbols 257..264 are 3..10, then four symbols per extra bit, 285 is 258
            uint32_t len;
            if (sym < 265) len = (uint32_t)sym - 254u;
            else if (sym == 285) len = 258u;
            else {
                const int xb = (sym - 261) >> 2;
                len = 3u + ((4u + (uint32_t)((sym - 261) & 3)) << xb) + r.take(xb);
            }
            r.refill();
            const int ds = decode_bits(r.peek(MAXBITS), MAXBITS, t.dcount, t.dsym, n);
            if (ds < 0 || ds > 29) return CORRUPT;
            r.drop(n);
            if (ds != 3 || (len & 3u) || nlit != 0u) return UNSUPPORTED;     // distance 4, whole words
            if (done == 0u) return CORRUPT;                                  // nothing to copy from
            if ((len >> 2) > out_words - done) return CORRUPT;
            for (uint32_t k = 0; k < (len >> 2); ++k) io.put(prev);
            done += len >> 2;
        }
        if (!ended) return CORRUPT;
        if (nlit != 0u) return UNSUPPORTED;
    }
    return CORRUPT;
}

}  // namespace mpg_inflate
