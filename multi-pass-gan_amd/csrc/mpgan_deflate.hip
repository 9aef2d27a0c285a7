// Device-side DEFLATE for .uni volumes (uniio.writeUniFromDevice, codec "device"): the payload is cut into units of
// MPG_DEFLATE_UNIT bytes and every unit becomes a byte-aligned, non-final raw DEFLATE stream (RFC 1951) in its own slot,
// so that only compressed bytes cross to the host.  Fluid densities after the cutoff are mostly runs of one 32-bit
// word, so the tokens are word-granular and need no match search:
//   word i equal to word i-1 extends a run; a run is cut into matches of distance 4 and length 4 * min(r, 64);
//   every other word is four literal bytes; fixed Huffman code (BTYPE 01); a unit whose fixed form would be longer
//   than its stored form is written as one stored block (BTYPE 00).
// A fixed-Huffman unit ends with an empty stored block (00 00 FF FF after the padding, zlib's sync-flush marker), which
// byte-aligns it: units concatenate into one member body, and the host closes a member with an empty final block.
// The same kernel computes the CRC-32 of each unit's input; the host combines unit CRCs into member CRCs.
//
// Dynamic mode (codec "device_dynamic", mpg_deflate_encode_dynamic): same units, tokens and framing, but the
// literal/length symbols of a unit get a Huffman code of their own (BTYPE 10).  Per unit: histogram of the symbols
// 0..285 in LDS (one copy per wave) -> ranks by (count, symbol) -> two-queue Huffman tree on one thread -> leaf depths,
// counted per length with everything deeper than 15 on 15 -> while that over-subscribes the code, one leaf leaves the
// last level and a leaf of the deepest shorter level moves down with it -> lengths handed out in rank order, canonical
// codes.  The header sends all nineteen lengths of ONE code-length code that never changes (4 bits for 0, 4..12, 16, 17,
// 18; 5 bits for the rest), the lengths run-length coded greedily with 16 / 17 / 18, and a distance code of two 1-bit
// codes (symbols 0 and 3) of which only 3 is used: complete, one bit per match.  The exact sizes of the dynamic, fixed
// and stored forms are known before anything is emitted; the shortest is written (dynamic only where strictly
// shorter).  tests/deflate_dynamic_ref.py restates all of this in Python, and the kernel is held to it byte for byte.
#include <cstdint>

#include "mpgan_crc.h"
#include "mpgan_internal.h"

namespace {

typedef uint32_t u4v __attribute__((ext_vector_type(4)));

constexpr int UNIT = MPG_DEFLATE_UNIT;         // payload bytes per unit
constexpr int UW = UNIT / 4;                   // words per unit
constexpr int SLOT = MPG_DEFLATE_SLOT;         // workspace bytes per unit (>= stored form, multiple of 16)
constexpr int NT = 512;                        // threads per block: 8 waves
constexpr int WPT = UW / NT;                   // contiguous words per thread
constexpr int NWAVE = NT / 64;
static_assert(UNIT % 16 == 0 && UNIT <= 65535, "16-byte loads; one stored block per unit");
static_assert(SLOT % 16 == 0 && SLOT >= UNIT + 5, "slot holds the stored form");
static_assert(WPT == 16, "pad() and the 17-bit run masks are written for 16 words per thread");

// LDS word index of unit word i: one pad word per thread piece, so that the 64 lanes of a wave, each walking its own
// piece (stride WPT words), touch 64 different banks (stride 17)
__device__ __forceinline__ int pad(int i) { return i + (i >> 4); }
constexpr int IN_WORDS = UW + UW / WPT + 1;
constexpr int OUT_WORDS = SLOT / 4;
constexpr size_t LDS_BYTES = (size_t)(OUT_WORDS + IN_WORDS + 4 * 256 + 2 * NWAVE + 4) * sizeof(uint32_t);

// Dynamic mode: the per-unit code table and block header live behind the fixed layout; everything else the code
// construction needs borrows the output image, which is not written before the emit pass and is zeroed again before it.
constexpr int NSYM = 286;                      // literal/length alphabet
constexpr int NSYM_PAD = 288;
constexpr int MAXBITS = 15;
constexpr int HDR_WORDS = 64;                  // 74 fixed bits + at most 290 code lengths of 5 bits = 1524 bits
constexpr size_t LDS_BYTES_DYN = LDS_BYTES + (size_t)(NSYM_PAD + HDR_WORDS + 4) * sizeof(uint32_t);
static_assert(LDS_BYTES_DYN <= 80 * 1024, "two blocks per CU");
constexpr int X_HIST = 0;                               // one histogram per wave
constexpr int X_FREQ = X_HIST + NWAVE * NSYM_PAD;       // their sum
constexpr int X_W = X_FREQ + NSYM_PAD;                  // node weights: leaves in rank order, then internal nodes
constexpr int X_SYM = X_W + 2 * NSYM_PAD;               // symbol of the leaf of rank r
constexpr int X_PAR = X_SYM + NSYM_PAD;                 // parent node
constexpr int X_LEN = X_PAR + 2 * NSYM_PAD;             // code length of symbol s
constexpr int X_NC = X_LEN + NSYM_PAD;                  // [1..15] leaves per code length, [16] used symbols, [17] highest one
constexpr int X_END = X_NC + 32;
static_assert(X_END <= OUT_WORDS, "scratch fits the output image");

// The code-length code of the dynamic header is the same in every unit: 4 bits for 0, 4..12 and the run symbols
// 16, 17, 18, 5 bits for 1, 2, 3, 13, 14, 15 (13 / 16 + 6 / 32 = 1, a complete code).  Canonical codes, MSB first.
__device__ __forceinline__ void cl_code(int sym, uint32_t& code, int& n) {
    if (sym == 0) { code = 0; n = 4; }
    else if (sym <= 3) { code = 26 + (sym - 1); n = 5; }
    else if (sym <= 12) { code = 1 + (sym - 4); n = 4; }
    else if (sym <= 15) { code = 29 + (sym - 13); n = 5; }
    else { code = 10 + (sym - 16); n = 4; }
    code = __brev(code) >> (32 - n);
}

// serial bit writer of one thread into plain LDS words (the block header)
struct HeaderWriter {
    uint32_t* out;
    unsigned long long acc;
    int fill, wi;
    __device__ __forceinline__ void put(uint32_t bits, int n) {
        acc |= (unsigned long long)bits << fill;
        fill += n;
        if (fill >= 32) {
            out[wi++] = (uint32_t)acc;
            acc >>= 32;
            fill -= 32;
        }
    }
    __device__ __forceinline__ void sym(int s) {
        uint32_t c; int n;
        cl_code(s, c, n);
        put(c, n);
    }
};

using mpg_crc::gf_mul;
using mpg_crc::POLY;                           // gzip CRC-32, bit-reflected

struct Tables {
    uint32_t crc[4][256];      // slice-by-4: crc[k][b] = register after byte b and k zero bytes
    uint32_t xp[NT];           // x^(8 * 4 * WPT * j) mod P: moves a piece CRC past j later pieces
};

constexpr Tables make_tables() {
    Tables t{};
    mpg_crc::fill_slice_tables(t.crc);
    uint32_t step = 0x40000000u;                                    // x^1
    for (int bits = 1; bits < 32 * WPT; bits *= 2) step = gf_mul(step, step);
    t.xp[0] = 0x80000000u;                                          // x^0
    for (int j = 1; j < NT; ++j) t.xp[j] = gf_mul(t.xp[j - 1], step);
    return t;
}
static_assert((32 * WPT & (32 * WPT - 1)) == 0, "x^(bits per piece) by squaring");

__device__ const Tables d_tables = make_tables();

// ---------------------------------------------------------------- block scans (8 waves of 64)
__device__ __forceinline__ uint32_t block_excl_sum(uint32_t v, uint32_t* scr, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) scr[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < NWAVE; ++k) {
        const uint32_t s = scr[k];
        if (k < wave) before += s;
        all += s;
    }
    __syncthreads();
    total = all;
    return x - v + before;
}

// max over the threads before this one (-1 if none)
__device__ __forceinline__ int block_excl_max(int v, int* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x = max(x, y);
    }
    if (lane == 63) scr[wave] = x;
    __syncthreads();
    int before = -1;
#pragma unroll
    for (int k = 0; k < NWAVE; ++k)
        if (k < wave) before = max(before, scr[k]);
    __syncthreads();
    const int up = __shfl_up(x, 1);
    return lane > 0 ? max(before, up) : before;
}

// ---------------------------------------------------------------- fixed Huffman codes, bit-reversed for LSB-first packing
__device__ __forceinline__ int literal_bits(uint32_t w) {
    return 32 + ((w & 0xffu) >= 144u) + (((w >> 8) & 0xffu) >= 144u) + (((w >> 16) & 0xffu) >= 144u) + ((w >> 24) >= 144u);
}

// length symbol (257..284) of a match of q words (1..64), its e extra bits and their value
__device__ __forceinline__ void match_symbol(int q, int& sym, int& e, uint32_t& extra) {
    const int len = 4 * q;
    e = 0;
    extra = 0;
    if (len <= 10)
        sym = 254 + len;
    else {
        const int l = len - 3;
        e = (31 - __clz(l)) - 2;
        sym = 261 + 4 * e + ((l >> e) & 3);
        extra = (uint32_t)l & ((1u << e) - 1u);
    }
}

// match of q words (1..64) at distance 4: length code + extra bits + distance code 3 (5 bits, no extra)
__device__ __forceinline__ void match_code(int q, uint32_t& bits, int& n) {
    int sym, e;
    uint32_t extra;
    match_symbol(q, sym, e, extra);
    uint32_t code;
    int nl;
    if (sym < 280) { code = __brev((uint32_t)(sym - 256)) >> 25; nl = 7; }
    else           { code = __brev((uint32_t)(0xC0 + sym - 280)) >> 24; nl = 8; }
    bits = code | (extra << nl) | (24u << (nl + e));      // distance code 00011, first bit lowest
    n = nl + e + 5;
}

// Bit writer of one thread: its bits are a contiguous range of the unit's stream.  Only the first and the last output
// word of the range can hold other threads' bits, and those two go through LDS atomic OR on the zeroed buffer.
struct BitWriter {
    uint32_t* out;
    unsigned long long acc;
    int fill, wi;
    bool first;
    __device__ __forceinline__ void put(uint32_t bits, int n) {
        acc |= (unsigned long long)bits << fill;
        fill += n;
        if (fill >= 32) {
            if (first) atomicOr(&out[wi], (uint32_t)acc);
            else out[wi] = (uint32_t)acc;
            first = false;
            acc >>= 32;
            fill -= 32;
            ++wi;
        }
    }
    __device__ __forceinline__ void finish() {
        if (fill > 0) atomicOr(&out[wi], (uint32_t)acc);
    }
};

// One block per unit (grid-stride).  slots[u * SLOT ..]: the unit's stream, sizes[u] its length, crcs[u] the CRC-32 of
// its input bytes.  DYN: the unit's literal/length symbols get a Huffman code of their own (BTYPE 10) where that is the
// shortest of the three forms; the tokens, the framing and the CRC are those of the fixed mode.
template <bool DYN>
__global__ __launch_bounds__(NT) void deflate_units_kernel(const uint32_t* __restrict__ src, size_t n_words, unsigned n_units,
                                                           unsigned char* __restrict__ slots, uint32_t* __restrict__ sizes,
                                                           uint32_t* __restrict__ crcs) {
    extern __shared__ u4v lds4[];
    uint32_t* s_out = reinterpret_cast<uint32_t*>(lds4);           // 16-byte aligned: read back 16 bytes at a time
    uint32_t* s_in = s_out + OUT_WORDS;
    uint32_t* s_tab = s_in + IN_WORDS;
    uint32_t* s_scr = s_tab + 4 * 256;
    uint32_t* s_code = s_scr + 2 * NWAVE + 4;                      // DYN: bit-reversed code | length << 16 per symbol
    uint32_t* s_hdr = s_code + NSYM_PAD;                           // DYN: the block header, s_hdr[HDR_WORDS] its bit count
    const int t = threadIdx.x;

    for (int k = t; k < 4 * 256; k += NT) s_tab[k] = d_tables.crc[k >> 8][k & 255];

    for (unsigned u = blockIdx.x; u < n_units; u += gridDim.x) {
        const size_t w0 = (size_t)u * UW;
        const int nw = (int)((n_words - w0) < (size_t)UW ? (n_words - w0) : (size_t)UW);
        const uint32_t* in = src + w0;

        // stage: zero the output image, load the unit with 16-byte loads
        for (int q = t; q < SLOT / 16; q += NT) lds4[q] = u4v{0u, 0u, 0u, 0u};
        const int nq = nw >> 2;
        for (int q = t; q < nq; q += NT) {
            const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(in) + q);
            const int p = pad(4 * q);
            s_in[p] = v.x; s_in[p + 1] = v.y; s_in[p + 2] = v.z; s_in[p + 3] = v.w;
        }
        if (t < (nw & 3)) s_in[pad(4 * nq + t)] = in[4 * nq + t];
        __syncthreads();

        // this thread's piece: words [base, base + cnt)
        const int base = t * WPT;
        const int cnt = min(max(nw - base, 0), WPT);
        uint32_t eqmask = 0;          // bit k: word base + k repeats its predecessor; bit cnt: so does the word after
        int last_lit = -1, lit_bits = 0;
        {
            uint32_t prev = base > 0 && cnt > 0 ? s_in[pad(base - 1)] : 0u;
#pragma unroll
            for (int k = 0; k < WPT; ++k) {
                if (k < cnt) {
                    const uint32_t w = s_in[pad(base + k)];
                    if (base + k > 0 && w == prev) eqmask |= 1u << k;
                    else { last_lit = base + k; lit_bits += literal_bits(w); }
                    prev = w;
                }
            }
            if (cnt == WPT && base + WPT < nw && s_in[pad(base + WPT)] == prev) eqmask |= 1u << WPT;
        }

        // CRC-32 of the piece that ENDS 4 * WPT * t bytes before the unit's end: every shift is a whole number of
        // pieces (table xp), the short piece is the first one, which also takes the 0xffffffff start value
        uint32_t crc_part;
        {
            const int hi = nw - WPT * t, lo = max(hi - WPT, 0);
            uint32_t c = (hi > 0 && lo == 0) ? 0xffffffffu : 0u;
            for (int i = lo; i < hi; ++i) {
                c ^= s_in[pad(i)];
                if (c != 0u)
                    c = s_tab[768 + (c & 255u)] ^ s_tab[512 + ((c >> 8) & 255u)] ^ s_tab[256 + ((c >> 16) & 255u)] ^ s_tab[c >> 24];
            }
            uint32_t m = 0, b = d_tables.xp[t];
            if (c != 0u) {
#pragma unroll 4
                for (int i = 0; i < 32; ++i) {
                    if (c & (0x80000000u >> i)) m ^= b;
                    b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
                }
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) m ^= __shfl_xor(m, d);
            crc_part = m;
        }

        // where the run that reaches this piece started: the last literal word before it
        const int lit_before = block_excl_max(last_lit, reinterpret_cast<int*>(s_scr));

        // pass 1: bits of this piece's tokens.  A match is charged to the LAST word it covers: the word that closes a
        // 64-word chunk of its run, or the run itself
        uint32_t my_bits = lit_bits + (t == 0 ? 3 : 0);
        {
            int lit = lit_before;
#pragma unroll
            for (int k = 0; k < WPT; ++k) {
                if (k < cnt) {
                    if (!((eqmask >> k) & 1u)) lit = base + k;
                    else {
                        const int p = (base + k - lit - 1) & 63;
                        if (p == 63 || !((eqmask >> (k + 1)) & 1u)) {
                            uint32_t mb; int mn;
                            match_code(p + 1, mb, mn);
                            my_bits += mn;
                        }
                    }
                }
            }
        }
        if ((t & 63) == 0) s_scr[NWAVE + (t >> 6)] = crc_part;
        uint32_t token_bits;
        const uint32_t off = block_excl_sum(my_bits, s_scr, token_bits);     // its barriers also publish the wave CRCs

        // header (3) + tokens + end of block (7) + empty stored block: header (3), padding, 00 00 FF FF
        const uint32_t body = (token_bits + 7 + 3 + 7) >> 3;
        const uint32_t fixed_size = body + 4;
        const uint32_t stored_size = 5u + 4u * (uint32_t)nw;
        const bool stored = fixed_size > stored_size;
        uint32_t size = stored ? stored_size : fixed_size;

        bool dynamic = false;
        uint32_t dyn_off = 0, dyn_body = 0;
        if constexpr (DYN) {
            // histogram of the literal/length symbols, one copy per wave on the still zero output image.  The top byte
            // of a float (sign and exponent) hardly changes along a piece: it is counted in a register first
            {
                uint32_t* hist = s_out + X_HIST + (t >> 6) * NSYM_PAD;
                int lit = lit_before, top = -1;
                uint32_t top_n = 0;
#pragma unroll
                for (int k = 0; k < WPT; ++k) {
                    if (k < cnt) {
                        if (!((eqmask >> k) & 1u)) {
                            lit = base + k;
                            const uint32_t w = s_in[pad(base + k)];
                            atomicAdd(&hist[w & 255u], 1u);
                            atomicAdd(&hist[(w >> 8) & 255u], 1u);
                            atomicAdd(&hist[(w >> 16) & 255u], 1u);
                            if ((int)(w >> 24) != top) {
                                if (top_n) atomicAdd(&hist[top], top_n);
                                top = (int)(w >> 24);
                                top_n = 0;
                            }
                            ++top_n;
                        } else {
                            const int p = (base + k - lit - 1) & 63;
                            if (p == 63 || !((eqmask >> (k + 1)) & 1u)) {
                                int sym, e; uint32_t extra;
                                match_symbol(p + 1, sym, e, extra);
                                atomicAdd(&hist[sym], 1u);
                            }
                        }
                    }
                }
                if (top_n) atomicAdd(&hist[top], top_n);
                if (t == 0) atomicAdd(&hist[256], 1u);                       // end of block
            }
            __syncthreads();
            uint32_t* x_freq = s_out + X_FREQ;
            uint32_t* x_w = s_out + X_W;
            uint32_t* x_sym = s_out + X_SYM;
            uint32_t* x_par = s_out + X_PAR;
            uint32_t* x_len = s_out + X_LEN;
            uint32_t* x_nc = s_out + X_NC;
            if (t < NSYM) {
                uint32_t f = 0;
#pragma unroll
                for (int k = 0; k < NWAVE; ++k) f += s_out[X_HIST + k * NSYM_PAD + t];
                x_freq[t] = f;
            }
            __syncthreads();
            // rank of every used symbol by (count, symbol): leaf r of the tree is the symbol of rank r
            if (t < NSYM) {
                const uint32_t f = x_freq[t];
                if (f > 0u) {
                    int r = 0;
                    for (int s = 0; s < NSYM; ++s) {
                        const uint32_t g = x_freq[s];
                        r += (g > 0u && (g < f || (g == f && s < t))) ? 1 : 0;
                    }
                    x_w[r] = f;
                    x_sym[r] = (uint32_t)t;
                    atomicAdd(&x_nc[16], 1u);
                    atomicMax(&x_nc[17], (uint32_t)t);
                }
            }
            __syncthreads();
            const int n_used = (int)x_nc[16];                                // >= 2: a literal byte and the end of block
            // Huffman tree by the two-queue method: leaves in rank order, internal nodes in the order they are made
            // (both by rising weight); of two equal weights the leaf goes first
            if (t == 0) {
                int li = 0, ni = n_used, nn = n_used;
                uint32_t lw = x_w[0], iw = 0xffffffffu;
                for (int k = 0; k + 1 < n_used; ++k) {
                    uint32_t sum = 0;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        if (li < n_used && (ni >= nn || lw <= iw)) {
                            sum += lw;
                            x_par[li] = (uint32_t)nn;
                            ++li;
                            lw = li < n_used ? x_w[li] : 0xffffffffu;
                        } else {
                            sum += iw;
                            x_par[ni] = (uint32_t)nn;
                            ++ni;
                            iw = ni < nn ? x_w[ni] : 0xffffffffu;
                        }
                    }
                    x_w[nn] = sum;
                    if (ni == nn) iw = sum;
                    ++nn;
                }
            }
            __syncthreads();
            // depth of every leaf, counted per code length with everything deeper than 15 on 15
            if (t < n_used) {
                const int root = 2 * n_used - 2;
                int node = t, d = 0;
                while (node != root && d < 2 * NSYM) { node = (int)x_par[node]; ++d; }
                atomicAdd(&x_nc[min(d, MAXBITS)], 1u);
            }
            __syncthreads();
            // length limit: while the code is over-subscribed, take one leaf off the last level and move a leaf of the
            // deepest shorter level down with it (one unit of 2^-15 each time)
            if (t == 0) {
                uint32_t total = 0;
                for (int i = 1; i <= MAXBITS; ++i) total += x_nc[i] << (MAXBITS - i);
                while (total > (1u << MAXBITS)) {
                    x_nc[MAXBITS] -= 1u;
                    for (int i = MAXBITS - 1; i >= 1; --i) {
                        if (x_nc[i] > 0u) { x_nc[i] -= 1u; x_nc[i + 1] += 2u; break; }
                    }
                    --total;
                }
            }
            __syncthreads();
            // lengths go out in rank order, the longest to the rarest symbol
            if (t < n_used) {
                int L = MAXBITS;
                uint32_t acc = x_nc[MAXBITS];
                while ((uint32_t)t >= acc && L > 1) { --L; acc += x_nc[L]; }
                x_len[x_sym[t]] = (uint32_t)L;
            }
            __syncthreads();
            // canonical codes (RFC 1951 3.2.2), and on thread 0 the block header
            if (t < NSYM_PAD) {
                uint32_t v = 0;
                const uint32_t L = t < NSYM ? x_len[t] : 0u;
                if (L > 0u) {
                    uint32_t code = 0;
                    for (uint32_t b = 1; b < L; ++b) code = (code + x_nc[b]) << 1;
                    for (int s = 0; s < t; ++s) code += (x_len[s] == L) ? 1u : 0u;
                    v = (__brev(code) >> (32u - L)) | (L << 16);
                }
                s_code[t] = v;
            }
            if (t == 0) {
                const int hlit = max((int)x_nc[17] + 1, 257);
                HeaderWriter hw{s_hdr, 0ull, 0, 0};
                hw.put(4u, 3);                                               // BFINAL 0, BTYPE 10
                hw.put((uint32_t)(hlit - 257), 5);
                hw.put(3u, 5);                                               // HDIST: four distance codes
                hw.put(15u, 4);                                              // HCLEN: all nineteen
                // lengths of the code-length code in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                // (three bits each, the first in the lowest bits)
                hw.put(04444u, 12); hw.put(04444u, 12); hw.put(04444u, 12); hw.put(0554u, 9); hw.put(0555u, 9); hw.put(5u, 3);
                // code lengths of the literal/length alphabet, then of the distance alphabet: 1 0 0 1, so that the code of
                // distance symbol 3 is the single bit 1 and the code is complete
                const int total_len = hlit + 4;
                int i = 0;
                while (i < total_len) {
                    const uint32_t v = i < hlit ? x_len[i] : ((i - hlit == 0 || i - hlit == 3) ? 1u : 0u);
                    int j = i + 1;
                    while (j < total_len && (j < hlit ? x_len[j] : ((j - hlit == 0 || j - hlit == 3) ? 1u : 0u)) == v) ++j;
                    int r = j - i;
                    if (v == 0u) {
                        while (r >= 11) { const int c = min(r, 138); hw.sym(18); hw.put((uint32_t)(c - 11), 7); r -= c; }
                        if (r >= 3) { hw.sym(17); hw.put((uint32_t)(r - 3), 3); r = 0; }
                    } else {
                        hw.sym((int)v);
                        --r;
                        while (r >= 3) { const int c = min(r, 6); hw.sym(16); hw.put((uint32_t)(c - 3), 2); r -= c; }
                    }
                    for (; r > 0; --r) hw.sym((int)v);
                    i = j;
                }
                const int hdr_bits = 32 * hw.wi + hw.fill;
                if (hw.fill > 0) s_hdr[hw.wi] = (uint32_t)hw.acc;
                s_hdr[HDR_WORDS] = (uint32_t)hdr_bits;
            }
            __syncthreads();

            // bits of this piece under the unit's code; thread 0 is charged the header, the last thread the end of block
            uint32_t dyn_bits = t == 0 ? s_hdr[HDR_WORDS] : 0u;
            {
                int lit = lit_before;
#pragma unroll
                for (int k = 0; k < WPT; ++k) {
                    if (k < cnt) {
                        if (!((eqmask >> k) & 1u)) {
                            lit = base + k;
                            const uint32_t w = s_in[pad(base + k)];
                            dyn_bits += (s_code[w & 255u] >> 16) + (s_code[(w >> 8) & 255u] >> 16) + (s_code[(w >> 16) & 255u] >> 16) +
                                        (s_code[w >> 24] >> 16);
                        } else {
                            const int p = (base + k - lit - 1) & 63;
                            if (p == 63 || !((eqmask >> (k + 1)) & 1u)) {
                                int sym, e; uint32_t extra;
                                match_symbol(p + 1, sym, e, extra);
                                dyn_bits += (s_code[sym] >> 16) + (uint32_t)e + 1u;
                            }
                        }
                    }
                }
            }
            if (t == NT - 1) dyn_bits += s_code[256] >> 16;
            uint32_t dyn_total;
            dyn_off = block_excl_sum(dyn_bits, s_scr, dyn_total);
            dyn_body = (dyn_total + 3 + 7) >> 3;                             // empty stored block: header (3), padding
            const uint32_t dyn_size = dyn_body + 4;
            dynamic = dyn_size < size;
            if (dynamic) size = dyn_size;
            // the output image again
            for (int q = t; q < (X_END + 3) / 4; q += NT) lds4[q] = u4v{0u, 0u, 0u, 0u};
            __syncthreads();
        }

        if (DYN && dynamic) {
            for (int k = t; k < (int)((s_hdr[HDR_WORDS] + 31u) >> 5); k += NT) atomicOr(&s_out[k], s_hdr[k]);
            BitWriter bw{s_out, 0ull, (int)(dyn_off & 31u), (int)(dyn_off >> 5), true};
            if (t == 0) { bw.fill = (int)(s_hdr[HDR_WORDS] & 31u); bw.wi = (int)(s_hdr[HDR_WORDS] >> 5); }
            int lit = lit_before;
#pragma unroll
            for (int k = 0; k < WPT; ++k) {
                if (k < cnt) {
                    if (!((eqmask >> k) & 1u)) {
                        lit = base + k;
                        const uint32_t w = s_in[pad(base + k)];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t c = s_code[(w >> (8 * j)) & 255u];
                            bw.put(c & 0xffffu, (int)(c >> 16));
                        }
                    } else {
                        const int p = (base + k - lit - 1) & 63;
                        if (p == 63 || !((eqmask >> (k + 1)) & 1u)) {
                            int sym, e; uint32_t extra;
                            match_symbol(p + 1, sym, e, extra);
                            const uint32_t c = s_code[sym];
                            const int nl = (int)(c >> 16);
                            bw.put((c & 0xffffu) | (extra << nl) | (1u << (nl + e)), nl + e + 1);    // distance code: the bit 1
                        }
                    }
                }
            }
            if (t == NT - 1) { const uint32_t c = s_code[256]; bw.put(c & 0xffffu, (int)(c >> 16)); }
            bw.finish();
            if (t == NT - 1) {                                               // LEN 0000, NLEN FFFF behind the padding
                const uint32_t at = dyn_body + 2;
                atomicOr(&s_out[at >> 2], 0xffu << (8 * (at & 3u)));
                atomicOr(&s_out[(at + 1) >> 2], 0xffu << (8 * ((at + 1) & 3u)));
            }
        } else if (!stored) {
            // pass 2: emit
            BitWriter bw{s_out, 0ull, (int)(off & 31u), (int)(off >> 5), true};
            if (t == 0) bw.put(2u, 3);                                       // BFINAL 0, BTYPE 01
            int lit = lit_before;
#pragma unroll
            for (int k = 0; k < WPT; ++k) {
                if (k < cnt) {
                    if (!((eqmask >> k) & 1u)) {
                        lit = base + k;
                        const uint32_t w = s_in[pad(base + k)];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t b = (w >> (8 * j)) & 255u;
                            if (b < 144u) bw.put(__brev(0x30u + b) >> 24, 8);
                            else bw.put(__brev(0x190u + (b - 144u)) >> 23, 9);
                        }
                    } else {
                        const int p = (base + k - lit - 1) & 63;
                        if (p == 63 || !((eqmask >> (k + 1)) & 1u)) {
                            uint32_t mb; int mn;
                            match_code(p + 1, mb, mn);
                            bw.put(mb, mn);
                        }
                    }
                }
            }
            bw.finish();
            if (t == NT - 1) {                                               // LEN 0000, NLEN FFFF behind the padding
                const uint32_t at = body + 2;
                atomicOr(&s_out[at >> 2], 0xffu << (8 * (at & 3u)));
                atomicOr(&s_out[(at + 1) >> 2], 0xffu << (8 * ((at + 1) & 3u)));
            }
        } else {
            // one stored block: 00 | LEN | NLEN | the bytes, i.e. the input shifted by five bytes
            const uint32_t len = 4u * (uint32_t)nw, nlen = (~len) & 0xffffu;
            for (int k = t; k < nw + 2; k += NT) {
                const uint32_t a = k >= 2 ? s_in[pad(k - 2)] : 0u;
                const uint32_t b = (k >= 1 && k - 1 < nw) ? s_in[pad(k - 1)] : 0u;
                uint32_t v;
                if (k == 0) v = (len << 8) | ((nlen & 0xffu) << 24);
                else if (k == 1) v = (nlen >> 8) | (b << 8);
                else v = (a >> 24) | (b << 8);
                s_out[k] = v;
            }
        }
        __syncthreads();

        u4v* dst = reinterpret_cast<u4v*>(slots + (size_t)u * SLOT);
        const int quads = (int)((size + 15u) >> 4);
        for (int q = t; q < quads; q += NT) dst[q] = lds4[q];
        if (t == 0) {
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < NWAVE; ++k) c ^= s_scr[NWAVE + k];
            sizes[u] = size;
            crcs[u] = c ^ 0xffffffffu;
        }
        __syncthreads();
    }
}

// Compaction: out[sum(sizes[0..u)) ..] = slot u.  One block per unit; each block folds the sizes before its own (at most
// a slab's worth of units), then copies with aligned 4-byte stores, the two source words of each funnel-shifted into place.
constexpr int CT = 256;

__global__ __launch_bounds__(CT) void deflate_compact_kernel(const unsigned char* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                             unsigned n_units, unsigned char* __restrict__ out, size_t out_bytes) {
    __shared__ unsigned long long red[CT];
    const unsigned u = blockIdx.x;
    unsigned long long s = 0;
    for (unsigned k = threadIdx.x; k < u; k += CT) s += sizes[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int d = CT / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    const size_t at = (size_t)red[0];
    const uint32_t size = sizes[u];
    if (size > (uint32_t)SLOT || at + size > out_bytes) return;           // never past either buffer
    const unsigned char* sp = slots + (size_t)u * SLOT;
    unsigned char* dp = out + at;
    const uint32_t head = min((uint32_t)((4u - (uint32_t)((uintptr_t)dp & 3u)) & 3u), size);
    const uint32_t words = (size - head) >> 2;
    const uint32_t tail = size - head - 4u * words;
    if (threadIdx.x < head) dp[threadIdx.x] = sp[threadIdx.x];
    if (threadIdx.x < tail) dp[head + 4u * words + threadIdx.x] = sp[head + 4u * words + threadIdx.x];
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sp);           // slots are 16-byte aligned
    uint32_t* dw = reinterpret_cast<uint32_t*>(dp + head);
    const uint32_t sh = 8u * head;                                        // head < 4
    for (uint32_t j = threadIdx.x; j < words; j += CT) {
        const uint32_t lo = sw[j];
        // the high word is read only when it is needed; it lies inside the slot (size + 4 <= SLOT)
        const uint32_t hi = sh != 0u ? sw[j + 1] : 0u;
        dw[j] = sh != 0u ? (lo >> sh) | (hi << (32u - sh)) : lo;
    }
}

}  // namespace

extern "C" size_t mpg_deflate_ws_bytes(size_t n_bytes) {
    return ((n_bytes + MPG_DEFLATE_UNIT - 1) / MPG_DEFLATE_UNIT) * (size_t)MPG_DEFLATE_SLOT;
}

template <bool DYN>
static int deflate_encode(mpg_stream_t stream, const void* src, size_t n_bytes, void* slots, uint32_t* sizes, uint32_t* crcs) {
    MPG_REQUIRE(src && slots && sizes && crcs, "mpg_deflate_encode: null pointer");
    MPG_REQUIRE(n_bytes >= 4 && n_bytes % 4 == 0, "mpg_deflate_encode: %zu bytes is not a positive multiple of 4", n_bytes);
    MPG_REQUIRE(n_bytes <= (size_t)MPG_DEFLATE_SLAB, "mpg_deflate_encode: %zu bytes exceed one slab (%d)", n_bytes, MPG_DEFLATE_SLAB);
    MPG_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)slots & 15) == 0, "mpg_deflate_encode: src and slots must be 16-byte aligned");
    const unsigned n_units = (unsigned)((n_bytes + UNIT - 1) / UNIT);
    const unsigned grid = n_units < 1024u ? n_units : 1024u;
    const hipError_t e = mpg::launch_dyn_lds<deflate_units_kernel<DYN>>(dim3(grid), dim3(NT), DYN ? LDS_BYTES_DYN : LDS_BYTES,
                                                                        (hipStream_t)stream, reinterpret_cast<const uint32_t*>(src),
                                                                        n_bytes / 4, n_units, reinterpret_cast<unsigned char*>(slots),
                                                                        sizes, crcs);
    if (e != hipSuccess) return mpg::hip_check(e, "mpg_deflate_encode: dynamic LDS");
    MPG_LAUNCH_CHECK("deflate_units_kernel");
}

extern "C" int mpg_deflate_encode(mpg_stream_t stream, const void* src, size_t n_bytes, void* slots, uint32_t* sizes,
                                  uint32_t* crcs) {
    return deflate_encode<false>(stream, src, n_bytes, slots, sizes, crcs);
}

extern "C" int mpg_deflate_encode_dynamic(mpg_stream_t stream, const void* src, size_t n_bytes, void* slots, uint32_t* sizes,
                                          uint32_t* crcs) {
    return deflate_encode<true>(stream, src, n_bytes, slots, sizes, crcs);
}

extern "C" int mpg_deflate_compact(mpg_stream_t stream, const void* slots, const uint32_t* sizes, size_t n_units, void* out,
                                   size_t out_bytes) {
    MPG_REQUIRE(slots && sizes && out, "mpg_deflate_compact: null pointer");
    MPG_REQUIRE(n_units >= 1 && n_units <= (size_t)(MPG_DEFLATE_SLAB / MPG_DEFLATE_UNIT), "mpg_deflate_compact: %zu units", n_units);
    MPG_REQUIRE(((uintptr_t)slots & 15) == 0, "mpg_deflate_compact: slots must be 16-byte aligned");
    hipLaunchKernelGGL(deflate_compact_kernel, dim3((unsigned)n_units), dim3(CT), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(slots), sizes, (unsigned)n_units, reinterpret_cast<unsigned char*>(out),
                       out_bytes);
    MPG_LAUNCH_CHECK("deflate_compact_kernel");
}
