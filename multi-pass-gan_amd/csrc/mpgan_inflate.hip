// Device-side inflate for .uni volumes (uniio.readUniToDevice): the inverse of mpgan_deflate.hip.  A file written with the
// unit index records the length of every unit stream, so the units (MPG_DEFLATE_UNIT payload bytes each, independent,
// byte-aligned, non-final raw DEFLATE streams) decode in parallel: one wave per unit, grid-stride.
//
// Huffman decoding is a dependent chain (table read -> shift -> table read), so the wave runs the decode core
// (mpgan_inflate_core.h) in lockstep, every lane on the same values, and works as a wave only at the edges:
//   input   a 1 KiB window of the stream in LDS, loaded with one 16-byte load per lane from the stream's own 16-byte lines
//           of `packed` (aligned down from its arbitrary start; never a line the stream does not touch);
//   tables  2 KiB in LDS; the 512-entry fast table is filled 64 entries at a time;
//   output  a 2 KiB piece in LDS; when it is full the wave stores it with 16-byte stores and every lane takes the CRC-32 of
//           eight of its words, moved to the piece's end by a GF(2) product and folded over the wave.
// 5 KiB of LDS per wave: the 32 waves a CU can hold fit its 160 KiB.
#include <cstdint>
#include <vector>

#include "mpgan_crc.h"
#include "mpgan_inflate_core.h"
#include "mpgan_internal.h"

namespace {

typedef uint32_t u4v __attribute__((ext_vector_type(4)));

constexpr uint32_t UNIT = MPG_DEFLATE_UNIT;
constexpr uint32_t IN_WORDS = 256;             // input window: one 16-byte line per lane
constexpr uint32_t PIECE = 512;                // output piece in words
constexpr uint32_t LANE_WORDS = PIECE / 64;    // words of a piece whose CRC one lane takes
static_assert(UNIT % (4 * PIECE) == 0, "whole pieces start 16-byte aligned in the output");

struct CrcTables {
    uint32_t crc[4][256];
    uint32_t xp[PIECE + 1];                    // x^(32 j) mod P: moves a CRC register past j later words
};

constexpr CrcTables make_tables() {
    CrcTables t{};
    mpg_crc::fill_slice_tables(t.crc);
    uint32_t step = 0x40000000u;                                    // x^1
    for (int bits = 1; bits < 32; bits *= 2) step = mpg_crc::gf_mul(step, step);
    t.xp[0] = 0x80000000u;                                          // x^0
    for (uint32_t j = 1; j <= PIECE; ++j) t.xp[j] = mpg_crc::gf_mul(t.xp[j - 1], step);
    return t;
}

__device__ const CrcTables d_tables = make_tables();

struct Lds {
    u4v in[IN_WORDS / 4];
    u4v piece[PIECE / 4];
    mpg_inflate::Tables tab;
};
static_assert(sizeof(Lds) <= 5 * 1024, "32 waves per CU");

// What the decode core sees of one wave.  Every member has the same value in all lanes but `ln`.
struct WaveIO {
    Lds& s;
    const u4v* lines;          // the stream's first 16-byte line
    uint32_t n_lines;          // lines it touches
    unsigned char* dst;        // the unit's output, 16-byte aligned
    uint32_t win;              // first input word in the window
    uint32_t fill, stored;     // words in the piece / already in dst
    uint32_t reg;              // CRC register over the stored words
    int ln;

    __device__ __forceinline__ uint32_t word(uint32_t i) {
        if (i - win >= IN_WORDS) {                                           // the core asks for i < 4 * n_lines only
            __syncthreads();
            win = i & ~3u;
            const uint32_t q = (win >> 2) + (uint32_t)ln;
            if (q < n_lines) s.in[ln] = __builtin_nontemporal_load(lines + q);
            __syncthreads();
        }
        return reinterpret_cast<const uint32_t*>(s.in)[i - win];
    }
    __device__ __forceinline__ void put(uint32_t w) {
        reinterpret_cast<uint32_t*>(s.piece)[fill] = w;
        if (++fill == PIECE) flush();
    }
    // store the piece (the core keeps stored + fill within the unit's output) and take its CRC
    __device__ __forceinline__ void flush() {
        __syncthreads();
        const uint32_t n = fill;
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(s.piece);
        u4v* d16 = reinterpret_cast<u4v*>(dst + 4 * (size_t)stored);
        for (uint32_t q = (uint32_t)ln; q < (n >> 2); q += 64u) d16[q] = s.piece[q];
        if ((uint32_t)ln < (n & 3u)) reinterpret_cast<uint32_t*>(d16)[(n & ~3u) + (uint32_t)ln] = pw[(n & ~3u) + (uint32_t)ln];
        const uint32_t lo = min(n, LANE_WORDS * (uint32_t)ln), hi = min(n, lo + LANE_WORDS);
        uint32_t c = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            c ^= pw[i];
            c = d_tables.crc[3][c & 255u] ^ d_tables.crc[2][(c >> 8) & 255u] ^ d_tables.crc[1][(c >> 16) & 255u] ^ d_tables.crc[0][c >> 24];
        }
        uint32_t m = c != 0u ? mpg_crc::gf_mul(c, d_tables.xp[n - hi]) : 0u;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) m ^= __shfl_xor(m, d);
        reg = mpg_crc::gf_mul(reg, d_tables.xp[n]) ^ m;
        stored += n;
        fill = 0;
        __syncthreads();
    }
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// One wave (= one block) per unit, grid-stride.
__global__ __launch_bounds__(64) void inflate_units_kernel(const unsigned char* __restrict__ packed, const unsigned long long* __restrict__ offsets,
                                                           const uint32_t* __restrict__ sizes, unsigned n_units,
                                                           unsigned char* __restrict__ out, size_t n_bytes, uint32_t* __restrict__ crcs,
                                                           uint32_t* __restrict__ status) {
    __shared__ Lds s;
    for (unsigned u = blockIdx.x; u < n_units; u += gridDim.x) {
        const size_t off = (size_t)offsets[u];
        const uint32_t size = sizes[u];
        const size_t at = (size_t)u * UNIT;
        const uint32_t out_bytes = (uint32_t)((n_bytes - at) < (size_t)UNIT ? (n_bytes - at) : (size_t)UNIT);
        const uint32_t lead = (uint32_t)(off & 15u);
        WaveIO io{s, reinterpret_cast<const u4v*>(packed + (off - lead)), (lead + size + 15u) >> 4, out + at, 0x80000000u, 0u, 0u,
                  0xffffffffu, (int)threadIdx.x};
        const int st = mpg_inflate::inflate_unit(io, s.tab, lead, size, out_bytes);
        if (io.fill != 0u) io.flush();
        if (threadIdx.x == 0) {
            crcs[u] = io.reg ^ 0xffffffffu;
            status[u] = (uint32_t)st;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int mpg_inflate_units(mpg_stream_t stream, const void* packed, size_t packed_bytes, const uint64_t* offsets,
                                 const uint32_t* sizes, size_t n_units, void* out, size_t n_bytes, uint32_t* crcs, uint32_t* status) {
    MPG_REQUIRE(packed && offsets && sizes && out && crcs && status, "mpg_inflate_units: null pointer");
    MPG_REQUIRE(((uintptr_t)packed & 15) == 0 && packed_bytes % 16 == 0,
                "mpg_inflate_units: packed must be 16-byte aligned and a whole number of 16-byte lines (%zu bytes)", packed_bytes);
    MPG_REQUIRE(((uintptr_t)out & 15) == 0, "mpg_inflate_units: out must be 16-byte aligned");
    MPG_REQUIRE(n_bytes >= 4 && n_bytes % 4 == 0, "mpg_inflate_units: %zu bytes is not a positive multiple of 4", n_bytes);
    MPG_REQUIRE(n_units == (n_bytes + UNIT - 1) / UNIT && n_units <= (size_t)1 << 24, "mpg_inflate_units: %zu units for %zu bytes", n_units,
                n_bytes);
    for (size_t u = 0; u < n_units; ++u) {
        MPG_REQUIRE(sizes[u] <= mpg_inflate::MAX_STREAM, "mpg_inflate_units: unit %zu: a stream of %u bytes", u, sizes[u]);
        MPG_REQUIRE(offsets[u] <= packed_bytes && sizes[u] <= packed_bytes - offsets[u],
                    "mpg_inflate_units: unit %zu (offset %llu, %u bytes) leaves the %zu packed bytes", u, (unsigned long long)offsets[u],
                    sizes[u], packed_bytes);
    }
    // offsets and sizes travel in one block of device memory that lives in stream order
    const hipStream_t hs = (hipStream_t)stream;
    const size_t off_bytes = n_units * sizeof(unsigned long long), all_bytes = off_bytes + n_units * sizeof(uint32_t);
    std::vector<unsigned char> host(all_bytes);
    for (size_t u = 0; u < n_units; ++u) {
        reinterpret_cast<unsigned long long*>(host.data())[u] = offsets[u];
        reinterpret_cast<uint32_t*>(host.data() + off_bytes)[u] = sizes[u];
    }
    void* dev = nullptr;
    hipError_t e = hipMallocAsync(&dev, all_bytes, hs);
    if (e != hipSuccess) return mpg::hip_check(e, "mpg_inflate_units: hipMallocAsync");
    e = hipMemcpyAsync(dev, host.data(), all_bytes, hipMemcpyHostToDevice, hs);
    if (e == hipSuccess) e = hipStreamSynchronize(hs);                       // `host` is free to go
    if (e != hipSuccess) {
        (void)hipFreeAsync(dev, hs);
        return mpg::hip_check(e, "mpg_inflate_units: descriptor upload");
    }
    const unsigned grid = n_units < 256u * 32u ? (unsigned)n_units : 256u * 32u;
    hipLaunchKernelGGL(inflate_units_kernel, dim3(grid), dim3(64), 0, hs, reinterpret_cast<const unsigned char*>(packed),
                       reinterpret_cast<const unsigned long long*>(dev),
                       reinterpret_cast<const uint32_t*>(reinterpret_cast<unsigned char*>(dev) + off_bytes), (unsigned)n_units,
                       reinterpret_cast<unsigned char*>(out), n_bytes, crcs, status);
    const hipError_t launched = hipGetLastError();
    e = hipFreeAsync(dev, hs);
    if (launched != hipSuccess) return mpg::hip_check(launched, "inflate_units_kernel");
    return mpg::hip_check(e, "mpg_inflate_units: hipFreeAsync");
}
