// CRC-32 (gzip, bit-reflected) pieces shared by the device .uni writer (mpgan_deflate.hip) and reader (mpgan_inflate.hip):
// the slice-by-4 byte tables and the GF(2) product that moves a CRC register past later bytes.
#pragma once
#include <cstdint>

namespace mpg_crc {

constexpr uint32_t POLY = 0xEDB88320u;

// a * b mod P in the reflected representation (bit 31 is x^0), as zlib's multmodp
constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
    }
    return p;
}

// slice-by-4: t[k][b] = register after byte b and k zero bytes
constexpr void fill_slice_tables(uint32_t (&t)[4][256]) {
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t c = b;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? POLY : 0u);
        t[0][b] = c;
    }
    for (int k = 1; k < 4; ++k)
        for (int b = 0; b < 256; ++b) t[k][b] = (t[k - 1][b] >> 8) ^ t[0][t[k - 1][b] & 255u];
}

}  // namespace mpg_crc
