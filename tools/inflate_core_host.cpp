// The decode core of the device .uni reader (multi-pass-gan_amd/csrc/mpgan_inflate_core.h) as a stand-alone CPU program,
// for a sanitizer build:
//   g++ -O1 -g -fsanitize=address,undefined -I multi-pass-gan_amd/csrc tools/inflate_core_host.cpp -o inflate_core_host
//   inflate_core_host streams.bin results.bin
// streams.bin: uint32 count, then per stream uint32 lead (0..15: where the stream starts in its first 16-byte line), uint32
// size, uint32 out_bytes and the size bytes.  results.bin: per stream uint32 status, uint32 CRC-32 of the bytes produced,
// uint32 their count, and the bytes.  Input and output live in heap blocks of exactly the sizes the core may touch (the
// stream's 16-byte lines; out_bytes), so the sanitizer sees any step outside them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpgan_inflate_core.h"

namespace {

struct HostIO {
    const unsigned char* in;     // the stream's 16-byte lines
    uint32_t* out;
    uint32_t n_out;
    uint32_t word(uint32_t i) const {
        uint32_t w;
        std::memcpy(&w, in + 4 * (size_t)i, 4);
        return w;
    }
    void put(uint32_t w) { out[n_out++] = w; }
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
};

uint32_t crc32(const unsigned char* p, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return c ^ 0xffffffffu;
}

bool read_u32(std::FILE* f, uint32_t& v) { return std::fread(&v, 4, 1, f) == 1; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s streams.bin results.bin\n", argv[0]);
        return 2;
    }
    std::FILE* fi = std::fopen(argv[1], "rb");
    std::FILE* fo = fi ? std::fopen(argv[2], "wb") : nullptr;
    uint32_t count = 0;
    if (!fi || !fo || !read_u32(fi, count)) {
        std::fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    mpg_inflate::Tables* tables = new mpg_inflate::Tables;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t lead = 0, size = 0, out_bytes = 0;
        if (!read_u32(fi, lead) || !read_u32(fi, size) || !read_u32(fi, out_bytes) || lead > 15 || size > (64u << 20) ||
            out_bytes > (64u << 20)) {
            std::fprintf(stderr, "stream %u: bad record\n", k);
            return 2;
        }
        const size_t lines = ((size_t)lead + size + 15) / 16 * 16;
        unsigned char* in = static_cast<unsigned char*>(std::malloc(lines ? lines : 1));
        uint32_t* out = static_cast<uint32_t*>(std::malloc(out_bytes ? out_bytes : 1));
        std::memset(in, 0xA5, lines);
        if (size && std::fread(in + lead, 1, size, fi) != size) {
            std::fprintf(stderr, "stream %u: short file\n", k);
            return 2;
        }
        HostIO io{in, out, 0};
        const uint32_t status = (uint32_t)mpg_inflate::inflate_unit(io, *tables, lead, size, out_bytes);
        const uint32_t produced = 4 * io.n_out;
        const uint32_t crc = crc32(reinterpret_cast<const unsigned char*>(out), produced);
        std::fwrite(&status, 4, 1, fo);
        std::fwrite(&crc, 4, 1, fo);
        std::fwrite(&produced, 4, 1, fo);
        std::fwrite(out, 1, produced, fo);
        std::free(in);
        std::free(out);
    }
    delete tables;
    std::fclose(fi);
    return std::fclose(fo) == 0 ? 0 : 2;
}
