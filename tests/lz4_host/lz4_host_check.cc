// lz4_host_check.cc -- runs the host decoders of host/codecs.hpp over a file of cases written by tests/test_lz4_blocks.py and writes
// what they returned; the test compares.  A stand-alone program: it is built twice, plain and under the address and undefined-behaviour
// sanitizers, and every input and output lives in a heap block of exactly its size, so a read or write one byte out is a report.
//
//   lz4_host_check CASES RESULTS
// CASES, per record: u16 name length, name, u8 kind, u32 capacity, u32 length, bytes.
//   kind 0: one LZ4 block for lz4_block_decompress, capacity = the bytes it must decode to;
//   kind 2, 4: a whole chunk (12-byte header included) for bshuf_decompress_lz4 with that element size, capacity = elements.
// RESULTS, per record: i64 what the decoder returned, u32 count, that many bytes of output (0 when it refused).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "codecs.hpp"

template <typename T>
static bool get(std::FILE* f, T& v) { return std::fread(&v, sizeof v, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint16_t name_len;
    unsigned n = 0;
    while (get(in, name_len)) {
        std::string name(name_len, '\0');
        uint8_t kind;
        uint32_t cap, len;
        if (std::fread(name.data(), 1, name_len, in) != name_len || !get(in, kind) || !get(in, cap) || !get(in, len)) return 3;
        std::unique_ptr<uint8_t[]> src(new uint8_t[len]);   // (new[0] is a valid block of no bytes)
        if (len && std::fread(src.get(), 1, len, in) != len) return 3;
        const size_t out_bytes = kind == 0 ? cap : (size_t)cap * kind;
        std::unique_ptr<uint8_t[]> dst(new uint8_t[out_bytes]);
        std::memset(dst.get(), 0xEE, out_bytes);
        long r;
        if (kind == 0) r = ffshost::lz4_block_decompress(src.get(), len, dst.get(), cap);
        else r = len < 12 ? -1 : ffshost::bshuf_decompress_lz4(src.get() + 12, len - 12, dst.get(), cap, kind);
        const int64_t ret = r;
        const uint32_t count = r < 0 ? 0u : (uint32_t)(kind == 0 ? (size_t)r : out_bytes);
        std::fwrite(&ret, sizeof ret, 1, out);
        std::fwrite(&count, sizeof count, 1, out);
        if (count) std::fwrite(dst.get(), 1, count, out);
        ++n;
    }
    if (std::fclose(out) != 0) return 4;
    std::printf("%u cases\n", n);
    return 0;
}
