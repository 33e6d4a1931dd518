// Checks csrc/encoded_plan.hpp, the host's decisions about a batch of encoded frames, without a GPU (tests/test_encoded_plan.py builds this
// with the address and undefined-behaviour sanitizers and runs it in its own process).  Every expected value is a literal worked out by
// hand from the formats; every buffer is a heap block of exactly the bytes it stands for, the chunk under test last, so that a read past a
// chunk's end is a sanitizer report.  Prints a FAIL line per mismatch and OK at the end.
#include <cstdio>
#include <cstring>
#include <memory>

#include "encoded_plan.hpp"

using namespace ffsamd;
using Ranges = std::vector<std::pair<size_t, size_t>>;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

static std::unique_ptr<uint8_t[]> block(size_t n, uint8_t fill = 0xEE) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    std::memset(p.get(), fill, n);
    return p;
}

static void blocking() {
    for (const size_t es : {(size_t)2, (size_t)4}) {
        const uint32_t B = es == 2 ? 4096u : 2048u;   // 8192 bytes of elements
        const struct { size_t n; uint32_t blocks, last, tail; } cases[] = {
            {7, 0, B, 7}, {8, 1, 8, 0}, {B, 1, B, 0}, {(size_t)B + 7, 1, B, 7}, {(size_t)B + 8, 2, 8, 0}, {(size_t)B + 9, 2, 8, 1}, {2 * (size_t)B + 15, 3, 8, 7}};
        for (const auto& k : cases) {
            const BshufBlocking g = bshuf_blocking(k.n, es);
            CHECK(g.block_elems == B && g.blocks == k.blocks && g.last_elems == k.last && g.tail_elems == k.tail);
        }
    }
}

static void chunk_check() {   // frames of 5 x 3 pixels of 2 bytes: 30 raw bytes, 0x1E
    std::string why;
    const auto lz4 = [&](const uint8_t* p, size_t n) { why.clear(); return chunk_ok(FFS_CODEC_BSLZ4, p, n, 5, 3, 2, why); };
    const auto bo = [&](const uint8_t* p, size_t n) { why.clear(); return chunk_ok(FFS_CODEC_BYTE_OFFSET, p, n, 5, 3, 2, why); };
    const char* const too_short = "ffs_submit_compressed: a chunk is shorter than its 12-byte header";
    CHECK(!lz4(nullptr, 100) && why == too_short);
    auto h11 = block(11, 0);
    h11[7] = 30;
    CHECK(!lz4(h11.get(), 11) && why == too_short);
    auto h12 = block(12, 0);
    h12[7] = 30;
    CHECK(lz4(h12.get(), 12) && why.empty());
    h12[7] = 31;
    CHECK(!lz4(h12.get(), 12) && why == "ffs_submit_compressed: chunk header says 31 bytes, the context's frames have 30");
    h12[7] = 29;
    CHECK(!lz4(h12.get(), 12) && why == "ffs_submit_compressed: chunk header says 29 bytes, the context's frames have 30");
    h12[7] = 30;
    h12[0] = 1;   // the total is eight bytes, big-endian: 2^56 + 30
    CHECK(!lz4(h12.get(), 12) && why == "ffs_submit_compressed: chunk header says 72057594037927966 bytes, the context's frames have 30");
    auto b14 = block(14), b15 = block(15);
    CHECK(!bo(b14.get(), 14) && why == "ffs_submit_encoded: a byte-offset chunk of 14 bytes cannot hold a frame of 15 pixels");
    CHECK(bo(b15.get(), 15) && why.empty());
    CHECK(!bo(nullptr, 15) && why == "ffs_submit_encoded: a byte-offset chunk of 0 bytes cannot hold a frame of 15 pixels");
}

static void placement() {
    auto stage = block(1000);
    const uint8_t* S = stage.get();
    std::vector<size_t> base;
    Placement pl;
    {   // nothing in place: 16-aligned running sums of the sizes, one of them a multiple of 16 already
        auto a = block(5), b = block(16), c = block(33), d = block(1);
        const void* chunks[] = {a.get(), b.get(), c.get(), d.get()};
        const size_t bytes[] = {5, 16, 33, 1};
        for (const bool with_stage : {true, false}) {
            base.assign(7, 99);
            CHECK(place_chunks(chunks, bytes, 4, with_stage ? S : nullptr, with_stage ? 1000 : 0, base, pl));
            CHECK(!pl.in_place && base == (std::vector<size_t>{0, 16, 32, 80}) && pl.lo == 0 && pl.hi == 96 && pl.staging == 96 + 24 + 4096);
        }
    }
    {   // everything in place, at odd offsets and in no order
        const void* chunks[] = {S + 35, S + 19, S + 501};
        const size_t bytes[] = {10, 7, 99};
        CHECK(place_chunks(chunks, bytes, 3, S, 1000, base, pl));
        CHECK(pl.in_place && base == (std::vector<size_t>{35, 19, 501}) && pl.lo == 16 && pl.hi == 600);
    }
    {   // a chunk that ends with the buffer lies in it; one byte longer and it does not
        const void* chunks[] = {S + 3, S + 990};
        size_t bytes[] = {4, 10};
        CHECK(place_chunks(chunks, bytes, 2, S, 1000, base, pl));
        CHECK(pl.in_place && base == (std::vector<size_t>{3, 990}) && pl.lo == 0 && pl.hi == 1000);
        bytes[1] = 11;
        base.assign(2, 77);
        CHECK(!place_chunks(chunks, bytes, 2, S, 1000, base, pl) && base == (std::vector<size_t>{77, 77}));
        CHECK(place_chunks(chunks + 1, bytes + 1, 1, S, 1000, base, pl));   // ... alone: to be copied
        CHECK(!pl.in_place && base == (std::vector<size_t>{0}) && pl.hi == 16);
    }
    {   // one of three outside
        auto out = block(8);
        const void* chunks[] = {S + 100, out.get(), S + 200};
        const size_t bytes[] = {8, 8, 8};
        CHECK(!place_chunks(chunks, bytes, 3, S, 1000, base, pl));
    }
    {   // the sizes alone decide the copied case (nothing is read): 2^32 - 16 staged bytes pass the limit, one byte more does not
        auto a = block(1);
        const void* chunks[] = {a.get(), a.get()};
        size_t bytes[] = {0x80000000ull, 0x7FFFFFF0ull};
        CHECK(place_chunks(chunks, bytes, 2, S, 1000, base, pl) && base[1] == 0x80000000ull && pl.hi == 0xFFFFFFF0ull && pl.hi <= kMaxStagedBytes);
        bytes[1] = 0x7FFFFFF1ull;
        CHECK(place_chunks(chunks, bytes, 2, S, 1000, base, pl) && pl.hi == 0x100000000ull && pl.hi > kMaxStagedBytes);
    }
}

static void ranges() {
    Ranges r;
    {
        const size_t base[] = {35}, bytes[] = {10};
        copy_ranges(base, bytes, 1, r);
        CHECK(r == (Ranges{{32, 45}}));
    }
    {   // descending addresses, each more than 512 KiB from the next
        const size_t base[] = {2000005, 1000000, 5}, bytes[] = {10, 20, 30};
        copy_ranges(base, bytes, 3, r);
        CHECK(r == (Ranges{{0, 35}, {1000000, 1000020}, {2000000, 2000015}}));
    }
    {   // a chunk inside another's range does not shorten it
        const size_t base[] = {100, 0}, bytes[] = {10, 1000};
        copy_ranges(base, bytes, 2, r);
        CHECK(r == (Ranges{{0, 1000}}));
    }
    // the first range ends at 96; 96 + 524288 = 524384 = 16 * 32774: a begin there still merges, and so does a chunk at 524399 (its begin
    // rounds down to it); 524400 is the next 16-byte step
    const size_t bytes[] = {96, 10};
    for (const size_t second : {(size_t)524384, (size_t)524399}) {
        const size_t base[] = {0, second};
        copy_ranges(base, bytes, 2, r);
        CHECK(r == (Ranges{{0, second + 10}}));
    }
    const size_t base[] = {0, 524400};
    copy_ranges(base, bytes, 2, r);
    CHECK(r == (Ranges{{0, 96}, {524400, 524410}}));
}

// [4-byte big-endian length][that many bytes] at p; returns the byte behind it.  `have`: the payload bytes actually present.
static size_t put_block(uint8_t* p, uint32_t len, size_t have) {
    const uint8_t word[4] = {(uint8_t)(len >> 24), (uint8_t)(len >> 16), (uint8_t)(len >> 8), (uint8_t)len};
    std::memcpy(p, word, 4);
    std::memset(p + 4, 0x55, have);
    return 4 + have;
}

static void walk() {
    // Three blocks a frame, a raw tail of 3 two-byte elements.  Chunk 0 at 0: header 12, blocks of 5, 1 and 300 (01 2C) bytes, tail:
    // 12 + 9 + 5 + 304 + 6 = 336 bytes.  Chunk 1 at 336: blocks of 2, 66051 (00 01 02 03) and 7 bytes: 12 + 6 + 66055 + 11 + 6 = 66090.
    const uint32_t len0[3] = {5, 1, 300}, len1[3] = {2, 66051, 7};
    const size_t base[2] = {0, 336};
    const auto build = [&](size_t bytes1, size_t payload_of_last) {   // chunk 1 cut to bytes1, its last block present with that many payload bytes
        auto st = block(336 + bytes1);
        size_t at = 12;
        for (const uint32_t l : len0) at += put_block(st.get() + at, l, l);
        at = 336 + 12;
        for (int b = 0; b < 3 && at + 4 <= 336 + bytes1; ++b) at += put_block(st.get() + at, len1[b], b == 2 ? payload_of_last : len1[b]);
        return st;
    };
    const std::vector<uint32_t> want = {16, 5, 25, 1, 30, 300, 330, 6, 352, 2, 358, 66051, 66413, 7, 66420, 6};
    const auto flat = [](const std::vector<BlockEntry>& t) {
        std::vector<uint32_t> v;
        for (const BlockEntry& e : t) v.insert(v.end(), {e.offset, e.bytes});
        return v;
    };
    {
        const size_t bytes[2] = {336, 66090};
        auto st = build(66090, 7);
        std::vector<BlockEntry> whole(8, BlockEntry{9, 9}), split(8, BlockEntry{9, 9});
        size_t pos[2] = {12, 12};
        CHECK(walk_block_chains(st.get(), base, bytes, pos, 0, 2, 3, 6, whole.data()) && pos[0] == 330 && pos[1] == 66084);
        size_t pos2[2] = {12, 12};
        CHECK(walk_block_chains(st.get(), base, bytes, pos2, 0, 1, 3, 6, split.data()));
        CHECK(walk_block_chains(st.get(), base, bytes, pos2, 1, 2, 3, 6, split.data()));
        CHECK(flat(whole) == want && flat(split) == want);
    }
    const struct { size_t bytes1, last_payload; } bad[] = {
        {12 + 6 + 2, 0},                  // ends inside the second length word
        {12 + 6 + 66055 + 4 + 3, 3},      // the last block says 7 bytes, 3 are there (and no tail)
        {12 + 6 + 66055 + 11, 7},         // every block whole, the tail missing
    };
    for (const auto& k : bad) {
        const size_t bytes[2] = {336, k.bytes1};
        auto st = build(k.bytes1, k.last_payload);
        std::vector<BlockEntry> tab(8);
        size_t pos[2] = {12, 12};
        CHECK(!walk_block_chains(st.get(), base, bytes, pos, 0, 2, 3, 6, tab.data()));
        size_t pos1[2] = {12, 12};
        CHECK(!walk_block_chains(st.get(), base, bytes, pos1, 1, 2, 3, 6, tab.data()));
        CHECK(walk_block_chains(st.get(), base, bytes, pos1, 0, 1, 3, 6, tab.data()));   // chunk 0 is whole
    }
}

static void byte_offset_table() {   // 2000 pixels: at most 14000 bytes are parsed, tiles of 4096
    const size_t base[] = {16, 4128, 24128}, bytes[] = {4096, 20000, 4097};
    std::vector<BoFrame> fr(3, BoFrame{9, 9, 9, 9});
    const BoTiles t = bo_frame_table(base, bytes, 3, 2000, fr.data());
    const uint32_t want[3][4] = {{16, 4096, 0, 0}, {4128, 14000, 1, 0}, {24128, 4097, 5, 0}};
    for (int f = 0; f < 3; ++f) CHECK(fr[f].base == want[f][0] && fr[f].end == want[f][1] && fr[f].tile0 == want[f][2] && fr[f].total == want[f][3]);
    CHECK(t.sum == 7 && t.max_tiles == 4);
    CHECK(bo_tiles(0) == 0 && bo_tiles(1) == 1 && bo_tiles(4096) == 1 && bo_tiles(4097) == 2);
}

int main() {
    blocking();
    chunk_check();
    placement();
    ranges();
    walk();
    byte_offset_table();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("OK\n");
    return failures ? 1 : 0;
}
