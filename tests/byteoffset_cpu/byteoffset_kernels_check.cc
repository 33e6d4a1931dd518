// The three byte-offset kernels (csrc/kernels_byteoffset.hpp) run on the host, lane by lane, against the host decoder of
// host/codecs.hpp: token mixes that put a tile or segment cut at every offset inside a token, chunks at odd offsets, trailing bytes,
// chunks that end early (status bit, zeros).  The chunk buffer has exactly the 64 bytes of slack the library gives it and the
// image has padding that must stay untouched, so the program is also what to run under -fsanitize=address.
#include "kernels_byteoffset.hpp"
#include "codecs.hpp"   // (host/, on the include path)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
using namespace ffsamd;
template <typename PixelT>
static int run(uint32_t W, uint32_t H, const std::vector<std::vector<uint8_t>>& chunks, const std::vector<size_t>& gaps, const char* what) {
    const uint32_t n = chunks.size();
    std::vector<size_t> base(n); size_t cur = gaps[0];
    for (uint32_t f = 0; f < n; ++f) { base[f] = cur; cur += chunks[f].size() + gaps[(f + 1) % gaps.size()]; }
    const size_t hi = cur;
    uint8_t* comp = (uint8_t*)malloc(hi + 64);   // exact: ASan sees any over-read
    memset(comp, 0x80, hi + 64);
    std::vector<BoFrame> fr(n); size_t tiles = 0; uint32_t max_tiles = 0;
    for (uint32_t f = 0; f < n; ++f) {
        memcpy(comp + base[f], chunks[f].data(), chunks[f].size());
        fr[f] = {(uint32_t)base[f], (uint32_t)std::min<uint64_t>(chunks[f].size(), 7ull * W * H), (uint32_t)tiles, 0};
        tiles += bo_tiles(fr[f].end); max_tiles = std::max(max_tiles, bo_tiles(fr[f].end));
    }
    uint2* lane = (uint2*)malloc(tiles * 448 * 8); uint2* map = (uint2*)malloc(tiles * 7 * 8); uint4* state = (uint4*)malloc(tiles * 16);
    const uint32_t pitch = ((W * sizeof(PixelT) + 15) / 16) * 16 + 16; const uint64_t fs = (uint64_t)pitch * H;
    uint8_t* img = (uint8_t*)malloc(fs * n); memset(img, 0xAB, fs * n);
    uint32_t err = 0;
    BoArgs a{comp, fr.data(), lane, map, state, img, fs, pitch, W, H, &err};
    launch(k_bo_summarise, max_tiles, n, a);
    launch(k_bo_compose, n, 1, a);
    launch(k_bo_emit<PixelT>, max_tiles, n, a);
    int bad = 0; bool any_short = false;
    for (uint32_t f = 0; f < n; ++f) {
        std::vector<PixelT> want((size_t)W * H, 0);
        const size_t k = ffshost::byte_offset_decompress(chunks[f].data(), chunks[f].size(), want.data(), (size_t)W * H);
        if (k < (size_t)W * H) any_short = true;
        for (uint32_t y = 0; y < H; ++y) for (uint32_t x = 0; x < W; ++x) {
            const PixelT g = *(PixelT*)(img + f * fs + (size_t)y * pitch + x * sizeof(PixelT));
            if (g != want[(size_t)y * W + x]) { if (!bad++) printf("%s: frame %u (%u,%u) got %u want %u\n", what, f, y, x, (unsigned)g, (unsigned)want[(size_t)y * W + x]); }
        }
        for (uint32_t y = 0; y < H; ++y) for (uint32_t b = W * sizeof(PixelT); b < pitch; ++b) if (img[f * fs + (size_t)y * pitch + b] != 0xAB) { if (!bad++) printf("%s: pad written\n", what); }
    }
    if (any_short != ((err & 256u) != 0)) { printf("%s: flag %u but short=%d\n", what, err, (int)any_short); ++bad; }
    free(comp); free(lane); free(map); free(state); free(img);
    printf("%s %ux%u es=%zu n=%u tiles=%zu: %s\n", what, W, H, sizeof(PixelT), n, tiles, bad ? "FAIL" : "ok");
    return bad;
}
int main() {
    std::mt19937 rng(3); int bad = 0;
    for (auto [W, H] : {std::pair<uint32_t, uint32_t>{3, 1}, {7, 1}, {1, 300}, {67, 45}, {200, 37}}) {
        const size_t n = (size_t)W * H;
        std::vector<std::vector<uint8_t>> cs;
        std::vector<int32_t> v(n);
        for (auto& x : v) x = (int32_t)rng(); cs.push_back(ffshost::byte_offset_compress(v.data(), n));
        for (auto& x : v) x = 0; cs.push_back(ffshost::byte_offset_compress(v.data(), n));
        const int64_t cyc[8] = {128, -128, -32640, 32768, -2139062144ll, -2147483648ll, 127, -127};
        { uint32_t c = 0; for (size_t i = 0; i < n; ++i) { c += (uint32_t)cyc[i % 8]; v[i] = (int32_t)c; } } cs.push_back(ffshost::byte_offset_compress(v.data(), n));
        for (int p = 0; p < 7; ++p) for (int big : {100000, 1000}) { int32_t c = 0; for (size_t i = 0; i < n; ++i) { c += (int)i < p ? 1 : (i % 2 ? -big : big); v[i] = c; } cs.push_back(ffshost::byte_offset_compress(v.data(), n)); }
        auto with_trailer = cs; for (auto& c : with_trailer) { c.insert(c.end(), 700, 0); c.insert(c.end(), 300, 0x80); }
        bad += run<uint16_t>(W, H, cs, {0}, "packed"); bad += run<uint32_t>(W, H, cs, {1, 3, 2, 7, 5}, "odd offsets");
        bad += run<uint32_t>(W, H, with_trailer, {3}, "trailer"); bad += run<uint16_t>(W, H, with_trailer, {0, 16}, "trailer16");
        // truncated
        std::vector<std::vector<uint8_t>> tr;
        for (int cut = 1; cut <= 8 && (size_t)cut < cs[0].size(); ++cut) tr.push_back(std::vector<uint8_t>(cs[0].begin(), cs[0].end() - cut));
        tr.push_back(std::vector<uint8_t>(cs[4].begin(), cs[4].begin() + std::max<size_t>(n, 1)));
        bad += run<uint32_t>(W, H, tr, {5, 1}, "truncated");
    }
    printf(bad ? "EMU FAIL\n" : "EMU OK\n");
    return bad != 0;
}
