// encoded_plan.hpp -- the host's decisions about a batch of encoded frames (bitshuffle-LZ4, CBF byte-offset and raw Jungfrau chunks) as plain
// arithmetic: no HIP header, no allocation of device or pinned memory, no copy.  ffs_encoded.hip acts on them; the decode kernels
// (kernels_decode.hpp, kernels_byteoffset.hpp) share the constants and BoFrame; tests/encoded_plan_check.cc compiles the same text.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "ffs_hip.h"

namespace ffsamd {

// ---- bitshuffle-LZ4: blocking --------------------------------------------------------------------------------------------------
constexpr int kDecBlockBytes = 8192;                 // bitshuffle target block size

// bitshuffle's blocking of a frame of `nelem` elements (bshuf_default_block_size, and the loop of bshuf_blocked_wrap_fun): full blocks
// of 8192 / elem_bytes elements, a last block of the remaining multiple of 8 (none when fewer than 8 remain), the rest raw
struct BshufBlocking {
    uint32_t block_elems = 0;   // elements of a full block
    uint32_t blocks = 0;        // LZ4 blocks of a frame, the shortened last one included
    uint32_t last_elems = 0;    // elements of the last LZ4 block
    uint32_t tail_elems = 0;    // raw elements behind it (< 8)
};
inline BshufBlocking bshuf_blocking(size_t nelem, size_t elem_bytes) {
    const size_t block = (size_t)kDecBlockBytes / elem_bytes;
    const size_t n_full = nelem / block, rem = nelem - n_full * block;
    return {(uint32_t)block, (uint32_t)(n_full + (rem >= 8 ? 1 : 0)), (uint32_t)(rem >= 8 ? rem / 8 * 8 : block), (uint32_t)(rem % 8)};
}

// ---- one chunk against the context's frames ------------------------------------------------------------------------------------
// true: the chunk may hold a frame of W x H pixels of elem_bytes.  false: `why` has the refusal.  bitshuffle-LZ4: a 12-byte header whose
// first 8 bytes are the frame's raw size, big-endian; byte-offset: no header, every element takes at least one byte; raw Jungfrau words:
// exactly W * H 16-bit words, into 32-bit pixels only.
inline bool chunk_ok(int codec, const void* chunk, size_t bytes, size_t W, size_t H, size_t elem_bytes, std::string& why) {
    const uint8_t* p = static_cast<const uint8_t*>(chunk);
    if (codec == FFS_CODEC_JUNGFRAU_RAW) {
        if (elem_bytes != 4) {
            why = "ffs_submit_encoded: raw Jungfrau words convert to 32-bit photon counts: the context must have pixel_bytes 4, this one has "
                  + std::to_string(elem_bytes);
            return false;
        }
        if (p && bytes == W * H * 2) return true;
        why = "ffs_submit_encoded: a raw Jungfrau chunk of " + std::to_string(p ? bytes : 0) + " bytes is not a frame of " + std::to_string(W * H)
              + " 16-bit words (" + std::to_string(W * H * 2) + " bytes)";
        return false;
    }
    if (codec == FFS_CODEC_BYTE_OFFSET) {
        if (p && bytes >= W * H) return true;
        why = "ffs_submit_encoded: a byte-offset chunk of " + std::to_string(p ? bytes : 0) + " bytes cannot hold a frame of " + std::to_string(W * H)
              + " pixels";
        return false;
    }
    if (!p || bytes < 12) {
        why = "ffs_submit_compressed: a chunk is shorter than its 12-byte header";
        return false;
    }
    uint64_t total = 0;
    for (int i = 0; i < 8; ++i) total = (total << 8) | p[i];
    if (total == W * H * elem_bytes) return true;
    why = "ffs_submit_compressed: chunk header says " + std::to_string(total) + " bytes, the context's frames have " + std::to_string(W * H * elem_bytes);
    return false;
}

// ---- where the chunks lie in the staging buffer ----------------------------------------------------------------------------------
// Either every chunk lies inside the stream's staging buffer [stage, stage + stage_bytes) already (in place: base[f] is where), or none
// does and the caller copies chunk f to base[f], the 16-aligned running sum of the sizes -- after it has made the buffer hold `staging`
// bytes (the bases depend on the sizes alone).  [lo, hi): the bytes of the buffer the chunks span, lo rounded down to 16.
constexpr size_t kMaxStagedBytes = 0xFFFFFFF0ull;   // the tables hold 32-bit offsets: a larger `hi` is refused (after the staging request)
constexpr size_t kMergeGap = 524288;                // copy ranges closer than this travel as one copy

struct Placement {
    bool in_place = false;
    size_t lo = 0, hi = 0;
    size_t staging = 0;   // not in place: the bytes to ask for, with headroom
};
// false: some chunks lie in the buffer and some do not (`base` is not written)
inline bool place_chunks(const void* const* chunks, const size_t* bytes, uint32_t n, const void* stage, size_t stage_bytes, std::vector<size_t>& base,
                         Placement& pl) {
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(stage);
    uint32_t inside = 0;
    for (uint32_t f = 0; f < n; ++f) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(chunks[f]);
        if (a >= s0 && a + bytes[f] <= s0 + stage_bytes) ++inside;
    }
    if (inside != 0 && inside != n) return false;
    pl = Placement{inside != 0};
    base.assign(n, 0);
    if (pl.in_place) {
        pl.lo = SIZE_MAX;
        for (uint32_t f = 0; f < n; ++f) {
            base[f] = reinterpret_cast<uintptr_t>(chunks[f]) - s0;
            pl.lo = std::min(pl.lo, base[f]);
            pl.hi = std::max(pl.hi, base[f] + bytes[f]);
        }
        pl.lo &= ~(size_t)15;
    } else {
        for (uint32_t f = 0; f < n; ++f) {
            base[f] = pl.hi;
            pl.hi = (pl.hi + bytes[f] + 15) & ~(size_t)15;
        }
        pl.staging = pl.hi + pl.hi / 4 + 4096;
    }
    return true;
}

// Raw Jungfrau words are loaded 16 bytes at a time from where the chunk lies: the staged bases are multiples of 16 by construction, a chunk
// the caller placed in the buffer must be.  The index of the first chunk that is not, or n.
inline uint32_t first_unaligned_base(const size_t* base, uint32_t n) {
    for (uint32_t f = 0; f < n; ++f)
        if (base[f] % 16 != 0) return f;
    return n;
}

// Chunks placed by the caller (a driver's fixed slots leave gaps between them): only the bytes of the chunks cross PCIe.  r: n entries
// to work in; on return the sorted, merged [begin, end) ranges to copy, each begin rounded down to 16 -- ranges closer than kMergeGap are
// one (the gap costs what a copy of its own would).
inline void copy_ranges(const size_t* base, const size_t* bytes, uint32_t n, std::vector<std::pair<size_t, size_t>>& r) {
    r.resize(n);
    for (uint32_t f = 0; f < n; ++f) r[f] = {base[f] & ~(size_t)15, base[f] + bytes[f]};
    std::sort(r.begin(), r.end());
    size_t m = 0;
    for (uint32_t f = 1; f < n; ++f) {
        if (r[f].first <= r[m].second + kMergeGap) r[m].second = std::max(r[m].second, r[f].second);
        else r[++m] = r[f];
    }
    r.resize(n ? m + 1 : 0);
}

// ---- bitshuffle-LZ4: the block table ---------------------------------------------------------------------------------------------
// DecodeArgs::table (a uint2 there): where a block's payload lies in the staged bytes, and its length
struct BlockEntry { uint32_t offset, bytes; };
// Behind its header a chunk is a chain of [4-byte big-endian length][payload] per block and then the raw tail.  Walks the chains of frames
// [f0, f1) side by side (so that their cache misses overlap) from pos[f] (12 at the start; left behind the last block) and writes rows
// f0 .. f1 - 1 of tab[n][blocks + 1], the tail's entry last.  `stage + base[f]` is chunk f, bytes[f] long.  false: a length word or the
// tail runs past the end of its chunk (no length word is read that does).
inline bool walk_block_chains(const uint8_t* stage, const size_t* base, const size_t* bytes, size_t* pos, uint32_t f0, uint32_t f1, uint32_t blocks,
                              size_t tail_bytes, BlockEntry* tab) {
    const size_t stride = (size_t)blocks + 1;
    for (uint32_t b = 0; b < blocks; ++b)
        for (uint32_t f = f0; f < f1; ++f) {
            if (pos[f] + 4 > bytes[f]) return false;
            const uint8_t* p = stage + base[f] + pos[f];
            const uint32_t clen = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            tab[f * stride + b] = {(uint32_t)(base[f] + pos[f] + 4), clen};
            pos[f] += 4 + (size_t)clen;
        }
    bool ok = true;
    for (uint32_t f = f0; f < f1; ++f) {
        if (pos[f] + tail_bytes > bytes[f]) ok = false;
        tab[f * stride + blocks] = {(uint32_t)(base[f] + pos[f]), (uint32_t)tail_bytes};
    }
    return ok;
}

// ---- CBF byte-offset: the frame table --------------------------------------------------------------------------------------------
constexpr int kBoSeg = 64;                               // bytes per lane
constexpr int kBoTile = 64 * kBoSeg;                     // bytes per wave

struct BoFrame {            // one per frame of the batch (host-written; k_bo_compose fills in `total`)
    uint32_t base;          // the chunk's offset in `comp`
    uint32_t end;           // parse bound: min(chunk_bytes, 7 W H)
    uint32_t tile0;         // index of the chunk's first tile in the batch's tables
    uint32_t total;         // elements the chunk holds (k_bo_compose)
};
// (constexpr: the kernels call it too)
constexpr uint32_t bo_tiles(uint32_t end) { return (end + (uint32_t)kBoTile - 1u) / (uint32_t)kBoTile; }

// tiles of the whole batch (what the summary tables must hold) and of its longest chunk (the launches' grid)
struct BoTiles { size_t sum = 0; uint32_t max_tiles = 0; };
// fr[n]: where every chunk lies, how much of it is parsed (seven bytes per element at the most: nothing behind that is ever parsed) and
// where its tiles lie in the summary tables
inline BoTiles bo_frame_table(const size_t* base, const size_t* bytes, uint32_t n, uint64_t pixels, BoFrame* fr) {
    BoTiles t;
    for (uint32_t f = 0; f < n; ++f) {
        fr[f] = {(uint32_t)base[f], (uint32_t)std::min<uint64_t>(bytes[f], 7 * pixels), (uint32_t)t.sum, 0u};
        t.sum += bo_tiles(fr[f].end);
        t.max_tiles = std::max(t.max_tiles, bo_tiles(fr[f].end));
    }
    return t;
}

}  // namespace ffsamd
