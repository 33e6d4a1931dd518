// kernels_byteoffset.hpp (included by ffs_encoded.hip) -- CBF byte-offset chunk decode on the GPU.
//
// What the reference does: CBFRead::get_image decodes the binary section on the reading thread (cbfread.hpp:49-106,
// decompress_byte_offset) and the raw frame crosses PCIe.  Here the section crosses PCIe as it lies in the file and is decoded
// into the pitched device image the threshold kernels read.
//
// The codec: current = 0 (32 bits); a token is one byte c != 0x80 (current += int8), or 0x80 + two bytes s != 0x8000
// (current += int16), or 0x80 00 80 + four bytes (current += int32); every token emits `current`.  Where a token starts depends on
// every byte before it, and its value on every token before it: a serial chain, cut here into three launches.
//
// A token that starts before a cut at byte E makes the next token start at E + r, r in 0..6, so a piece of the chunk is summarised
// by a map over those 7 entry offsets: r -> (exit offset into the next piece, tokens started in the piece, sum of their deltas
// modulo 2^32).  Maps compose associatively.
//   1. k_bo_summarise: a wave per TILE of 4096 bytes, a lane per SEGMENT of 64.  The tile is staged in LDS (coalesced dword
//      loads); each lane computes its segment's map in ONE backward pass (the state of a token start at p is that of p + 1, p + 3
//      or p + 7 plus its own token: a shift register of seven states, so all seven entry offsets come out of 64 steps); seven lanes
//      then walk the 64 maps, one per entry offset of the tile, and leave the tile's map and, per entry offset, the state in which
//      every lane's segment is entered (relative to the tile's).
//   2. k_bo_compose: a wave per frame walks the tiles' maps (staged in LDS, 64 at a time) from offset 0, element 0, value 0 and
//      gives every tile its true entry state; the frame's element count decides kOvfCorruptByteOffset.
//   3. k_bo_emit: a wave per tile again; a lane looks up its segment's entry state (the table of step 1 at the tile's true entry
//      offset), parses its segment once, forwards, into an LDS array of the tile's elements, and the wave stores that array to
//      the image, consecutive lanes consecutive elements (rows end anywhere: row and column per element).
// No workgroup waits for another inside a launch; every loop is bounded by the segment, the tile or the table; a token whose bytes
// run past the parse bound min(chunk_bytes, 7 W H) emits nothing, and neither does anything behind it (it lies past the bound).
#pragma once
#include "ffs_device.h"
#include "encoded_plan.hpp"   // kBoSeg, kBoTile, BoFrame, bo_tiles: shared with the host's planning

namespace ffsamd {

constexpr int kBoRowWords = kBoSeg / 4 + 3;              // a lane's LDS row: its segment, 8 bytes of the next one, one word that spreads rows over the banks (19 is odd)
constexpr int kBoStageWords = kBoTile / 4 + 2;           // dwords staged per tile: the tile and the 8 bytes behind it

struct BoArgs {
    const uint8_t* comp;    // all chunks of the batch (64 bytes of slack behind them)
    BoFrame* frames;        // [n_frames]
    uint2* lane_pre;        // [tiles][7][64]: entering the tile at offset r, lane's segment is entered at .x & 7, after .x >> 3 elements and a delta sum of .y
    uint2* tile_map;        // [tiles][7]: the tile's map, .x = exit | count << 3, .y = delta sum
    uint4* tile_state;      // [tiles]: (true entry offset, first element, value before it, elements of the tile)
    uint8_t* image;         // pitched device frames
    uint64_t frame_stride;
    uint32_t pitch;
    uint32_t W, H;
    uint32_t* error;        // the stream's status word: kOvfCorruptByteOffset when a chunk holds fewer than W * H elements
};

// Stage tile `t` of a chunk in LDS, row per lane segment.  Dwords are loaded aligned and shifted by the chunk's misalignment; a dword
// is loaded only if it starts before the parse bound (what is not loaded reads as zero; bytes at or past the bound are never
// part of a token that counts).
__device__ __forceinline__ void bo_stage(uint32_t* s_rows, const uint8_t* comp, const BoFrame& fr, uint32_t t, int lane) {
    const uint64_t g0 = (uint64_t)fr.base + (uint64_t)t * kBoTile;   // byte address of the tile in comp
    const uint32_t sh = (uint32_t)g0 & 3u;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(comp + (g0 - sh));
    const uint64_t lim = (uint64_t)fr.base + fr.end;                 // first byte address not to be parsed
    for (uint32_t i = lane; i < (uint32_t)kBoStageWords; i += 64) {
        const uint64_t a = g0 - sh + 4ull * i;                       // aligned address of the low dword
        const uint32_t lo = a < lim ? src[i] : 0u;
        const uint32_t hi = (sh != 0u && a + 4 < lim) ? src[i + 1] : 0u;
        const uint32_t w = sh ? (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> (8u * sh)) : lo;
        const uint32_t seg = i / (kBoSeg / 4), k = i % (kBoSeg / 4);
        if (seg < 64u) s_rows[seg * kBoRowWords + k] = w;
        if (k < 2u && seg > 0u) s_rows[(seg - 1u) * kBoRowWords + kBoSeg / 4 + k] = w;   // the look-ahead of the segment before
    }
}

// one token from the 8 bytes at its start: its length and delta
__device__ __forceinline__ void bo_token(unsigned long long win, uint32_t& len, uint32_t& delta) {
    const uint32_t c = (uint32_t)win & 0xFFu, s16 = (uint32_t)(win >> 8) & 0xFFFFu;
    const bool one = c != 0x80u, three = s16 != 0x8000u;
    len = one ? 1u : three ? 3u : 7u;
    delta = one ? (uint32_t)(int32_t)(int8_t)c : three ? (uint32_t)(int32_t)(int16_t)s16 : (uint32_t)(win >> 24);
}

__global__ __launch_bounds__(64) void k_bo_summarise(const BoArgs a) {
    __shared__ uint32_t s_rows[64 * kBoRowWords];
    __shared__ uint2 s_map[64 * 7];     // [lane][r]
    __shared__ uint2 s_pre[7 * 64];     // [r][lane]
    const int lane = threadIdx.x;
    const uint32_t t = blockIdx.x;
    const BoFrame fr = a.frames[blockIdx.y];
    if (t >= bo_tiles(fr.end)) return;
    bo_stage(s_rows, a.comp, fr, t, lane);
    __syncthreads();

    // ---- the segment's map, backwards: st[j] is the state of a token start at p + 1 + j
    const uint32_t* row = s_rows + lane * kBoRowWords;
    const long long left = (long long)fr.end - ((long long)t * kBoTile + (long long)lane * kBoSeg);   // bytes from the segment's start to the bound
    const int end_rel = (int)(left < -1 ? -1 : left > 1024 ? 1024 : left);
    uint32_t ec[7], sm[7];   // exit | count << 3, delta sum
#pragma unroll
    for (int j = 0; j < 7; ++j) { ec[j] = (uint32_t)j; sm[j] = 0u; }   // (a start at 64 + j enters the next segment at j, with nothing counted)
    unsigned long long win = ((unsigned long long)row[kBoSeg / 4 + 1] << 32) | row[kBoSeg / 4];
    uint32_t word = 0;
    for (int p = kBoSeg - 1; p >= 0; --p) {
        if ((p & 3) == 3) word = row[p >> 2];
        win = (win << 8) | ((word >> (8 * (p & 3))) & 0xFFu);
        uint32_t len, delta;
        bo_token(win, len, delta);
        const bool valid = p + (int)len <= end_rel;
        const uint32_t nec = len == 1u ? ec[0] : len == 3u ? ec[2] : ec[6];
        const uint32_t nsm = len == 1u ? sm[0] : len == 3u ? sm[2] : sm[6];
#pragma unroll
        for (int j = 6; j > 0; --j) { ec[j] = ec[j - 1]; sm[j] = sm[j - 1]; }
        ec[0] = nec + (valid ? 8u : 0u);
        sm[0] = nsm + (valid ? delta : 0u);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) s_map[lane * 7 + j] = make_uint2(ec[j], sm[j]);
    __syncthreads();

    // ---- the tile's map: lane r < 7 enters at offset r and walks the 64 segments
    const uint64_t tile = (uint64_t)fr.tile0 + t;
    if (lane < 7) {
        uint32_t r = (uint32_t)lane, cnt = 0, sum = 0;
        for (int l = 0; l < 64; ++l) {
            s_pre[lane * 64 + l] = make_uint2(r | (cnt << 3), sum);
            const uint2 m = s_map[l * 7 + (int)r];
            r = m.x & 7u;
            cnt += m.x >> 3;
            sum += m.y;
        }
        a.tile_map[tile * 7 + lane] = make_uint2(r | (cnt << 3), sum);
    }
    __syncthreads();
    for (int i = lane; i < 7 * 64; i += 64) a.lane_pre[tile * (7 * 64) + i] = s_pre[i];
}

// One wave per frame.  Bounded by the frame's tile count.
__global__ __launch_bounds__(64) void k_bo_compose(const BoArgs a) {
    __shared__ uint2 s_map[64 * 7];
    __shared__ uint4 s_state[64];
    const int lane = threadIdx.x;
    BoFrame& fr = a.frames[blockIdx.x];
    const uint32_t n_tiles = bo_tiles(fr.end);
    const uint64_t tile0 = fr.tile0;
    uint32_t r = 0, k = 0, v = 0;   // (lane 0's)
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 64) {
        const uint32_t n = n_tiles - t0 < 64u ? n_tiles - t0 : 64u;
        for (uint32_t i = lane; i < n * 7u; i += 64) s_map[i] = a.tile_map[(tile0 + t0) * 7 + i];
        __syncthreads();
        if (lane == 0) {
            for (uint32_t j = 0; j < n; ++j) {
                const uint2 m = s_map[j * 7u + r];
                s_state[j] = make_uint4(r, k, v, m.x >> 3);
                r = m.x & 7u;
                k += m.x >> 3;
                v += m.y;
            }
        }
        __syncthreads();
        if ((uint32_t)lane < n) a.tile_state[tile0 + t0 + lane] = s_state[lane];
        __syncthreads();
    }
    if (lane == 0) {
        fr.total = k;
        if (k < a.W * a.H) atomicOr(a.error, kOvfCorruptByteOffset);
    }
}

template <typename PixelT>
__global__ __launch_bounds__(64) void k_bo_emit(const BoArgs a) {
    __shared__ uint32_t s_rows[64 * kBoRowWords];
    __shared__ PixelT s_val[kBoTile];    // the tile's elements (a token is at least one byte)
    const int lane = threadIdx.x;
    const uint32_t t = blockIdx.x;
    const BoFrame fr = a.frames[blockIdx.y];
    const uint32_t n_px = a.W * a.H;
    uint8_t* img = a.image + (uint64_t)blockIdx.y * a.frame_stride;
    auto put = [&](uint32_t e, PixelT v) {
        const uint32_t y = e / a.W, x = e - y * a.W;
        *reinterpret_cast<PixelT*>(img + (uint64_t)y * a.pitch + (uint64_t)x * sizeof(PixelT)) = v;
    };
    // a chunk that holds too few elements: the missing pixels are zeros (the whole launch shares them out)
    if (fr.total < n_px) {
        const uint32_t step = gridDim.x * 64u;
        for (uint64_t e = (uint64_t)fr.total + t * 64u + lane; e < n_px; e += step) put((uint32_t)e, (PixelT)0);
    }
    if (t >= bo_tiles(fr.end)) return;
    const uint64_t tile = (uint64_t)fr.tile0 + t;
    const uint4 st = a.tile_state[tile];   // (entry offset, first element, value, elements)
    const uint32_t n_el = st.w < (uint32_t)kBoTile ? st.w : (uint32_t)kBoTile;
    if (n_el == 0u || st.y >= n_px) return;   // (nothing starts here, or all of it lies behind the frame)
    bo_stage(s_rows, a.comp, fr, t, lane);
    __syncthreads();

    const uint2 pre = a.lane_pre[tile * (7 * 64) + (st.x < 7u ? st.x : 0u) * 64u + lane];
    const uint32_t* row = s_rows + lane * kBoRowWords;
    const long long left = (long long)fr.end - ((long long)t * kBoTile + (long long)lane * kBoSeg);
    const int end_rel = (int)(left < -1 ? -1 : left > 1024 ? 1024 : left);
    uint32_t pos = pre.x & 7u, i = pre.x >> 3, v = st.z + pre.y;
    while (pos < (uint32_t)kBoSeg) {   // (pos grows by at least one)
        const uint32_t w = pos >> 2, sh = (pos & 3u) * 8u;
        const unsigned long long lo = ((unsigned long long)row[w + 1] << 32) | row[w];
        const unsigned long long win = sh ? (lo >> sh) | ((unsigned long long)row[w + 2] << (64u - sh)) : lo;
        uint32_t len, delta;
        bo_token(win, len, delta);
        if ((int)(pos + len) > end_rel) break;
        v += delta;
        if (i < n_el) s_val[i] = (PixelT)v;
        ++i;
        pos += len;
    }
    __syncthreads();
    for (uint32_t j = lane; j < n_el; j += 64) {
        const uint64_t e = (uint64_t)st.y + j;
        if (e < n_px) put((uint32_t)e, s_val[j]);
    }
}
template __global__ void k_bo_emit<uint16_t>(const BoArgs);
template __global__ void k_bo_emit<uint32_t>(const BoArgs);

}  // namespace ffsamd
