// kernels_pixstats.hpp (included by ffs_products.hip only) -- the per-pixel statistics over a run (ffs_ctx_set_pixel_stats, DESIGN.md
// section 3.7): per pixel, in how many frames it counted, the sum and the sum of squares of its values there, and the largest of them --
// what a mask, a gain map and a "virtual powder pattern" are made from.  A pixel value counts when p < limit (launch_geometry.hpp,
// counting_limit: the radial profile's rule); the valid-pixel mask plays no part.  The reference has no counterpart.
//
// One launch a batch, no atomics: a lane owns 16 B of one pixel row -- PX = 8 or 4 pixels -- and walks the batch's frames at that
// position, kPixStatsUnroll independent loads in flight, with count, sum, sum of squares and maximum of its PX pixels in registers; then
// it adds them into the context's accumulators with ONE read-modify-write.  The accumulator traffic is per batch, not per frame.  Two
// launches on the same accumulators must not overlap: the host serialises them (ffs_products.hip, launch_pixel_stats).
//
// The accumulators are laid out for that read-modify-write, not for the caller (ffs_ctx_get_pixel_stats un-interleaves them,
// pixstats_entry in ffs_internal.hpp is the host's statement of where an entry lies): lanes are numbered row by row, i = y * groups + x / PX, and
// sixty-four consecutive lanes -- a wave -- form a tile.  A lane's PX entries of a plane are PX * sizeof(entry) / 16 chunks of 16 B; chunk k
// of lane l of tile t lies at 16 B x ((t * chunks + k) * 64 + l): every 16-byte access of a wave is one contiguous kilobyte.  A lane
// that straddles W stays inside the pixel row (rows hold pitch_px >= W pixels, a multiple of 128) and its entries beyond W exist, hold
// whatever the row padding gave, and are never handed out.
//
// 16-bit pixels: the sum within a batch is a 32-bit register -- exact up to kPixStatsMaxFrames = 65 536 frames (65 536 x 65 535 < 2^32);
// the host splits a longer batch into launches of at most that many.  In memory every sum is 64 bits.  p * p of a 16-bit pixel fits 32
// bits and is widened as it is added.  32-bit pixels count below 2^24 only: p * p < 2^48, one 32 x 32 -> 64 bit multiply-add.
#pragma once
#include <type_traits>

#include "ffs_device.h"

namespace ffsamd {

constexpr int kPixStatsThreads = 256;
constexpr int kPixStatsUnroll = 4;                  // frames whose loads a lane has in flight
constexpr uint32_t kPixStatsMaxFrames = 1u << 16;   // frames of one launch: what the 32-bit sums of the 16-bit kernel hold

struct PixStatsArgs {
    const void* image;          // [frame][y][pitch bytes], as the threshold stage reads it
    uint64_t frame_stride;
    uint32_t pitch;
    uint32_t groups;            // lanes of a row: ceil(W / PX)
    uint32_t n_lanes;           // groups * H
    uint32_t n_frames;          // <= kPixStatsMaxFrames
    uint32_t limit;             // a pixel value counts when p < limit
    uint4 *count, *max, *sum, *sum_sq;   // the four planes, in tiles (above)
};

template <typename PixelT>
struct PixStatsRegs {
    static constexpr int PX = 16 / (int)sizeof(PixelT);
    using SumT = typename std::conditional<sizeof(PixelT) == 2, uint32_t, uint64_t>::type;
    uint32_t cnt[PX], mx[PX];
    SumT sm[PX];
    uint64_t sq[PX];
};

template <typename PixelT>
__device__ __forceinline__ void pixstats_fold(PixStatsRegs<PixelT>& r, const uint4 v, uint32_t limit) {
    constexpr int PX = PixStatsRegs<PixelT>::PX;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const uint32_t p = lane_pixel<PX>(v, j);
        const bool ok = p < limit;
        const uint32_t q = ok ? p : 0u;
        r.cnt[j] += ok ? 1u : 0u;
        r.sm[j] += q;
        if constexpr (PX == 8) r.sq[j] += (uint64_t)(q * q);   // (65535^2 < 2^32)
        else r.sq[j] += (uint64_t)q * q;
        r.mx[j] = max(r.mx[j], q);
    }
}

template <typename PixelT>
__global__ __launch_bounds__(kPixStatsThreads) void k_pixel_stats(PixStatsArgs a) {
    constexpr int PX = PixStatsRegs<PixelT>::PX;
    const uint32_t i = blockIdx.x * (uint32_t)kPixStatsThreads + threadIdx.x;
    if (i >= a.n_lanes) return;
    const uint32_t y = i / a.groups, g = i - y * a.groups;
    const uint8_t* at = static_cast<const uint8_t*>(a.image) + (uint64_t)y * a.pitch + (uint64_t)g * 16u;
    PixStatsRegs<PixelT> r;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        r.cnt[j] = 0u;
        r.mx[j] = 0u;
        r.sm[j] = 0;
        r.sq[j] = 0ull;
    }
    uint32_t f = 0;
    for (; f + kPixStatsUnroll <= a.n_frames; f += kPixStatsUnroll) {
        uint4 v[kPixStatsUnroll];
#pragma unroll
        for (int u = 0; u < kPixStatsUnroll; ++u) v[u] = *reinterpret_cast<const uint4*>(at + (uint64_t)(f + u) * a.frame_stride);
#pragma unroll
        for (int u = 0; u < kPixStatsUnroll; ++u) pixstats_fold<PixelT>(r, v[u], a.limit);
    }
    for (; f < a.n_frames; ++f) pixstats_fold<PixelT>(r, *reinterpret_cast<const uint4*>(at + (uint64_t)f * a.frame_stride), a.limit);

    // the one read-modify-write: chunk k of this lane's entries in each plane (every load is issued before the first store)
    constexpr int C32 = PX / 4, C64 = PX / 2;
    const uint64_t tile = i >> 6, lane = i & 63u;
    uint4* pc = a.count + tile * C32 * 64u + lane;
    uint4* pm = a.max + tile * C32 * 64u + lane;
    uint4* ps = a.sum + tile * C64 * 64u + lane;
    uint4* pq = a.sum_sq + tile * C64 * 64u + lane;
    uint4 c[C32], m[C32], s[C64], q[C64];
#pragma unroll
    for (int k = 0; k < C32; ++k) {
        c[k] = pc[k * 64];
        m[k] = pm[k * 64];
    }
#pragma unroll
    for (int k = 0; k < C64; ++k) {
        s[k] = ps[k * 64];
        q[k] = pq[k * 64];
    }
#pragma unroll
    for (int k = 0; k < C32; ++k) {
        c[k].x += r.cnt[4 * k];
        c[k].y += r.cnt[4 * k + 1];
        c[k].z += r.cnt[4 * k + 2];
        c[k].w += r.cnt[4 * k + 3];
        m[k].x = max(m[k].x, r.mx[4 * k]);
        m[k].y = max(m[k].y, r.mx[4 * k + 1]);
        m[k].z = max(m[k].z, r.mx[4 * k + 2]);
        m[k].w = max(m[k].w, r.mx[4 * k + 3]);
        pc[k * 64] = c[k];
        pm[k * 64] = m[k];
    }
#pragma unroll
    for (int k = 0; k < C64; ++k) {
        const uint64_t s0 = (((uint64_t)s[k].y << 32) | s[k].x) + (uint64_t)r.sm[2 * k], s1 = (((uint64_t)s[k].w << 32) | s[k].z) + (uint64_t)r.sm[2 * k + 1];
        const uint64_t q0 = (((uint64_t)q[k].y << 32) | q[k].x) + r.sq[2 * k], q1 = (((uint64_t)q[k].w << 32) | q[k].z) + r.sq[2 * k + 1];
        ps[k * 64] = make_uint4((uint32_t)s0, (uint32_t)(s0 >> 32), (uint32_t)s1, (uint32_t)(s1 >> 32));
        pq[k * 64] = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
    }
}

}  // namespace ffsamd
