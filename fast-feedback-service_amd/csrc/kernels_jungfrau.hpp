// kernels_jungfrau.hpp (included by ffs_encoded.hip) -- raw Jungfrau words to photon counts on the GPU (FFS_CODEC_JUNGFRAU_RAW, DESIGN.md
// section 5d).  The rule is jungfrau_model.hpp's; the reference has no counterpart (its readers hand over photon counts).
//
// One launch per batch.  The frame is indexed FLAT: a lane owns the eight consecutive pixels 8 i .. 8 i + 7 of the dense chunk, whatever
// the width, so its raw load (16 B per frame, at byte 16 i of a chunk whose base is a multiple of 16) and its twelve calibration loads
// (32 B of each of the six dense planes, at byte 32 i) are aligned at every width.  It loads the 48 calibration values ONCE and then walks
// the batch's frames, the raw loads kJfAhead frames ahead of their use: the planes cost 24 B a pixel per batch, not per frame, and the
// bytes the launch must move are W H (24 + 6 B).
//
// The device copy of the calibration stays six dense planes, as the caller hands them over: consecutive lanes read consecutive 32-byte
// pieces of a plane, so every load instruction is a fully used run of 2 KiB per wave, as it would be interleaved; the setter is six plain
// copies with no reshuffle on the host (9.4 M pixels x 24 B per pedestal update), and a plane lies at the same flat index as the raw words.
//
// What width decides is the STORE: the image is pitched, so a group of eight lies in one row at a 32-byte aligned place only when
// W % 8 == 0 (kRows: two 16-byte stores); at any other width a group may straddle a row end and start anywhere, and its pixels are stored
// one dword at a time, row and column per pixel (the slower path: no detector of this library's workloads has such a width).  The last
// group of a frame may reach past W H: its loads stay inside the planes' and the staged chunks' slack (a multiple of 8 pixels is
// allocated), its stores are dropped.
#pragma once
#include "ffs_device.h"
#include "jungfrau_model.hpp"

namespace ffsamd {

constexpr int kJfLanePixels = 8;     // pixels a lane owns
constexpr int kJfBlock = 256;        // lanes of a workgroup: 2048 pixels
constexpr int kJfAhead = 4;          // frames a lane's raw loads run ahead
constexpr uint32_t kJfMaxFrames = 64;   // chunk bases a launch carries in its arguments (a longer batch takes another launch)

struct JfArgs {
    const uint8_t* comp;         // the staged chunks
    const float* planes;         // pedestal G0, G1, G2, factor G0, G1, G2: six planes, plane_stride floats apart
    uint64_t plane_stride;
    uint8_t* image;              // pitched device frames (32-bit pixels)
    uint64_t frame_stride;
    uint32_t pitch;
    uint32_t W;
    uint32_t n_px;               // W * H
    uint32_t n_frames;
    uint32_t base[kJfMaxFrames]; // where frame f's chunk lies in comp (a multiple of 16)
};

// kRows: W % 8 == 0
template <bool kRows>
__global__ __launch_bounds__(kJfBlock) void k_jungfrau_raw(const JfArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kJfBlock + threadIdx.x;   // the lane's group
    const uint64_t e0 = (uint64_t)i * kJfLanePixels;                    // ... and its first pixel
    if (e0 >= a.n_px) return;
    float cal[6][kJfLanePixels];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const float4* src = reinterpret_cast<const float4*>(a.planes + (uint64_t)p * a.plane_stride + e0);
        const float4 lo = src[0], hi = src[1];
        cal[p][0] = lo.x; cal[p][1] = lo.y; cal[p][2] = lo.z; cal[p][3] = lo.w;
        cal[p][4] = hi.x; cal[p][5] = hi.y; cal[p][6] = hi.z; cal[p][7] = hi.w;
    }
    auto raw_of = [&](uint32_t f) { return *reinterpret_cast<const uint4*>(a.comp + (uint64_t)a.base[f] + e0 * 2u); };
    // where the group's pixels go: one place (kRows), or one per pixel
    const uint32_t y0 = (uint32_t)(e0 / a.W), x0 = (uint32_t)(e0 - (uint64_t)y0 * a.W);
    const uint64_t off0 = (uint64_t)y0 * a.pitch + (uint64_t)x0 * 4u;
    uint4 ring[kJfAhead];
#pragma unroll
    for (int j = 0; j < kJfAhead; ++j)
        if ((uint32_t)j < a.n_frames) ring[j] = raw_of((uint32_t)j);
    for (uint32_t f0 = 0; f0 < a.n_frames; f0 += kJfAhead) {
#pragma unroll
        for (int j = 0; j < kJfAhead; ++j) {
            const uint32_t f = f0 + (uint32_t)j;
            if (f >= a.n_frames) break;
            const uint4 w = ring[j];
            if (f + kJfAhead < a.n_frames) ring[j] = raw_of(f + kJfAhead);
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
            uint32_t out[kJfLanePixels];
#pragma unroll
            for (int k = 0; k < kJfLanePixels; ++k) {
                const uint32_t r = (words[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;   // (little-endian words)
                out[k] = jf_photons(r, cal[0][k], cal[1][k], cal[2][k], cal[3][k], cal[4][k], cal[5][k]);
            }
            uint8_t* img = a.image + (uint64_t)f * a.frame_stride;
            if constexpr (kRows) {
                uint4* dst = reinterpret_cast<uint4*>(img + off0);
                dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
                dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
            } else {
                uint32_t y = y0, x = x0;
#pragma unroll
                for (int k = 0; k < kJfLanePixels; ++k) {
                    if (e0 + (uint64_t)k < a.n_px) *reinterpret_cast<uint32_t*>(img + (uint64_t)y * a.pitch + (uint64_t)x * 4u) = out[k];
                    if (++x == a.W) { x = 0; ++y; }
                }
            }
        }
    }
}

}  // namespace ffsamd
