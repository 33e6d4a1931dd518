// kernels_jfped.hpp (included by ffs_encoded.hip) -- dark frames of raw Jungfrau words folded into per-pixel, per-stage accumulators
// (ffs_stream_jungfrau_pedestal_fold).  The rule is jungfrau_pedestal_model.hpp's; the reference has no counterpart.
//
// One launch per batch of up to kJfPedMaxLaunch staged chunks, whose bases travel in the kernel arguments, in the style of k_jungfrau_raw.
// The frame is indexed FLAT: a lane owns the eight consecutive pixels 8 i .. 8 i + 7 of the dense chunk, whatever the width, so its raw load
// (16 B per frame, at byte 16 i of a chunk whose base is a multiple of 16) is aligned at every width.  It walks the batch's frames with the
// raw loads kJfPedAhead frames ahead of their use and keeps count, sum and sum of squares of its eight pixels for the three stages in
// registers; then it adds them into the context's accumulators with ONE read-modify-write per launch, no atomics.  Two launches on the same
// accumulators must not overlap: the host puts them into one HIP stream of the context (ffs_encoded.hip, the fold).
//
// A stage in which none of the lane's eight pixels counted during the launch is neither loaded nor stored.  A dark run is uniform in
// stage, so a launch then moves 20 B read + 20 B written per pixel (4 + 8 + 8) instead of 60 + 60: the bytes a launch must move are
// W H (2 frames + 40 per stage present).
//
// EXACT INSIDE A LAUNCH, for any content, in 64-bit registers where 32 bits would not do.  With at most 64 frames a launch and a < 2^14:
//   count  <= 64: the three stages' counts of a pixel share ONE 32-bit register, a byte each (64 < 256);
//   sum    <= 64 x 16383 < 2^20: a 32-bit register per pixel and stage;
//   sum_sq <= 64 x 16383^2 = 1.7e10 > 2^32: a 64-bit register per pixel and stage (a * a < 2^28 is one 32-bit multiply, widened as it is
//          added).  The walk is not split.
// 8 + 24 + 48 accumulator registers and the ring of 16.
//
// THE ACCUMULATORS ARE DENSE PLANES, as the caller reads them: count[3] (uint32), sum[3], sum_sq[3] (uint64), each plane_stride entries
// (W H rounded up to 8) apart, entry k of a plane is flat pixel k.  A lane's eight entries of a plane are 32 or 64 consecutive bytes, 16-byte
// aligned, and consecutive lanes hold consecutive pieces: the two (four) 16-byte accesses of a wave to a plane cover one contiguous run of
// 2 KiB (4 KiB) between them, every cache line used whole, which is what the tiles of kernels_pixstats.hpp buy; and
// ffs_ctx_get_jungfrau_pedestal is nine plain copies with no un-interleaving of 566 MB on the host (Jungfrau-9M), the index of an entry is
// the index of its raw word and of its calibration entry.  The tiles exist in kernels_pixstats.hpp because its lanes walk a PITCHED image row
// by row; here the frame is flat and dense already.
//
// The last group of a frame may reach past W H: its raw loads stay inside the staging area's slack (64 bytes behind the last chunk), its
// accumulator entries beyond W H exist (plane_stride), hold whatever lay behind the chunk, and are never handed out.
#pragma once
#include "ffs_device.h"
#include "jungfrau_pedestal_model.hpp"

namespace ffsamd {

constexpr int kJfPedLanePixels = 8;         // pixels a lane owns
constexpr int kJfPedBlock = 256;            // lanes of a workgroup: 2048 pixels
constexpr int kJfPedAhead = 4;              // frames a lane's raw loads run ahead
constexpr uint32_t kJfPedMaxLaunch = 64;    // frames of one launch: chunk bases in its arguments, a count in a byte (a longer batch takes another launch)

struct JfPedArgs {
    const uint8_t* comp;      // the staged chunks
    uint32_t* count;          // three planes, plane_stride entries apart
    uint64_t* sum;            // likewise
    uint64_t* sum_sq;
    uint64_t plane_stride;    // W * H rounded up to 8
    uint32_t n_px;            // W * H
    uint32_t n_frames;        // <= kJfPedMaxLaunch
    uint32_t base[kJfPedMaxLaunch];   // where frame f's chunk lies in comp (a multiple of 16)
};

__device__ __forceinline__ uint64_t jfped_u64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

__global__ __launch_bounds__(kJfPedBlock) void k_jungfrau_pedestal_fold(const JfPedArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kJfPedBlock + threadIdx.x;   // the lane's group
    const uint64_t e0 = (uint64_t)i * kJfPedLanePixels;                    // ... and its first pixel
    if (e0 >= a.n_px) return;
    uint32_t cw[kJfPedLanePixels];          // the three counts of a pixel, a byte each
    uint32_t sm[3][kJfPedLanePixels];
    uint64_t sq[3][kJfPedLanePixels];
#pragma unroll
    for (int k = 0; k < kJfPedLanePixels; ++k) {
        cw[k] = 0u;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            sm[s][k] = 0u;
            sq[s][k] = 0ull;
        }
    }
    auto raw_of = [&](uint32_t f) { return *reinterpret_cast<const uint4*>(a.comp + (uint64_t)a.base[f] + e0 * 2u); };
    uint4 ring[kJfPedAhead];
#pragma unroll
    for (int j = 0; j < kJfPedAhead; ++j)
        if ((uint32_t)j < a.n_frames) ring[j] = raw_of((uint32_t)j);
    for (uint32_t f0 = 0; f0 < a.n_frames; f0 += kJfPedAhead) {
#pragma unroll
        for (int j = 0; j < kJfPedAhead; ++j) {
            const uint32_t f = f0 + (uint32_t)j;
            if (f >= a.n_frames) break;
            const uint4 w = ring[j];
            if (f + kJfPedAhead < a.n_frames) ring[j] = raw_of(f + kJfPedAhead);
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < kJfPedLanePixels; ++k) {
                const uint32_t r = (words[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;   // (little-endian words)
                const bool counts = !jf_word_invalid(r);
                const uint32_t s = jf_stage(r);
                const uint32_t adc = counts ? jf_pedestal_adc(r) : 0u;
                const uint32_t adc2 = adc * adc;   // (< 2^28)
                cw[k] += counts ? (1u << (8u * s)) : 0u;
#pragma unroll
                for (uint32_t t = 0; t < 3; ++t) {
                    sm[t][k] += s == t ? adc : 0u;
                    sq[t][k] += (uint64_t)(s == t ? adc2 : 0u);
                }
            }
        }
    }
    // the one read-modify-write, a stage at a time and only the stages in which one of the eight pixels counted
    uint32_t any = 0u;
#pragma unroll
    for (int k = 0; k < kJfPedLanePixels; ++k) any |= cw[k];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (((any >> (8 * s)) & 0xFFu) == 0u) continue;
        uint4* pc = reinterpret_cast<uint4*>(a.count + (uint64_t)s * a.plane_stride + e0);
        uint4* ps = reinterpret_cast<uint4*>(a.sum + (uint64_t)s * a.plane_stride + e0);
        uint4* pq = reinterpret_cast<uint4*>(a.sum_sq + (uint64_t)s * a.plane_stride + e0);
        uint4 c[2], m[4], q[4];   // (every load is issued before the first store)
#pragma unroll
        for (int k = 0; k < 2; ++k) c[k] = pc[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[k] = ps[k];
            q[k] = pq[k];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            c[k].x += (cw[4 * k] >> (8 * s)) & 0xFFu;
            c[k].y += (cw[4 * k + 1] >> (8 * s)) & 0xFFu;
            c[k].z += (cw[4 * k + 2] >> (8 * s)) & 0xFFu;
            c[k].w += (cw[4 * k + 3] >> (8 * s)) & 0xFFu;
            pc[k] = c[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t m0 = jfped_u64(m[k].x, m[k].y) + (uint64_t)sm[s][2 * k], m1 = jfped_u64(m[k].z, m[k].w) + (uint64_t)sm[s][2 * k + 1];
            const uint64_t q0 = jfped_u64(q[k].x, q[k].y) + sq[s][2 * k], q1 = jfped_u64(q[k].z, q[k].w) + sq[s][2 * k + 1];
            ps[k] = make_uint4((uint32_t)m0, (uint32_t)(m0 >> 32), (uint32_t)m1, (uint32_t)(m1 >> 32));
            pq[k] = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
        }
    }
}

}  // namespace ffsamd
