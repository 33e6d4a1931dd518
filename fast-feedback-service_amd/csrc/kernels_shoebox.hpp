// kernels_shoebox.hpp (included by ffs_shoebox.hip only) -- summation integration of shoeboxes in Kabsch space (ffs_stream_shoebox_fold,
// DESIGN.md section 3.8c).  The rule and every decision are shoebox_model.hpp's; this file is how a wave gets there.
//
// One launch per fold, k_shoebox_fold<PixelT, Algorithm>: a wave per shoebox of the launch's list, kShoeboxWaves of them a workgroup.
//   Constants. The reflection's Kabsch frame (e1, e2, len, zeta) once per wave, every lane the same float64 sequence.
//   Corners.   The box is walked in strips of 63 pixel columns: lane l of a strip owns corner column x0 + l (64 corner columns a strip, the
//              last shared with the next strip's first) and pixel column x0 + l (63 of them).  A corner's xy term does not depend on the
//              image, so a lane computes it ONCE per corner and keeps a rolling pair in registers: the corner row above the pixel row and the
//              one below.  A box of any allowed size takes this one path; there is no oversized fallback.
//   Flags.     Per (pixel row, image): the image's three e3 terms (wave-uniform), the two corner rows' decisions, one __ballot of "either
//              row's corner is foreground", m | m >> 1 -- bit l is then pixel l's OR over its four corners.  No LDS for flags.
//   Pixels.    The mask bit is read once per pixel row, the pixel once per image; fg_sum, fg_count, the three moments, the tail count and the
//              flags are per-lane registers, summed (OR-ed) across the wave at the end.
//   Histogram. 256 dwords of wave-private LDS, one LDS add per counting background pixel below 256, as kernels_spotbg.hpp.
//   Record.    At the end ONE plain read-modify-write of the box's own device record by lane 0 and of the non-zero bins of its histogram,
//              lane l bins 4 l .. 4 l + 3.  A launch's list names a shoebox once and the library serialises the folds of a context into one
//              HIP stream, so exactly one wave at a time owns a shoebox: no global atomics.
// Bounds: a pixel or a mask byte is read only when 0 <= x < W, 0 <= y < H and the frame lies in the batch; the list's entries are table
// indices the host built (shoebox_plan.hpp), below the table's length.
#pragma once
#include "ffs_device.h"
#include "shoebox_model.hpp"

namespace ffsamd {

constexpr int kShoeboxWaves = 4;                  // shoeboxes per workgroup (1 KB of LDS each)
constexpr int kShoeboxThreads = 64 * kShoeboxWaves;
constexpr int kShoeboxStrip = 63;                 // pixel columns a strip of 64 corner columns covers

struct ShoeboxArgs {
    const void* image;          // [frame][y][pitch bytes], where the batch left its frames
    uint64_t frame_stride;
    uint32_t pitch;
    const uint8_t* maskbits;    // the context's valid-pixel bit plane, rows of mpitch bytes
    uint32_t mpitch;
    int W, H;
    uint32_t limit;             // a pixel counts when p < limit
    uint32_t n_frames;          // frames of the batch; frame f is image first_image + f
    int64_t first_image;
    uint32_t n_list;
    const uint32_t* list;       // [n_list] table indices, each once
    const ShoeboxEntry* boxes;  // the table
    ShoeboxAcc* acc;            // [table] accumulators
    uint32_t* hist;             // [table][kSpotBgBins]
    double ib, im;              // 1 / delta_b^2, 1 / delta_m^2
    ShoeboxGeometry geom;
};

__device__ __forceinline__ uint32_t shoebox_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t shoebox_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <typename PixelT, int Algorithm>
__global__ __launch_bounds__(kShoeboxThreads) void k_shoebox_fold(ShoeboxArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t shoebox_hist[kShoeboxWaves][kSpotBgBins];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* hist = shoebox_hist[wave];
    const uint32_t k = blockIdx.x * (uint32_t)kShoeboxWaves + wave;
    const bool live = k < a.n_list;   // (the same in every lane of a wave; the two barriers below are reached by every wave)
    *reinterpret_cast<uint4*>(hist + 4u * lane) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    uint64_t fg_sum = 0ull, m_x = 0ull, m_y = 0ull, m_z = 0ull;
    uint32_t fg_count = 0u, n_tail = 0u, flags = 0u, r = 0u;
    if (live) {
        r = a.list[k];
        const ShoeboxEntry b = a.boxes[r];
        const ShoeboxFrame f = shoebox_frame(a.geom, b.s1, b.phi);
        const int64_t n_lo = max((int64_t)b.z_min, a.first_image), n_hi = min((int64_t)b.z_max, a.first_image + (int64_t)a.n_frames);
        for (int32_t x0 = b.x_min; x0 < b.x_max; x0 += kShoeboxStrip) {
            const int32_t cx = x0 + (int32_t)lane;   // this lane's corner column and pixel column
            const bool corner_live = cx <= b.x_max, pixel_live = lane < (uint32_t)kShoeboxStrip && cx < b.x_max;
            const bool in_x = pixel_live && cx >= 0 && cx < a.W;
            double xy_above = corner_live ? shoebox_corner_xy(a.geom, f, cx, b.y_min, a.ib) : 0.0;
            for (int32_t py = b.y_min; py < b.y_max; ++py) {
                const double xy_below = corner_live ? shoebox_corner_xy(a.geom, f, cx, py + 1, a.ib) : 0.0;
                const bool in_image = in_x && py >= 0 && py < a.H;
                bool valid = false;
                if (in_image) valid = (((uint32_t)a.maskbits[(uint64_t)py * a.mpitch + (uint32_t)(cx >> 3)] >> (cx & 7)) & 1u) != 0u;
                for (int64_t n = n_lo; n < n_hi; ++n) {
                    const ShoeboxImage img = shoebox_image(a.geom, f, n, a.im);
                    const bool c = corner_live && (shoebox_corner_foreground(Algorithm, xy_above, img) || shoebox_corner_foreground(Algorithm, xy_below, img));
                    uint64_t m = __ballot(c);
                    m |= m >> 1;
                    const bool fg = pixel_live && ((m >> lane) & 1ull) != 0ull;
                    uint32_t p = 0u;
                    bool counts = false;
                    if (valid) {
                        const uint8_t* frame = static_cast<const uint8_t*>(a.image) + (uint64_t)(n - a.first_image) * a.frame_stride;
                        p = *reinterpret_cast<const PixelT*>(frame + (uint64_t)py * a.pitch + (uint64_t)cx * sizeof(PixelT));
                        counts = p < a.limit;
                    }
                    if (fg && counts) {
                        fg_sum += p, fg_count += 1u;
                        m_x += (uint64_t)p * (uint64_t)(2 * cx + 1), m_y += (uint64_t)p * (uint64_t)(2 * py + 1), m_z += (uint64_t)p * (uint64_t)(2 * n + 1);
                    } else if (fg) {
                        flags |= kShoeboxFgInvalid;
                    } else if (counts) {
                        if (p < (uint32_t)kSpotBgBins) atomicAdd(&hist[p], 1u);
                        else ++n_tail;
                    }
                }
                xy_above = xy_below;
            }
        }
    }
    __syncthreads();
    if (!live) return;

    fg_sum = shoebox_wave_sum(fg_sum), m_x = shoebox_wave_sum(m_x), m_y = shoebox_wave_sum(m_y), m_z = shoebox_wave_sum(m_z);
    fg_count = shoebox_wave_sum(fg_count), n_tail = shoebox_wave_sum(n_tail);
    flags = __ballot(flags != 0u) != 0ull ? kShoeboxFgInvalid : 0u;
    if (lane == 0u) {
        ShoeboxAcc o = a.acc[r];
        o.fg_sum += fg_sum, o.m_x += m_x, o.m_y += m_y, o.m_z += m_z;
        o.fg_count += fg_count, o.n_overflow += n_tail, o.flags |= flags;
        a.acc[r] = o;
    }
    const uint4 h = *reinterpret_cast<const uint4*>(hist + 4u * lane);
    uint32_t* g = a.hist + (uint64_t)r * (uint32_t)kSpotBgBins + 4u * lane;
    if (h.x) g[0] += h.x;
    if (h.y) g[1] += h.y;
    if (h.z) g[2] += h.z;
    if (h.w) g[3] += h.w;
}

}  // namespace ffsamd
