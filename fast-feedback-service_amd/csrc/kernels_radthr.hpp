// kernels_radthr.hpp (included by ffs_products.hip only) -- the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE): a
// pixel is strong when it stands above median + n_iqr x IQR of its shell of the caller's bin map (ffs_ctx_set_radial_bins, at most 128
// bins), both taken per frame over a histogram of the shell's counting pixels.  The reference has no counterpart (its algorithms are
// dispersion and dispersion_extended, spotfinder/spotfinder.cc:338-342); the definition is ffs_hip.h's, modelled on DIALS's radial_profile.
//
// Three launches in the dense stream, everything an integer but the cutoff's one product:
//   k_radthr_hist<PixelT>   grid (frames, bands): a workgroup of sixteen waves streams a band of contiguous rows of one frame with
//                           kernels_radial.hpp's band walk (16 B of pixels, the matching bin entries and mask bits per lane and load, the
//                           next load in flight) and counts into a table in LDS, n_bins x 257 counters: the values 0 .. 255 and a tail.  The
//                           table is up to 128.5 KiB -- one workgroup a CU, hence sixteen waves of it -- and its non-zero counters are then
//                           added to the frame's table in global memory, zeroed ahead of the launch (integers: any order, the same bits).
//   k_radthr_cut            grid (bins, frames): a wave per (frame, shell) scans the 257 counters, four bins a lane, and decides with
//                           radial_threshold_model.hpp: N, the quartiles, the status, the cutoff.  The record goes to pinned host memory,
//                           the cutoff (0xFFFFFFFF under a status other than 0: no pixel passes) to the device array k_radthr_strong reads.
//   k_radthr_strong<PixelT> grid (strips x tiles, frames): a wave per 64 eight-pixel groups and eight rows (an exact-stage tile) decides
//                           every pixel -- p > cutoff of its shell, an integer compare, and p > threshold -- and leaves what k_window leaves
//                           for the sparse stage: the non-zero bytes of a plane that is zero at launch, the occupancy bits, the per-tile
//                           counts, the byte mask when asked for.
// How a lane's count meets the table (tuning "radthr_form"): 1, one LDS add per counting pixel under the lane's own exec bit; 2, a run of
// equal (shell, value) pairs kept in registers, as k_radial keeps its run of equal bins, and added when the pair changes; 0 (default), the
// one that measured faster for the pixel size -- the run for 16-bit pixels (0.454 against 0.476 ms, 32 Eiger-16M frames, 100 shells), the
// plain add for 32-bit (0.297 against 0.324 ms, Jungfrau-9M).  DESIGN.md section 3.9 has both.
//
// With a blur (ffs_ctx_set_radial_blur narrow | wide) the first and the third launch take their blurred forms, at the
// end of this file, and decide on v = floor(S / Wn) of radial_blur_model.hpp in place of p; k_radthr_cut is the same.  Both recompute the
// blur from the frame (no blurred frame is stored):
//   k_radthr_hist_blur<PixelT, R>    the same grid, workgroup and table; a wave takes units of a band -- a run of up to 32 contiguous rows of
//                                    a strip of 62 eight-pixel groups -- instead of every sixteenth row, with blur_walk below.
//   k_radthr_strong_blur<PixelT, R>  grid (strips x runs, frames): a wave per such unit (four tiles), the tile count added every eight rows;
//                                    a strong pixel also has p >= 1.
//   blur_walk                        a ring of 2R + 1 rows of the lane's group (p x tap and the tap bits) in registers; per row the vertical
//                                    pass, the R edge columns of either neighbour from the lanes beside (lanes 0 and 63 carry the neighbouring
//                                    strips' groups and own no output), the horizontal pass, a shift where every tap is there and the
//                                    division by the weight of the taps that are, under a branch, where not.
#pragma once
#include "ffs_device.h"
#include "kernels_radial.hpp"
#include "radial_blur_model.hpp"
#include "radial_threshold_model.hpp"

namespace ffsamd {

constexpr int kRadThrHistThreads = 1024;
constexpr int kRadThrHistWaves = kRadThrHistThreads / 64;

struct RadThrArgs {
    RadialIn in;                  // what the histogram's band walk reads (bins8 is null); k_radthr_strong reads the same frames, map and limit
    uint32_t* hist;               // [frame][n_bins][kRadThrCounters], zero when k_radthr_hist starts
    uint32_t* cut;                // [frame][n_bins]: the cutoff, kRadThrNever under a status other than 0
    ffs_radial_shell* shells;     // [frame][n_bins], pinned host memory
    double n_iqr, threshold;
    // what k_radthr_strong writes (ThresholdArgs has the same names)
    uint8_t* bits;
    uint8_t* strong_bytes;
    uint32_t* tile_counts;
    uint32_t* occ;                // nullptr: nobody reads the occupancy bitmap
    uint32_t occ_frame_words, occ_spr;
    uint32_t bpitch;
    uint64_t plane_frame_stride, bytes_frame_stride;
    int n_tiles, dense_mask;
    uint32_t s_strips;            // strips of 64 groups in a row
};

static inline size_t radthr_lds_bytes(uint32_t n_bins) { return (size_t)n_bins * kRadThrCounters * 4u; }

template <typename PixelT, bool RUN>
__global__ __launch_bounds__(kRadThrHistThreads) void k_radthr_hist(RadThrArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t radthr_smem[];
    uint32_t* tab = reinterpret_cast<uint32_t*>(radthr_smem);
    const uint32_t n_tab = a.in.n_bins * (uint32_t)kRadThrCounters;
    const uint32_t frame = blockIdx.x, band = blockIdx.y;
    for (uint32_t i = threadIdx.x; i < n_tab; i += kRadThrHistThreads) tab[i] = 0u;
    __syncthreads();

    // (RUN) the lane's run: a counter's index (x) and how often (y)
    const uint2 last = radial_walk<PixelT, false, kRadThrHistWaves>(a.in, frame, band, make_uint2(0u, 0u), [&a, tab](uint2 run, uint32_t p, uint32_t b, uint32_t m) {
        // (the map's entries are below n_bins or kRadialNone: ffs_ctx_set_radial_bins checked them)
        const bool ok = radial_counts(a.in, m, b, p);
        const uint32_t at = b * (uint32_t)kRadThrCounters + min(p, (uint32_t)kRadThrValues);
        if constexpr (RUN) {
            if (ok && at != run.x) {
                if (run.y != 0u) atomicAdd(&tab[run.x], run.y);
                run.x = at;
                run.y = 0u;
            }
            if (ok) ++run.y;
        } else {
            if (ok) atomicAdd(&tab[at], 1u);
        }
        return run;
    });
    if constexpr (RUN) {
        if (last.y != 0u) atomicAdd(&tab[last.x], last.y);
    }
    __syncthreads();
    uint32_t* out = a.hist + (uint64_t)frame * n_tab;
    for (uint32_t i = threadIdx.x; i < n_tab; i += kRadThrHistThreads) {
        const uint32_t v = tab[i];
        if (v != 0u) atomicAdd(&out[i], v);
    }
}

__device__ __forceinline__ int radthr_wave_max(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(64) void k_radthr_cut(RadThrArgs a) {
    const uint32_t b = blockIdx.x, frame = blockIdx.y, lane = threadIdx.x;
    const uint64_t shell = (uint64_t)frame * a.in.n_bins + b;
    const uint32_t* h = a.hist + shell * (uint32_t)kRadThrCounters;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = h[lane * 4u + (uint32_t)k];
    const uint32_t n_overflow = h[kRadThrValues];
    const uint32_t mine = c[0] + c[1] + c[2] + c[3];
    const uint32_t incl = wave_inclusive_scan(mine);
    const uint64_t n = (uint64_t)__builtin_amdgcn_readlane((int)incl, 63) + n_overflow;   // (at most W x H: a frame's pixels are counted in 32 bits)
    const uint32_t status = radthr_status_of_counts(n, n_overflow);
    int q1 = -1, median = -1, q3 = -1;
    uint32_t cutoff = 0u;
    if (status == kRadThrOk) {   // (the same in every lane)
        const SpotBgPositions pos = spotbg_positions(n);
        uint64_t cum = incl - mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // the first value whose cumulative count reaches a position: exactly one (lane, k) each
            const uint64_t before = cum;
            cum += c[k];
            const int v = (int)(lane * 4u) + k;
            if (before < pos.p25 && cum >= pos.p25) q1 = v;
            if (before < pos.p50 && cum >= pos.p50) median = v;
            if (before < pos.p75 && cum >= pos.p75) q3 = v;
        }
        q1 = radthr_wave_max(q1);
        median = radthr_wave_max(median);
        q3 = radthr_wave_max(q3);
        cutoff = radthr_cutoff(median, q3 - q1, a.n_iqr);
    }
    if (lane == 0u) {
        ffs_radial_shell r;
        r.n_pixels = (uint32_t)n;
        r.n_overflow = n_overflow;
        r.q1 = q1;
        r.median = median;
        r.q3 = q3;
        r.cutoff = cutoff;
        r.status = status;
        r.reserved = 0u;
        a.shells[shell] = r;
        a.cut[shell] = status == kRadThrOk ? cutoff : kRadThrNever;
    }
}

// One row of a lane's group of eight pixels: the pixels, their bin entries and the valid-pixel mask byte; nothing outside the frame
template <typename PixelT>
struct RadThrRow {
    uint4 p0, p1, bn;
    uint32_t mb;
};
template <typename PixelT>
__device__ __forceinline__ RadThrRow<PixelT> radthr_row(const RadThrArgs& a, const uint8_t* img, int y, uint32_t g, bool own) {
    RadThrRow<PixelT> r;
    r.p0 = make_uint4(0u, 0u, 0u, 0u);
    r.p1 = r.p0;
    r.bn = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    r.mb = 0u;
    // (a group that straddles W stays inside the row's pitch_px pixels; what it reads beyond W has no mask bit and no bin)
    if (own && y < a.in.H) {
        const uint8_t* rp = img + (uint64_t)y * a.in.pitch + (uint64_t)g * (8u * sizeof(PixelT));
        r.p0 = *reinterpret_cast<const uint4*>(rp);
        if constexpr (sizeof(PixelT) == 4) r.p1 = *reinterpret_cast<const uint4*>(rp + 16);
        r.bn = *reinterpret_cast<const uint4*>(a.in.bins + (uint64_t)y * a.in.bin_pitch + (uint64_t)g * 8u);
        r.mb = a.in.maskbits[(uint64_t)y * a.in.mpitch + g];
    }
    return r;
}

template <typename PixelT>
__global__ __launch_bounds__(64) void k_radthr_strong(RadThrArgs a) {
    __shared__ uint32_t s_cut[kRadThrMaxBins];
    const uint32_t lane = threadIdx.x;
    const uint32_t strip = blockIdx.x % a.s_strips, tile = blockIdx.x / a.s_strips, frame = blockIdx.y;
    for (uint32_t i = lane; i < kRadThrMaxBins; i += 64u) s_cut[i] = i < a.in.n_bins ? a.cut[(uint64_t)frame * a.in.n_bins + i] : kRadThrNever;
    __syncthreads();
    const uint32_t g = strip * 64u + lane;              // this lane's group: pixels 8g .. 8g + 7
    const bool own = (int)(g * 8u) < a.in.W;
    const int y0 = (int)tile * kTileRows, y1 = min(a.in.H, y0 + kTileRows);
    const uint8_t* img = static_cast<const uint8_t*>(a.in.image) + (uint64_t)frame * a.in.frame_stride;
    uint8_t* plane = a.bits + (uint64_t)frame * a.plane_frame_stride;
    uint8_t* sbytes = a.strong_bytes + (uint64_t)frame * a.bytes_frame_stride;
    uint32_t cnt = 0u;
    RadThrRow<PixelT> row = radthr_row<PixelT>(a, img, y0, g, own);
    for (int y = y0; y < y1; ++y) {
        const RadThrRow<PixelT> next = radthr_row<PixelT>(a, img, y + 1 < y1 ? y + 1 : a.in.H, g, own);
        uint32_t sb = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t b = radial_bin_entry(row.bn, j);
            const uint32_t p = sizeof(PixelT) == 2 ? lane_pixel<8>(row.p0, j) : lane_pixel<4>(j < 4 ? row.p0 : row.p1, j & 3);
            // (a pixel beyond W has no mask bit: bits at x >= W are never set)
            const bool counts = ((row.mb >> j) & 1u) && b != kRadialNone && p < a.in.limit;   // (radial_counts, spelt out: through the helper the kernel compiles differently)
            const uint32_t cutoff = s_cut[b & (kRadThrMaxBins - 1u)];
            if (counts && p > cutoff && (double)p > a.threshold) sb |= 1u << j;
        }
        if (sb) {
            plane[(uint64_t)y * a.in.mpitch + g] = (uint8_t)sb;   // (the plane is all zero when the kernel starts)
            if (a.occ) {
                const uint32_t ob = (uint32_t)y * a.occ_spr + (g >> 4);   // the 16-byte segment of the plane row
                atomicOr(a.occ + (uint64_t)frame * a.occ_frame_words + (ob >> 5), 1u << (ob & 31u));
            }
        }
        if (a.dense_mask && own) {
            uint2 bytes;
            bytes.x = (sb & 1u) | ((sb & 2u) << 7) | ((sb & 4u) << 14) | ((sb & 8u) << 21);
            bytes.y = ((sb >> 4) & 1u) | ((sb & 0x20u) << 3) | ((sb & 0x40u) << 10) | ((sb & 0x80u) << 17);
            *reinterpret_cast<uint2*>(sbytes + (uint64_t)y * a.bpitch + (uint64_t)g * 8u) = bytes;
        }
        cnt += (uint32_t)__popc(sb);
        row = next;
    }
    if (__ballot(cnt != 0u)) {   // the tile's count
        const uint32_t total = __builtin_amdgcn_readlane(wave_inclusive_scan(cnt), 63);
        if (lane == 0u) atomicAdd(a.tile_counts + (uint64_t)frame * a.n_tiles + tile, total);
    }
}

// ---- the blurred forms (ffs_ctx_set_radial_blur) ---------------------------------------------------------------
// A wave walks a run of contiguous rows of one strip.  Lanes 1 .. 62 own a group of eight pixels each; lanes 0 and 63 carry the last group
// of the strip to the left and the first of the strip to the right and own no output, so every owning lane finds its horizontal neighbours
// in the lanes beside it.  A run re-reads R rows above and below itself; rows outside the frame and groups outside the row are never read.
constexpr int kRadBlurOwners = 62;      // groups a wave owns
constexpr int kRadBlurRunRows = 32;     // rows of a wave's run (a multiple of kTileRows): 2R / 32 of the rows are read twice
__device__ __forceinline__ uint32_t radblur_strips(int W) { return ((uint32_t)(W + 7) / 8u + (uint32_t)kRadBlurOwners - 1u) / (uint32_t)kRadBlurOwners; }

// A row of a lane's group as it was loaded ...
template <typename PixelT>
struct BlurRaw {
    uint4 p0, p1;
    uint32_t mb;
};
// ... and as the stencil keeps it: p x tap, packed as the frame has the pixels, and the tap bits of the group with the R nearest of either
// neighbour (bit i: the pixel at x = 8g - R + i)
template <typename PixelT>
struct BlurRow {
    uint32_t w[2 * sizeof(PixelT)];
    uint32_t te;
};
template <typename PixelT>
__device__ __forceinline__ uint32_t blur_px(const BlurRow<PixelT>& r, int j) {
    if constexpr (sizeof(PixelT) == 2) return (j & 1) ? r.w[j >> 1] >> 16 : r.w[j >> 1] & 0xFFFFu;
    else return r.w[j];
}

template <typename PixelT>
__device__ __forceinline__ BlurRaw<PixelT> blur_load(const RadialIn& in, const uint8_t* img, int y, int g, bool own) {
    BlurRaw<PixelT> r;
    r.p0 = make_uint4(0u, 0u, 0u, 0u);
    r.p1 = r.p0;
    r.mb = 0u;
    // (radthr_row's reads: a group that straddles W stays inside the row's pitch_px pixels, and what it reads beyond W has no mask bit)
    if (own && y >= 0 && y < in.H) {
        const uint8_t* rp = img + (uint64_t)y * in.pitch + (uint64_t)g * (8u * sizeof(PixelT));
        r.p0 = *reinterpret_cast<const uint4*>(rp);
        if constexpr (sizeof(PixelT) == 4) r.p1 = *reinterpret_cast<const uint4*>(rp + 16);
        r.mb = in.maskbits[(uint64_t)y * in.mpitch + (uint32_t)g];
    }
    return r;
}
__device__ __forceinline__ uint4 blur_bins(const RadialIn& in, int y, int g, bool own) {
    if (own && y < in.H) return *reinterpret_cast<const uint4*>(in.bins + (uint64_t)y * in.bin_pitch + (uint64_t)g * 8u);
    return make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
}

// The tap rule on a loaded row.  Called by the whole wave: the neighbours' tap bits come across the lanes.
template <typename PixelT, int R>
__device__ __forceinline__ BlurRow<PixelT> blur_taps(const BlurRaw<PixelT>& raw, uint32_t limit) {
    BlurRow<PixelT> r;
    uint32_t tb = 0u;
    uint32_t p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        p[j] = sizeof(PixelT) == 2 ? lane_pixel<8>(raw.p0, j) : lane_pixel<4>(j < 4 ? raw.p0 : raw.p1, j & 3);
        const bool tap = radblur_tap((raw.mb >> j) & 1u, p[j], limit);
        tb |= (tap ? 1u : 0u) << j;
        p[j] = tap ? p[j] : 0u;
    }
    if constexpr (sizeof(PixelT) == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.w[k] = p[2 * k] | (p[2 * k + 1] << 16);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) r.w[k] = p[k];
    }
    const uint32_t left = (uint32_t)__shfl_up((int)tb, 1, 64), right = (uint32_t)__shfl_down((int)tb, 1, 64);
    r.te = (left >> (8 - R)) | (tb << R) | ((right & ((1u << R) - 1u)) << (8 + R));
    return r;
}

// The walk: rows ya .. yb - 1 of group g, row after row, the load of the row that enters the ring next in flight while this one is
// decided.  each(y, v, counts, centre, bn): v[j] the blurred value of pixel j where bit j of `counts` says the pixel is a tap, the centre
// row as the ring has it (p x tap) and the row's bin entries.  Called by the whole wave with ya, yb the same in every lane.
template <typename PixelT, int R, typename Each>
__device__ __forceinline__ void blur_walk(const RadialIn& in, const uint8_t* img, int g, bool own, int ya, int yb, Each&& each) {
    constexpr int N = 2 * R + 1;
    constexpr uint32_t kAll = (1u << N) - 1u;
    BlurRow<PixelT> ring[N];   // rows y - R .. y + R
#pragma unroll
    for (int k = 0; k < N; ++k) ring[k] = blur_taps<PixelT, R>(blur_load<PixelT>(in, img, ya - R + k, g, own), in.limit);
    for (int y = ya; y < yb; ++y) {
        // (both loads are read behind the arithmetic below)
        const BlurRaw<PixelT> raw = blur_load<PixelT>(in, img, y + 1 < yb ? y + 1 + R : in.H, g, own);
        const uint4 bn = blur_bins(in, y, g, own);
        // the vertical pass, then the horizontal one over the group and R columns of either neighbour
        uint32_t e[8 + 2 * R];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t s = 0u;
#pragma unroll
            for (int k = 0; k < N; ++k) s += radblur_w1(R, k - R) * blur_px(ring[k], j);
            e[R + j] = s;
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            e[i] = (uint32_t)__shfl_up((int)e[R + 8 - R + i], 1, 64);
            e[R + 8 + i] = (uint32_t)__shfl_down((int)e[R + i], 1, 64);
        }
        uint32_t present = ring[0].te;   // columns whose taps are all there
#pragma unroll
        for (int k = 1; k < N; ++k) present &= ring[k].te;
        const uint32_t counts = (ring[R].te >> R) & 0xFFu;
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t S = 0u;
#pragma unroll
            for (int d = -R; d <= R; ++d) S += radblur_w1(R, d) * e[R + j + d];
            v[j] = S >> radblur_shift(R);
            if (((counts >> j) & 1u) && ((present >> j) & kAll) != kAll) {   // a tap is missing: the weight of those that are there
                uint32_t Wn = 0u;
#pragma unroll
                for (int k = 0; k < N; ++k) Wn += radblur_w1(R, k - R) * radblur_row_weight(R, (ring[k].te >> j) & kAll);
                v[j] = radblur_value(R, S, Wn);
            }
        }
        each(y, v, counts, ring[R], bn);
#pragma unroll
        for (int k = 0; k + 1 < N; ++k) ring[k] = ring[k + 1];
        ring[N - 1] = blur_taps<PixelT, R>(raw, in.limit);
    }
}

template <typename PixelT, int R>
__global__ __launch_bounds__(kRadThrHistThreads) void k_radthr_hist_blur(RadThrArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t radthr_smem[];
    uint32_t* tab = reinterpret_cast<uint32_t*>(radthr_smem);
    const uint32_t n_tab = a.in.n_bins * (uint32_t)kRadThrCounters;
    const uint32_t frame = blockIdx.x, band = blockIdx.y;
    for (uint32_t i = threadIdx.x; i < n_tab; i += kRadThrHistThreads) tab[i] = 0u;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint8_t* img = static_cast<const uint8_t*>(a.in.image) + (uint64_t)frame * a.in.frame_stride;
    const int y0 = (int)(band * a.in.band_rows), y1 = min(a.in.H, y0 + (int)a.in.band_rows);
    const uint32_t strips = radblur_strips(a.in.W);
    const uint32_t units = strips * (uint32_t)((y1 - y0 + kRadBlurRunRows - 1) / kRadBlurRunRows);   // a unit: a run of rows of one strip
    for (uint32_t u = wave; u < units; u += (uint32_t)kRadThrHistWaves) {
        const uint32_t strip = u % strips, run = u / strips;
        const int g = (int)(strip * (uint32_t)kRadBlurOwners + lane) - 1;
        const bool own = g >= 0 && g * 8 < a.in.W;
        const bool owner = own && lane >= 1u && lane <= (uint32_t)kRadBlurOwners;
        const int ya = y0 + (int)run * kRadBlurRunRows, yb = min(y1, ya + kRadBlurRunRows);
        blur_walk<PixelT, R>(a.in, img, g, own, ya, yb, [tab, owner](int, const uint32_t (&v)[8], uint32_t counts, const BlurRow<PixelT>&, const uint4& bn) {
            if (!owner) return;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t b = radial_bin_entry(bn, j);
                if (((counts >> j) & 1u) && b != kRadialNone) atomicAdd(&tab[b * (uint32_t)kRadThrCounters + min(v[j], (uint32_t)kRadThrValues)], 1u);
            }
        });
    }
    __syncthreads();
    uint32_t* out = a.hist + (uint64_t)frame * n_tab;
    for (uint32_t i = threadIdx.x; i < n_tab; i += kRadThrHistThreads) {
        const uint32_t c = tab[i];
        if (c != 0u) atomicAdd(&out[i], c);
    }
}

// grid (strips x runs, frames): a wave per run of kRadBlurRunRows rows of one strip; what k_radthr_strong leaves, decided on v, and p >= 1
template <typename PixelT, int R>
__global__ __launch_bounds__(64) void k_radthr_strong_blur(RadThrArgs a) {
    __shared__ uint32_t s_cut[kRadThrMaxBins];
    const uint32_t lane = threadIdx.x;
    const uint32_t strips = radblur_strips(a.in.W);
    const uint32_t strip = blockIdx.x % strips, run = blockIdx.x / strips, frame = blockIdx.y;
    for (uint32_t i = lane; i < kRadThrMaxBins; i += 64u) s_cut[i] = i < a.in.n_bins ? a.cut[(uint64_t)frame * a.in.n_bins + i] : kRadThrNever;
    __syncthreads();
    const int g = (int)(strip * (uint32_t)kRadBlurOwners + lane) - 1;
    const bool own = g >= 0 && g * 8 < a.in.W;
    const bool owner = own && lane >= 1u && lane <= (uint32_t)kRadBlurOwners;
    const int ya = (int)run * kRadBlurRunRows, yb = min(a.in.H, ya + kRadBlurRunRows);
    const uint8_t* img = static_cast<const uint8_t*>(a.in.image) + (uint64_t)frame * a.in.frame_stride;
    uint8_t* plane = a.bits + (uint64_t)frame * a.plane_frame_stride;
    uint8_t* sbytes = a.strong_bytes + (uint64_t)frame * a.bytes_frame_stride;
    uint32_t cnt = 0u;
    blur_walk<PixelT, R>(a.in, img, g, own, ya, yb, [&](int y, const uint32_t (&v)[8], uint32_t counts, const BlurRow<PixelT>& centre, const uint4& bn) {
        uint32_t sb = 0u;
        if (owner) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t b = radial_bin_entry(bn, j);
                const uint32_t cutoff = s_cut[b & (kRadThrMaxBins - 1u)];
                const bool in_shell = ((counts >> j) & 1u) && b != kRadialNone;
                if (in_shell && v[j] > cutoff && (double)v[j] > a.threshold && blur_px(centre, j) >= 1u) sb |= 1u << j;
            }
            if (sb) {
                plane[(uint64_t)y * a.in.mpitch + (uint32_t)g] = (uint8_t)sb;   // (the plane is all zero when the kernel starts)
                if (a.occ) {
                    const uint32_t ob = (uint32_t)y * a.occ_spr + ((uint32_t)g >> 4);
                    atomicOr(a.occ + (uint64_t)frame * a.occ_frame_words + (ob >> 5), 1u << (ob & 31u));
                }
            }
            if (a.dense_mask) {
                uint2 bytes;
                bytes.x = (sb & 1u) | ((sb & 2u) << 7) | ((sb & 4u) << 14) | ((sb & 8u) << 21);
                bytes.y = ((sb >> 4) & 1u) | ((sb & 0x20u) << 3) | ((sb & 0x40u) << 10) | ((sb & 0x80u) << 17);
                *reinterpret_cast<uint2*>(sbytes + (uint64_t)y * a.bpitch + (uint64_t)g * 8u) = bytes;
            }
        }
        cnt += (uint32_t)__popc(sb);
        if ((y & (kTileRows - 1)) == kTileRows - 1 || y + 1 == yb) {   // the tile's count (a run starts on a tile's first row)
            if (__ballot(cnt != 0u)) {
                const uint32_t total = __builtin_amdgcn_readlane(wave_inclusive_scan(cnt), 63);
                if (lane == 0u) atomicAdd(a.tile_counts + (uint64_t)frame * a.n_tiles + (uint32_t)(y / kTileRows), total);
            }
            cnt = 0u;
        }
    });
}

}  // namespace ffsamd
