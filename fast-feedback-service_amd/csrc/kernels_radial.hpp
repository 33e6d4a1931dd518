// kernels_radial.hpp (included by ffs_products.hip only) -- the per-frame radial profile (ffs_ctx_set_radial_bins):
// per frame and bin of a caller-defined bin map, the count, the sum and the sum of squares of the pixels that the valid-pixel mask,
// max_valid and (32-bit pixels) the oracle's p < 2^24 rule let through.  The reference has no counterpart (its per-image output is the
// strong mask, spotfinder/spotfinder.cc:887-933); DIALS builds its radial_profile threshold and its per-image analysis on this quantity.
//
// Two launches, no global atomics (the sums are integers: any order gives the same bits, and this order's cost does not depend on
// contention):
//   k_radial<PixelT>  grid (frames, bands): a workgroup of four waves streams a band of contiguous rows of one frame -- 16 B of pixels,
//                     the matching bin entries and the mask bits per lane and load, the next load in flight while this one is counted --
//                     into a table in LDS (n_bins x 20 B), and stores the table as the band's partial.  The frame is the grid's x: the
//                     workgroups that read the same rows of the bin map are dispatched together and find them in L2 / the Infinity Cache.
//   k_radial_sum      grid (bins / 256, frames): a thread per (frame, bin) adds the bands' partials into the result (pinned host memory).
// A lane keeps a RUN of equal bins in registers (bin, count, sum, sum of squares) across loads and rows -- a pixel's bin is usually its
// left and upper neighbour's -- and hands it over only when the bin changes, and at the end of the band.  Where the bin changes the lane
// adds its run to the table by itself (radial_add: three LDS adds under its own exec bit).  At the end of the band, where every lane of the
// wave holds a run and most hold the same few bins, handing over is a step of the whole wave (radial_flush): the distinct bins are peeled
// one at a time, the matching lanes' runs reduced across the wave, ONE LDS add per distinct bin -- sixty-four lanes adding to one LDS
// address would serialise.  (Measured and dropped, DESIGN.md section 3.6: the wave step at every change of any lane's bin, 5.5 ms for 32 Eiger
// frames and 100 shells against 0.59 ms -- a wave of 512 pixels nearly always has SOME lane on a shell boundary -- and the wave step only
// where sixteen or more lanes change in one step, 5.0 ms: the peel's dependent butterflies cost more than the adds that meet on an address.)
// k_radial<., true> reads the map in one byte an entry (maps of at most 255 bins, tuning "radial_map8": measured no faster, off).
#pragma once
#include "ffs_device.h"

namespace ffsamd {

constexpr uint32_t kRadialNone = 0xFFFFu;    // a bin-map entry that is in no bin (ffs_hip.h)
constexpr uint32_t kRadialMaxBins = 1024;    // 20 KB of LDS a workgroup
constexpr int kRadialThreads = 256;
constexpr int kRadialWaves = kRadialThreads / 64;

// What the band walk reads (radial_walk): k_radial's input, and the radial-profile threshold's (kernels_radthr.hpp)
struct RadialIn {
    const void* image;          // [frame][y][pitch bytes], as the threshold stage reads it
    uint64_t frame_stride;
    uint32_t pitch;
    const uint8_t* maskbits;    // the context's valid-pixel bit plane, rows of mpitch bytes
    uint32_t mpitch;
    const uint8_t* bins8;       // the same map in one byte an entry (0xFF: in no bin) when it has at most 255 bins and tuning "radial_map8" asks; else null
    const uint16_t* bins;       // [H][bin_pitch] entries; the entries beyond W are kRadialNone, every other one is < n_bins or kRadialNone
    uint32_t bin_pitch;         // = Layout::pitch_px
    int W, H;
    uint32_t n_bins;
    uint32_t n_bands, band_rows;   // bands of a frame (the grid's y) and the rows of one
    uint32_t limit;             // a pixel counts when p < limit (launch_geometry.hpp, counting_limit)
};
struct RadialArgs {
    RadialIn in;
    // partials, [frame][band][n_bins] each, and results, [frame][n_bins] each
    uint64_t *p_sum, *p_sq;
    uint32_t* p_count;
    uint64_t *r_sum, *r_sq;
    uint32_t* r_count;
};

static inline size_t radial_lds_bytes(uint32_t n_bins) { return (size_t)n_bins * 20u; }

// What a lane has of one load: PX = 16 / sizeof(PixelT) pixels, their bin entries and their mask bits (all zero / none outside the row)
template <typename PixelT>
struct RadialLoad {
    uint4 px;
    uint4 bn;      // 16-bit pixels: eight entries; 32-bit pixels: four, in x and y
    uint32_t mb;
};

// (one byte an entry: widened to the two-byte form's registers, so the counting loop is one)
__device__ __forceinline__ uint32_t radial_widen2(uint32_t b2) {   // two entries in the low 16 bits -> two 16-bit entries, 0xFF -> 0xFFFF
    const uint32_t lo = b2 & 0xFFu, hi = (b2 >> 8) & 0xFFu;
    return (lo == 0xFFu ? 0xFFFFu : lo) | ((hi == 0xFFu ? 0xFFFFu : hi) << 16);
}
template <typename PixelT, bool MAP8>
__device__ __forceinline__ RadialLoad<PixelT> radial_load(const RadialIn& a, const uint8_t* img, int y, int x0) {
    constexpr int PX = 16 / (int)sizeof(PixelT);
    RadialLoad<PixelT> r;
    r.px = make_uint4(0u, 0u, 0u, 0u);
    r.bn = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    r.mb = 0u;
    // (a lane whose first pixel is beyond W loads nothing; one that straddles W stays inside the row's pitch_px pixels, and what it reads
    // beyond W has no mask bit and no bin)
    if (y < a.H && x0 < a.W) {
        r.px = *reinterpret_cast<const uint4*>(img + (uint64_t)y * a.pitch + (uint64_t)x0 * sizeof(PixelT));
        const uint64_t at = (uint64_t)y * a.bin_pitch + (uint32_t)x0;
        if constexpr (PX == 8) {
            if constexpr (MAP8) {
                const uint2 b8 = *reinterpret_cast<const uint2*>(a.bins8 + at);
                r.bn = make_uint4(radial_widen2(b8.x), radial_widen2(b8.x >> 16), radial_widen2(b8.y), radial_widen2(b8.y >> 16));
            } else {
                r.bn = *reinterpret_cast<const uint4*>(a.bins + at);
            }
            r.mb = a.maskbits[(uint64_t)y * a.mpitch + (uint32_t)(x0 >> 3)];
        } else {
            if constexpr (MAP8) {
                const uint32_t b8 = *reinterpret_cast<const uint32_t*>(a.bins8 + at);
                r.bn.x = radial_widen2(b8);
                r.bn.y = radial_widen2(b8 >> 16);
            } else {
                const uint2 b2 = *reinterpret_cast<const uint2*>(a.bins + at);
                r.bn.x = b2.x;
                r.bn.y = b2.y;
            }
            r.mb = ((uint32_t)a.maskbits[(uint64_t)y * a.mpitch + (uint32_t)(x0 >> 3)] >> (x0 & 4)) & 0xFu;
        }
    }
    return r;
}

__device__ __forceinline__ uint32_t radial_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t radial_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// A lane hands its run to the workgroup's table by itself: where its bin changes in the middle of a band.  The lanes of a wave that get here
// in the same step stand at different shell boundaries (their pixels are eight or four columns apart), so their adds rarely meet on one address.
__device__ __forceinline__ void radial_add(uint32_t bin, uint32_t cnt, uint64_t s, uint64_t q, uint64_t* l_sum, uint64_t* l_sq, uint32_t* l_count) {
    atomicAdd(&l_count[bin], cnt);
    atomicAdd(reinterpret_cast<unsigned long long*>(&l_sum[bin]), (unsigned long long)s);
    atomicAdd(reinterpret_cast<unsigned long long*>(&l_sq[bin]), (unsigned long long)q);
}

// The lanes of `pending` (a ballot: the same value in every lane) hand their runs to the workgroup's table, combined inside the wave first: at
// the end of a band, where all sixty-four lanes hold a run and most of them the same few bins.  Called by the whole wave.
__device__ __forceinline__ void radial_flush(uint64_t pending, uint32_t bin, uint32_t cnt, uint64_t s, uint64_t q, uint64_t* l_sum, uint64_t* l_sq,
                                             uint32_t* l_count) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool mine = (pending >> lane) & 1ull;
    while (pending) {
        const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__ffsll((unsigned long long)pending) - 1));
        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)lead);
        const bool match = mine && bin == b;
        const uint64_t mm = __ballot(match);
        uint32_t c = match ? cnt : 0u;
        uint64_t ss = match ? s : 0ull, qq = match ? q : 0ull;
        if (mm & (mm - 1)) {   // more lanes than the leading one hold this bin: their runs become one
            c = radial_wave_sum(c);
            ss = radial_wave_sum(ss);
            qq = radial_wave_sum(qq);
        }
        if (lane == lead) {
            atomicAdd(&l_count[b], c);
            atomicAdd(reinterpret_cast<unsigned long long*>(&l_sum[b]), (unsigned long long)ss);
            atomicAdd(reinterpret_cast<unsigned long long*>(&l_sq[b]), (unsigned long long)qq);
        }
        pending &= ~mm;
    }
}

// The rule: a pixel counts when the mask has its bit, the map has it in a bin and its value is below the limit
__device__ __forceinline__ bool radial_counts(const RadialIn& a, uint32_t mask_bit, uint32_t b, uint32_t p) { return mask_bit && b != kRadialNone && p < a.limit; }

// Entry j of the bin entries a lane has of one load (two entries a word; with 32-bit pixels only the first four exist)
__device__ __forceinline__ uint32_t radial_bin_entry(const uint4& bn, int j) {
    const uint32_t bw = j < 2 ? bn.x : j < 4 ? bn.y : j < 6 ? bn.z : bn.w;
    return (j & 1) ? bw >> 16 : bw & 0xFFFFu;
}

// The band walk of a workgroup of WAVES waves over band `band` of frame `frame`: wave w takes rows w, w + WAVES, ... of the band, each from
// x = 0 in steps of 64 x PX pixels while x < W, with the next step's load in flight while this one is counted, and folds every pixel of
// every load, in that order, into what the lane keeps: run = each(run, p, b, mask_bit) -- value, bin entry, valid-pixel bit; whether the pixel
// counts is radial_counts of the three.  Returns the lane's last run.  (The run goes in and out BY VALUE and `each` applies the rule itself: a
// lambda that changed its run through a reference, or was handed the rule's result, compiled to another loop body -- profiles/r23a.)
template <typename PixelT, bool MAP8, int WAVES, typename Run, typename Each>
__device__ __forceinline__ Run radial_walk(const RadialIn& a, uint32_t frame, uint32_t band, Run run, Each&& each) {
    constexpr int PX = 16 / (int)sizeof(PixelT);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (the row loop below is the same in every lane)
    const uint8_t* img = static_cast<const uint8_t*>(a.image) + (uint64_t)frame * a.frame_stride;
    const int y_end = min(a.H, (int)((band + 1u) * a.band_rows));
    const int step = 64 * PX;                      // pixels of a wave's load
    int y = (int)(band * a.band_rows + wave), xw = 0;
    RadialLoad<PixelT> ld = radial_load<PixelT, MAP8>(a, img, y < y_end ? y : a.H, xw + (int)lane * PX);
    while (y < y_end) {
        int yn = y, xn = xw + step;
        if (xn >= a.W) { xn = 0; yn = y + WAVES; }
        const RadialLoad<PixelT> nx = radial_load<PixelT, MAP8>(a, img, yn < y_end ? yn : a.H, xn + (int)lane * PX);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const uint32_t p = lane_pixel<PX>(ld.px, j), b = radial_bin_entry(ld.bn, j);
            run = each(run, p, b, (ld.mb >> j) & 1u);
        }
        ld = nx;
        y = yn;
        xw = xn;
    }
    return run;
}

struct RadialRun { uint32_t cur, cnt; uint64_t s, q; };   // a lane's run of equal bins: the bin, count, sum, sum of squares

template <typename PixelT, bool MAP8>
__global__ __launch_bounds__(kRadialThreads) void k_radial(RadialArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t radial_smem[];
    const uint32_t n_bins = a.in.n_bins;
    uint64_t* l_sum = reinterpret_cast<uint64_t*>(radial_smem);
    uint64_t* l_sq = l_sum + n_bins;
    uint32_t* l_count = reinterpret_cast<uint32_t*>(l_sq + n_bins);
    const uint32_t frame = blockIdx.x, band = blockIdx.y;
    for (uint32_t i = threadIdx.x; i < n_bins; i += kRadialThreads) {
        l_sum[i] = 0ull;
        l_sq[i] = 0ull;
        l_count[i] = 0u;
    }
    __syncthreads();

    const RadialRun last = radial_walk<PixelT, MAP8, kRadialWaves>(a.in, frame, band, RadialRun{kRadialNone, 0u, 0ull, 0ull}, [&a, l_sum, l_sq, l_count](RadialRun r, uint32_t p, uint32_t b, uint32_t m) {
        const bool ok = radial_counts(a.in, m, b, p);
        const bool change = ok && b != r.cur;
        if (change) {
            if (r.cnt != 0u) radial_add(r.cur, r.cnt, r.s, r.q, l_sum, l_sq, l_count);
            r.cur = b;
            r.cnt = 0u;
            r.s = 0ull;
            r.q = 0ull;
        }
        if (ok) {
            ++r.cnt;
            r.s += p;
            r.q += (uint64_t)p * p;
        }
        return r;
    });
    {
        const uint64_t pending = __ballot(last.cnt != 0u);
        if (pending) radial_flush(pending, last.cur, last.cnt, last.s, last.q, l_sum, l_sq, l_count);
    }
    __syncthreads();
    const uint64_t base = ((uint64_t)frame * a.in.n_bands + band) * n_bins;
    for (uint32_t i = threadIdx.x; i < n_bins; i += kRadialThreads) {
        a.p_sum[base + i] = l_sum[i];
        a.p_sq[base + i] = l_sq[i];
        a.p_count[base + i] = l_count[i];
    }
}

__global__ __launch_bounds__(256) void k_radial_sum(RadialArgs a) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x, frame = blockIdx.y;
    if (b >= a.in.n_bins) return;
    uint32_t c = 0u;
    uint64_t s = 0ull, q = 0ull;
    uint64_t at = (uint64_t)frame * a.in.n_bands * a.in.n_bins + b;
    for (uint32_t band = 0; band < a.in.n_bands; ++band, at += a.in.n_bins) {
        c += a.p_count[at];
        s += a.p_sum[at];
        q += a.p_sq[at];
    }
    const uint64_t out = (uint64_t)frame * a.in.n_bins + b;
    a.r_count[out] = c;
    a.r_sum[out] = s;
    a.r_sq[out] = q;
}

}  // namespace ffsamd
