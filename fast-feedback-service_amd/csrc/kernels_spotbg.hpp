// kernels_spotbg.hpp (included by ffs_spotbg.hip only) -- the per-spot constant background (ffs_stream_spot_backgrounds, DESIGN.md section
// 3.8): per reflection of a batch, the Tukey-fenced level of the ring of pixels around its bounding box.  The model and its decisions are
// spot_background_model.hpp's (the reference's tukey_constant_background, include/integrator/background.hpp, in integers); this file is how a
// wave gets there.  The second model of the same ring, the robust Poisson GLM (ffs_stream_spot_backgrounds_glm, section 3.8b), is
// k_spot_background_glm at the end of the file; ring and histogram are one function, spotbg_ring_histogram, for both.
//
// One launch, k_spot_background<PixelT>: a wave per reflection, kSpotBgWaves of them a workgroup.
//   Ring.      The padded box, clipped to the frame, without the box itself, is four rectangles: the rows above and below the box over the
//              padded width (up to `border` rows each) and the columns left and right of it over the box's height (up to `border` columns
//              each).  The two bands are one index space of pw x (ht + hb) pixels, the two sides one of (wl + wr) x bh; the lanes walk the
//              two, sixty-four pixels a step.  A box never costs its area: a spot as wide as the frame costs its perimeter.
//   Histogram. 256 dwords of LDS per wave, one LDS add per valid pixel below 256.  The tail (values at or above 256) and nothing else is
//              counted in a register per lane and summed across the wave at the end: under a Poisson(300) background every pixel of the
//              ring is in the tail, and sixty-four lanes adding to one LDS address would serialise.
//              Kept: the plain per-lane add.  A Poisson(3) ring does put most of its pixels into eight bins, and adds of one wave
//              instruction that meet on an address are serialised (DESIGN.md section 3.6 measured that for the radial profile), but a
//              typical ring is under 100 pixels -- two wave instructions.  Measured and dropped: counting the lanes
//              that agree with a ballot and adding once per distinct bin, 0.072 ms against 0.051 ms for the 45 000 spots of 32 Eiger
//              frames -- peeling eight to ten distinct bins a step costs more than the adds that meet.  It stays behind
//              FFS_EXP_SPOTBG_COMBINE for the experiments build, as the A/B partner.
//   Decision.  By the whole wave: lane l owns bins 4 l .. 4 l + 3 (one 16-byte LDS load), an inclusive scan of the lanes' totals across the
//              wave places every lane's bins among the sorted values, the lane that holds a quartile's position is found by __ballot and
//              hands its bin to the others; the fence is applied by every lane to its own four bins and the inliers are summed across the
//              wave.  Lane 0 stores the record.
// The mask's bit plane (rows of mpitch bytes, bit x & 7 of byte x >> 3), the pixel pitch (bytes, not W) and the frame stride are addressed as
// kernels_radial.hpp does; a pixel counts under the radial profile's rules (mask bit, p < limit = min(max_valid + 1, 2^24)).
// Bounds: the host checks every box against the frame (x_min <= x_max < W, y_min <= y_max < H, frame < n_frames) before the launch; the
// kernel clips the ring to 0 .. W - 1, 0 .. H - 1, and clamps the box into the frame again by itself.
#pragma once
#include "ffs_device.h"
#include "spot_background_glm_model.hpp"
#include "spot_background_model.hpp"

namespace ffsamd {

constexpr int kSpotBgWaves = 4;                        // reflections per workgroup (1 KB of LDS each)
constexpr int kSpotBgThreads = 64 * kSpotBgWaves;
constexpr uint32_t kSpotBgInvalid = 0xFFFFFFFFu;      // not a pixel value that counts: every valid pixel is below 2^24

struct SpotBgBox {   // 16 B: one load
    uint16_t x_min, x_max, y_min, y_max;   // (frames are at most 65536 pixels wide and high: ffs_spotbg.hip refuses others)
    uint32_t frame;                        // frame in the batch
    uint32_t pad;
};
struct SpotBgOut {   // = ffs_spot_background (ffs_spotbg.hip asserts the layout)
    uint32_t n_pixels, n_overflow;
    int32_t q1, median, q3;
    uint32_t n_inliers;
    uint64_t inlier_sum;
    uint32_t status, reserved;
    double mean;     // filled in by the host
};

struct SpotBgArgs {
    const void* image;          // [frame][y][pitch bytes], where the batch left its frames
    uint64_t frame_stride;
    uint32_t pitch;
    const uint8_t* maskbits;    // the context's valid-pixel bit plane, rows of mpitch bytes
    uint32_t mpitch;
    int W, H;
    uint32_t limit;             // a pixel counts when p < limit: max_valid + 1 and 2^24, whichever is smaller
    int border;                 // 1 .. kSpotBgMaxBorder
    uint32_t n;                 // reflections
    const SpotBgBox* boxes;     // [n]
    SpotBgOut* out;             // [n] (pinned host memory)
};

__device__ __forceinline__ uint32_t spotbg_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t spotbg_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The bin that holds sorted position `pos` (1-based, at most the bins' total): lane `lane` owns bins 4 lane .. 4 lane + 3 with the counts h,
// `before` values lie in the bins of the lanes below it.  Called by the whole wave; the same value in every lane (-1: no such position).
__device__ __forceinline__ int32_t spotbg_wave_quantile(uint64_t pos, const uint4& h, uint32_t before, uint32_t lane) {
    const uint64_t c0 = (uint64_t)before + h.x, c1 = c0 + h.y, c2 = c1 + h.z, c3 = c2 + h.w;
    const bool mine = before < pos && pos <= c3;
    const int32_t v = (int32_t)(4u * lane) + (pos <= c0 ? 0 : pos <= c1 ? 1 : pos <= c2 ? 2 : 3);
    const uint64_t holders = __ballot(mine);
    if (holders == 0ull) return -1;
    return __shfl(v, (int)(__ffsll((unsigned long long)holders) - 1), 64);
}

// The ring of reflection r, pixel by pixel: the clipped geometry of the header's comment and the validity rules.  Both kernels walk it.
template <typename PixelT>
struct SpotBgRing {
    int X0, x_min, x_max, Y0, y_min, y_max;
    uint32_t pw, ht, wl, sw, n_band, total;   // (total: at most 32 (W + H) pixels)
    const uint8_t* img;
    const uint8_t* maskbits;
    uint32_t pitch, mpitch, limit;

    __device__ __forceinline__ SpotBgRing(const SpotBgArgs& a, uint32_t r) {
        const SpotBgBox bx = a.boxes[r];
        x_max = min((int)bx.x_max, a.W - 1), x_min = min((int)bx.x_min, x_max);
        y_max = min((int)bx.y_max, a.H - 1), y_min = min((int)bx.y_min, y_max);
        X0 = max(0, x_min - a.border);
        Y0 = max(0, y_min - a.border);
        const int X1 = min(a.W - 1, x_max + a.border), Y1 = min(a.H - 1, y_max + a.border);
        pw = (uint32_t)(X1 - X0 + 1), ht = (uint32_t)(y_min - Y0);
        const uint32_t hb = (uint32_t)(Y1 - y_max), wr = (uint32_t)(X1 - x_max), bh = (uint32_t)(y_max - y_min + 1);
        wl = (uint32_t)(x_min - X0);
        sw = wl + wr;
        n_band = pw * (ht + hb), total = n_band + sw * bh;
        img = static_cast<const uint8_t*>(a.image) + (uint64_t)bx.frame * a.frame_stride;
        maskbits = a.maskbits;
        pitch = a.pitch, mpitch = a.mpitch, limit = a.limit;
    }
    // pixel i of the ring, in the order bands then sides: its value when it is valid, kSpotBgInvalid else
    __device__ __forceinline__ uint32_t pixel(uint32_t i) const {
        int x, y;
        if (i < n_band) {   // the rows above the box, then the rows below it
            const uint32_t row = i / pw, col = i - row * pw;
            x = X0 + (int)col;
            y = row < ht ? Y0 + (int)row : y_max + 1 + (int)(row - ht);
        } else {            // the columns left of the box, then the columns right of it (sw > 0 here)
            const uint32_t j = i - n_band, row = j / sw, col = j - row * sw;
            y = y_min + (int)row;
            x = col < wl ? X0 + (int)col : x_max + 1 + (int)(col - wl);
        }
        const uint32_t p = *reinterpret_cast<const PixelT*>(img + (uint64_t)y * pitch + (uint64_t)x * sizeof(PixelT));
        const uint32_t mb = ((uint32_t)maskbits[(uint64_t)y * mpitch + (uint32_t)(x >> 3)] >> (x & 7)) & 1u;
        return (mb && p < limit) ? p : kSpotBgInvalid;
    }
};

// The ring of reflection r into the wave's histogram (256 zeroed dwords of LDS), one plain LDS add per valid pixel below kSpotBgBins;
// returns this lane's valid pixels at or above kSpotBgBins.  Called by the whole wave.
template <typename PixelT>
__device__ __forceinline__ uint32_t spotbg_ring_histogram(const SpotBgArgs& a, uint32_t r, uint32_t lane, uint32_t* hist) {
    const SpotBgRing<PixelT> ring(a, r);
    uint32_t n_tail = 0u;
    for (uint32_t i = lane; i < ring.total; i += 64u) {
        const uint32_t p = ring.pixel(i);
        if (p < (uint32_t)kSpotBgBins) atomicAdd(&hist[p], 1u);
        else if (p != kSpotBgInvalid) ++n_tail;
    }
    return n_tail;
}

// Inclusive scan of one value per lane across the wave
__device__ __forceinline__ uint32_t spotbg_wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if ((int)lane >= d) v += o;
    }
    return v;
}

template <typename PixelT>
__global__ __launch_bounds__(kSpotBgThreads) void k_spot_background(SpotBgArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t spotbg_hist[kSpotBgWaves][kSpotBgBins];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* hist = spotbg_hist[wave];
    const uint32_t r = blockIdx.x * (uint32_t)kSpotBgWaves + wave;
    const bool live = r < a.n;   // (the same in every lane of a wave; the two barriers below are reached by every wave)
    *reinterpret_cast<uint4*>(hist + 4u * lane) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    uint32_t n_tail = 0u;   // this lane's valid pixels at or above kSpotBgBins
    if (live) {
#ifndef FFS_EXP_SPOTBG_COMBINE
        n_tail = spotbg_ring_histogram<PixelT>(a, r, lane, hist);
#else
        // The A/B partner (experiments build with EXPFLAGS=-DFFS_EXP_SPOTBG_COMBINE, same results): the lanes of one step that hold the
        // same bin are counted with a ballot and ONE lane adds their number -- the wave walks the ring in uniform steps for that.
        const SpotBgRing<PixelT> ring(a, r);
        for (uint32_t base = 0u; base < ring.total; base += 64u) {
            const uint32_t i = base + lane;
            const uint32_t p = i < ring.total ? ring.pixel(i) : kSpotBgInvalid;
            if (p >= (uint32_t)kSpotBgBins && p != kSpotBgInvalid) ++n_tail;
            uint64_t pending = __ballot(p < (uint32_t)kSpotBgBins);
            while (pending) {
                const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__ffsll((unsigned long long)pending) - 1));
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)p, (int)lead);
                const uint64_t same = __ballot(p == v);
                if (lane == lead) hist[v] += (uint32_t)__popcll((unsigned long long)same);
                pending &= ~same;
            }
        }
#endif
    }
    __syncthreads();
    if (!live) return;

    const uint4 h = *reinterpret_cast<const uint4*>(hist + 4u * lane);
    const uint32_t mine = h.x + h.y + h.z + h.w;
    const uint32_t upto = spotbg_wave_scan(mine, lane);
    const uint32_t before = upto - mine;
    const uint32_t in_bins = __shfl(upto, 63, 64);
    const uint32_t n_overflow = spotbg_wave_sum(n_tail);
    const uint64_t n = (uint64_t)in_bins + n_overflow;

    SpotBgOut o;
    o.n_pixels = (uint32_t)n;
    o.n_overflow = n_overflow;
    o.q1 = o.median = o.q3 = -1;
    o.n_inliers = 0u;
    o.inlier_sum = 0ull;
    o.reserved = 0u;
    o.mean = 0.0;
    o.status = spotbg_status_of_counts(n, n_overflow);
    if (o.status == kSpotBgOk) {
        const SpotBgPositions pos = spotbg_positions(n);
        o.q1 = spotbg_wave_quantile(pos.p25, h, before, lane);
        o.median = spotbg_wave_quantile(pos.p50, h, before, lane);
        o.q3 = spotbg_wave_quantile(pos.p75, h, before, lane);
        if (spotbg_range_too_small(o.q1, o.q3)) {
            o.status = kSpotBgRange;
        } else {
            uint32_t cnt = 0u;
            uint64_t sum = 0ull;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int32_t v = (int32_t)(4u * lane) + k;
                const uint32_t c = k == 0 ? h.x : k == 1 ? h.y : k == 2 ? h.z : h.w;
                if (spotbg_inlier(v, o.q1, o.q3)) {
                    cnt += c;
                    sum += (uint64_t)v * c;
                }
            }
            cnt = spotbg_wave_sum(cnt);
            sum = spotbg_wave_sum(sum);
            o.status = spotbg_status_of_inliers(cnt);
            if (o.status == kSpotBgOk) {
                o.n_inliers = cnt;
                o.inlier_sum = sum;
            }
        }
    }
    if (lane == 0u) a.out[r] = o;
}

// ---- the robust Poisson GLM model (ffs_stream_spot_backgrounds_glm, DESIGN.md section 3.8b, spot_background_glm_model.hpp) ----
// k_spot_background_glm<PixelT>: the same wave per reflection, the same ring and histogram.  Then
//   Tables.  Lane l owns bins 4 l .. 4 l + 3; the scan of the lanes' counts gives C (the inclusive prefix counts), a second scan of the
//            lanes' sums of v * count gives S; both go to LDS, 1 KB each per wave (3 KB a wave with the histogram, 12 KB a workgroup).
//   Loop.    Wave-uniform: every lane runs the header's scalar float64 sequence on the same values, so the wave never diverges and the
//            four LDS reads of a step are broadcasts.  Its bounds are the header's (100 steps, 600 terms of the recurrence); no array, no
//            scratch.
//   Record.  Lane 0 stores it, beta and mean included: the host computes nothing afterwards.
struct SpotBgGlmOut {   // = ffs_spot_background_glm (ffs_spotbg.hip asserts the layout)
    uint32_t n_pixels, n_overflow;
    int32_t median;
    uint32_t n_iter;
    uint32_t status, reserved;
    double beta, mean;
};

// S's largest value is 255 * (pixels of a ring), and a ring has at most 2 * border * (W + H) pixels of frames the host holds to 65536 a side
static_assert(255ull * 2ull * kSpotBgMaxBorder * (65536ull + 65536ull) <= 0xFFFFFFFFull, "the prefix sums of v * count fit 32 bits");

struct SpotBgGlmLdsTables {   // the model's view of a wave's two tables
    const uint32_t* c;
    const uint32_t* s;
    FFS_SPOTBG_HD uint64_t count(int32_t j) const { return j < 0 ? 0ull : (uint64_t)c[j]; }
    FFS_SPOTBG_HD uint64_t sum(int32_t j) const { return j < 0 ? 0ull : (uint64_t)s[j]; }
};

template <typename PixelT>
__global__ __launch_bounds__(kSpotBgThreads) void k_spot_background_glm(SpotBgArgs a, SpotBgGlmOut* out) {
    __shared__ __attribute__((aligned(16))) uint32_t spotbg_hist[kSpotBgWaves][kSpotBgBins];
    __shared__ __attribute__((aligned(16))) uint32_t spotbg_count[kSpotBgWaves][kSpotBgBins];
    __shared__ __attribute__((aligned(16))) uint32_t spotbg_sum[kSpotBgWaves][kSpotBgBins];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* hist = spotbg_hist[wave];
    const uint32_t r = blockIdx.x * (uint32_t)kSpotBgWaves + wave;
    const bool live = r < a.n;   // (the same in every lane of a wave; the three barriers below are reached by every wave)
    *reinterpret_cast<uint4*>(hist + 4u * lane) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    uint32_t n_tail = 0u;
    if (live) n_tail = spotbg_ring_histogram<PixelT>(a, r, lane, hist);
    __syncthreads();

    const uint4 h = *reinterpret_cast<const uint4*>(hist + 4u * lane);
    const uint32_t mine = h.x + h.y + h.z + h.w;
    const uint32_t v0 = 4u * lane;
    const uint32_t mine_sum = v0 * h.x + (v0 + 1u) * h.y + (v0 + 2u) * h.z + (v0 + 3u) * h.w;
    const uint32_t upto = spotbg_wave_scan(mine, lane), upto_sum = spotbg_wave_scan(mine_sum, lane);
    const uint32_t before = upto - mine, before_sum = upto_sum - mine_sum;
    uint4 ct, st;
    ct.x = before + h.x, ct.y = ct.x + h.y, ct.z = ct.y + h.z, ct.w = ct.z + h.w;
    st.x = before_sum + v0 * h.x, st.y = st.x + (v0 + 1u) * h.y, st.z = st.y + (v0 + 2u) * h.z, st.w = st.z + (v0 + 3u) * h.w;
    *reinterpret_cast<uint4*>(spotbg_count[wave] + 4u * lane) = ct;
    *reinterpret_cast<uint4*>(spotbg_sum[wave] + 4u * lane) = st;
    __syncthreads();
    if (!live) return;

    const uint32_t in_bins = __shfl(upto, 63, 64);
    const uint32_t n_overflow = spotbg_wave_sum(n_tail);
    const uint64_t n = (uint64_t)in_bins + n_overflow;
    SpotBgGlmOut o;
    o.n_pixels = (uint32_t)n;
    o.n_overflow = n_overflow;
    o.median = -1;
    o.n_iter = 0u;
    o.reserved = 0u;
    o.beta = 0.0;
    o.mean = 0.0;
    o.status = spotbg_glm_status_of_counts(n, n_overflow);
    if (o.status == kSpotBgOk) {
        o.median = spotbg_wave_quantile(spotbg_glm_median_position(n), h, before, lane);
        const SpotBgGlmLdsTables tables{spotbg_count[wave], spotbg_sum[wave]};
        if (spotbg_glm_all_zero(n, n_overflow, tables.count(0))) {
            o.beta = -__builtin_inf();
        } else {
            const SpotBgGlmFit fit = spotbg_glm_fit(n, o.median, tables);
            o.beta = fit.beta;
            o.mean = fit.mean;
            o.n_iter = fit.n_iter;
            o.status = fit.status;
        }
    }
    if (lane == 0u) out[r] = o;
}

}  // namespace ffsamd
