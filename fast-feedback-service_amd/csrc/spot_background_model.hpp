// spot_background_model.hpp -- the decisions of the per-spot constant background (ffs_stream_spot_backgrounds) as plain
// integer arithmetic: the quartile positions, the order of the status checks and the fence predicate.  No HIP header: the kernel
// (kernels_spotbg.hpp) and a plain C++ test program (tests/spot_background_check.cc) compile the same text.
//
// The model is the Tukey fence over a histogram of one-count bins: kSpotBgBins bins for the values 0 .. kSpotBgBins - 1 and a high tail that
// is counted, not resolved.  It restates the constant background of the reference's integrator (include/integrator/background.hpp,
// tukey_constant_background) in integers.  The reference compares in float64 -- overflow > 0.25 N, v < q1 - 1.5 iqr, v > q3 + 1.5 iqr,
// q3 + 1.5 iqr >= 256 -- on operands that are small integers or halves of them, so the same comparisons of the doubled values are exact and
// equal: 4 overflow > N, 2 v < 2 q1 - 3 iqr, 2 v > 2 q3 + 3 iqr, 2 q3 + 3 iqr >= 512.
// Order of the checks, the reference's: no pixels (1), too much in the tail (2), the upper fence beyond the bins (3), no inliers (4).
// Status 4 cannot be reached once 1-3 are excluded -- q1's bin is never empty and always inside the fence -- and is kept for parity with that
// order.  Once status 2 is excluded all three quartiles lie inside the bins: the tail holds at most N / 4 values, so the bins hold at least
// ceil(3 N / 4) >= (3 N + 1) / 4, the position of q3.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FFS_SPOTBG_HD __host__ __device__
#else
#define FFS_SPOTBG_HD
#endif

namespace ffsamd {

constexpr int kSpotBgBins = 256;          // one-count bins: the values 0 .. 255; a value at or above goes to the tail
constexpr uint32_t kSpotBgMaxBorder = 16;

// FFS_SPOT_BG_* of ffs_hip.h
constexpr uint32_t kSpotBgOk = 0, kSpotBgNoPixels = 1, kSpotBgOverflow = 2, kSpotBgRange = 3, kSpotBgNoInliers = 4;

// 1-based positions of q1, the median and q3 among n sorted values
struct SpotBgPositions {
    uint64_t p25, p50, p75;
};
FFS_SPOTBG_HD inline SpotBgPositions spotbg_positions(uint64_t n) { return SpotBgPositions{(n + 3) / 4, (n + 1) / 2, (3 * n + 1) / 4}; }

// What is decided from the counts alone, before any quartile: kSpotBgNoPixels, kSpotBgOverflow, or kSpotBgOk for "go on"
FFS_SPOTBG_HD inline uint32_t spotbg_status_of_counts(uint64_t n, uint64_t n_overflow) {
    if (n == 0) return kSpotBgNoPixels;
    if (4 * n_overflow > n) return kSpotBgOverflow;
    return kSpotBgOk;
}
// The upper fence q3 + 1.5 iqr reaches the end of the bins: the range is too small to tell the inliers from the tail
FFS_SPOTBG_HD inline bool spotbg_range_too_small(int32_t q1, int32_t q3) { return 2 * q3 + 3 * (q3 - q1) >= 2 * kSpotBgBins; }
// A value inside the fence q1 - 1.5 iqr .. q3 + 1.5 iqr (and inside the bins)
FFS_SPOTBG_HD inline bool spotbg_inlier(int32_t v, int32_t q1, int32_t q3) {
    const int32_t iqr3 = 3 * (q3 - q1);
    return 2 * q1 - iqr3 <= 2 * v && 2 * v <= 2 * q3 + iqr3 && v < kSpotBgBins;
}
// The last check, once the inliers are counted
FFS_SPOTBG_HD inline uint32_t spotbg_status_of_inliers(uint64_t n_inliers) { return n_inliers == 0 ? kSpotBgNoInliers : kSpotBgOk; }

// The eight integers of ffs_spot_background
struct SpotBgResult {
    uint32_t n_pixels = 0, n_overflow = 0;
    int32_t q1 = -1, median = -1, q3 = -1;
    uint32_t n_inliers = 0;
    uint64_t inlier_sum = 0;
    uint32_t status = kSpotBgNoPixels;
};

// The whole model over one histogram, bin after bin: what the kernel's wave computes a few bins per lane (the CPU check program's side).
inline SpotBgResult spotbg_from_histogram(const uint32_t* bins, uint32_t n_overflow) {
    SpotBgResult r;
    uint64_t n = n_overflow;
    for (int v = 0; v < kSpotBgBins; ++v) n += bins[v];
    r.n_pixels = (uint32_t)n;
    r.n_overflow = n_overflow;
    r.status = spotbg_status_of_counts(n, n_overflow);
    if (r.status != kSpotBgOk) return r;
    const SpotBgPositions p = spotbg_positions(n);
    uint64_t cum = 0;
    for (int v = 0; v < kSpotBgBins; ++v) {
        cum += bins[v];
        if (r.q1 < 0 && cum >= p.p25) r.q1 = v;
        if (r.median < 0 && cum >= p.p50) r.median = v;
        if (r.q3 < 0 && cum >= p.p75) r.q3 = v;
    }
    if (spotbg_range_too_small(r.q1, r.q3)) {
        r.status = kSpotBgRange;
        return r;
    }
    uint64_t cnt = 0, sum = 0;
    for (int v = 0; v < kSpotBgBins; ++v)
        if (spotbg_inlier(v, r.q1, r.q3)) {
            cnt += bins[v];
            sum += (uint64_t)v * bins[v];
        }
    r.status = spotbg_status_of_inliers(cnt);
    if (r.status == kSpotBgOk) {
        r.n_inliers = (uint32_t)cnt;
        r.inlier_sum = sum;
    }
    return r;
}

}  // namespace ffsamd
