// radial_threshold_model.hpp -- the decisions of the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE) as plain
// arithmetic: the quartile positions, the order of the status checks and the cutoff with its two separately rounded float64 operations.
// No HIP header: the kernel (kernels_radthr.hpp, k_radthr_cut) and a plain C++ test program (tests/radial_threshold_check.cc) compile the
// same text.  The reference has no counterpart (its two algorithms are dispersion and dispersion_extended, spotfinder/spotfinder.cc:338-342);
// the model follows DIALS's radial_profile threshold -- median + n_iqr x IQR per shell -- over a histogram, and claims no parity with it.
//
// The histogram of a (frame, shell) has kRadThrCounters counters: one-count bins for the values 0 .. 255 and a tail that is counted, not
// resolved.  Order of the checks: no pixels (1); the position of q3 lies in the tail (2); else the three quartiles lie inside the bins (0).
#pragma once
#include <stdint.h>

#include "spot_background_model.hpp"

namespace ffsamd {

constexpr uint32_t kRadThrMaxBins = 128;      // shells: 128 x 257 x 4 B = 128.5 KiB of LDS a workgroup, inside a CU's 160 KiB
constexpr int kRadThrValues = 256;            // one-count bins: the values 0 .. 255; a value at or above goes to the tail
constexpr int kRadThrCounters = kRadThrValues + 1;
constexpr double kRadThrMaxNIqr = 1048576.0;  // n_iqr <= 2^20: 255 + 2^20 x 255 < 2^32, the cutoff is a uint32
constexpr uint32_t kRadThrNever = 0xFFFFFFFFu;   // the cutoff the strong kernel reads for a shell whose status is not 0: no pixel passes

// FFS_RADIAL_THR_* of ffs_hip.h
constexpr uint32_t kRadThrOk = 0, kRadThrEmpty = 1, kRadThrOverflow = 2;

// What is decided from the counts alone: kRadThrEmpty, kRadThrOverflow (the value at the third position is >= 256), or kRadThrOk
FFS_SPOTBG_HD inline uint32_t radthr_status_of_counts(uint64_t n, uint64_t n_overflow) {
    if (n == 0) return kRadThrEmpty;
    if (spotbg_positions(n).p75 > n - n_overflow) return kRadThrOverflow;
    return kRadThrOk;
}

// floor(median + n_iqr x iqr) in float64: the product and the sum each rounded to nearest on their own, never fused.  0 <= median, iqr <= 255
// and 0 <= n_iqr <= 2^20, so the sum is below 2^32 and the conversion truncates a non-negative number.
FFS_SPOTBG_HD inline uint32_t radthr_cutoff(int32_t median, int32_t iqr, double n_iqr) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__dadd_rn((double)median, __dmul_rn(n_iqr, (double)iqr));
#else
    volatile double product = n_iqr * (double)iqr;   // (volatile: the compiler may not contract the two into a fused multiply-add)
    const double t = (double)median + product;
    return (uint32_t)t;
#endif
}

// The seven integers of ffs_radial_shell (its eighth word is reserved)
struct RadThrShell {
    uint32_t n_pixels = 0, n_overflow = 0;
    int32_t q1 = -1, median = -1, q3 = -1;
    uint32_t cutoff = 0, status = kRadThrEmpty;
};

// The whole model over one histogram of kRadThrCounters counters, bin after bin: what the kernel's wave computes four bins per lane (the CPU
// check program's side).
inline RadThrShell radthr_from_histogram(const uint32_t* counters, double n_iqr) {
    RadThrShell r;
    uint64_t n = counters[kRadThrValues];
    for (int v = 0; v < kRadThrValues; ++v) n += counters[v];
    r.n_pixels = (uint32_t)n;
    r.n_overflow = counters[kRadThrValues];
    r.status = radthr_status_of_counts(n, r.n_overflow);
    if (r.status != kRadThrOk) return r;
    const SpotBgPositions p = spotbg_positions(n);
    uint64_t cum = 0;
    for (int v = 0; v < kRadThrValues; ++v) {
        cum += counters[v];
        if (r.q1 < 0 && cum >= p.p25) r.q1 = v;
        if (r.median < 0 && cum >= p.p50) r.median = v;
        if (r.q3 < 0 && cum >= p.p75) r.q3 = v;
    }
    r.cutoff = radthr_cutoff(r.median, r.q3 - r.q1, n_iqr);
    return r;
}

}  // namespace ffsamd
