// spot_background_glm_model.hpp -- the robust Poisson GLM background of a spot's ring (ffs_stream_spot_backgrounds_glm, DESIGN.md section
// 3.8b): the order of the status checks, the seed, the IRLS step and the two elementary functions it needs.  No HIP header: the kernel
// (kernels_spotbg.hpp), tools/ffs_hosttool.cc (spotbgglm) and a plain C++ test program (tests/spot_background_glm_check.cc) compile the same
// text, all three with -ffp-contract=off.
//
// The model is the constant robust Poisson GLM of Parkhurst et al. 2016 (J. Appl. Cryst. 49, 1912) as the reference's integrator runs it over
// a histogram of one-count bins and a counted tail (include/integrator/background.hpp, glm_constant_background): beta = log mu, Huber's psi
// with c = 1.345, at most 100 IRLS steps, tolerance 1e-3.  Two things are restated, neither changes what is computed in exact arithmetic:
//   The score from four integers.  psi_c is the identity strictly inside (-c, c) and -c / +c outside, so with j1 = floor(mu - c s) and
//   j2 = floor(mu + c s) the bins v <= j1 give -c, the bins v > j2 and the tail +c, the bins between (v - mu) / s.  With C and S the inclusive
//   prefix sums of count and of v * count: n_low = C(j1), n_in = C(j2) - C(j1), s_in = S(j2) - S(j1), n_high = N - n_low - n_in and
//   U = ((s_in - n_in mu) / s + c (n_high - n_low) - N epsi1) mu / s.  The integers are exact and know no order.
//   The probabilities by one recurrence.  t_0 = exp(-mu), t_k = t_{k-1} (mu / k), s_k = s_{k-1} + t_k up to k = j2 + 1: every pdf the model
//   needs is a term, every cdf a partial sum, a negative index gives 0.  No lgamma.
// Order of the checks: no pixels (1), fewer than 10 (5), too much in the tail (2, the integer form of spot_background_model.hpp), then
//   the ring whose counting pixels are all 0: OK with mean 0, beta = -inf and no step taken.  This departs from the reference, which walks
//   beta down some seventy steps until delta / beta rounds below the tolerance and returns a mean near 1e-33 whose digits are rounding
//   noise; 0 is the maximum-likelihood mean and the limit of the fit, and it is decided in integers;
// then the seed log(median or 1) and the loop, which ends in degenerate (6) when mu or s is not > 0, mu is not < 512, or b or delta is not
// finite; not converged (7) after 100 steps; degenerate (6) for beta outside (-300, 300).
// The bound mu < 512 is not the reference's.  It caps the recurrence at kSpotBgGlmMaxTerms terms, so no loop's length is decided by the data
// alone, and keeps exp(-mu) a normal number.  The bins end at 255 and at most a quarter of the ring is clipped at +c, so a fit the reference
// accepts does not get there (no case of tests/golden/spot_background_glm_ref.json that the reference calls valid ends in 6).
// Status 7 is reached: a ring of two levels far apart with the median on the lower one (51 pixels at 0 and 49 at 250) makes the step cycle,
// here and in the reference.  Status 6 was reached by no histogram tried (the cases of tests/spot_background_glm_cases.py and rings built
// to overshoot: bins 0 and 255 with a full quarter in the tail); it is kept, as status 4 of the Tukey model is, because the loop's bounds
// rest on it.  A beta at or below -700 counts as mu = 0 there: spotbg_glm_exp is not asked outside its range.
//
// Floating point.  Every operation below is one of + - * /, sqrt, floor and a conversion between an integer and a double: IEEE, correctly
// rounded, the same on the host and on the device.  exp and the seed's logarithm are therefore this header's own, built from those (libm's
// and the device library's are not correctly rounded and differ from each other); they are good to a few units in the last place, which is
// all the model needs -- what matters is that every compilation of this text gives the same bits.
#pragma once
#include <stdint.h>

#include "spot_background_model.hpp"

namespace ffsamd {

// FFS_SPOT_BG_* of ffs_hip.h, continued
constexpr uint32_t kSpotBgFewPixels = 5, kSpotBgDegenerate = 6, kSpotBgNotConverged = 7;

constexpr uint32_t kSpotBgGlmMinPixels = 10;
constexpr int kSpotBgGlmMaxIter = 100;
constexpr int kSpotBgGlmMaxTerms = 600;      // of the recurrence: j2 + 1 <= floor(512 + 1.345 sqrt(512)) + 1 = 543
constexpr double kSpotBgGlmC = 1.345;        // Huber's tuning constant
constexpr double kSpotBgGlmTolerance = 1e-3;
constexpr double kSpotBgGlmMaxMu = 512.0;

// ln 2 in two parts: the high part has 32 significant bits, so k * kLn2Hi is exact for |k| < 2^20
constexpr double kSpotBgLn2Hi = 0x1.62e42feep-1, kSpotBgLn2Lo = 0x1.a39ef35793c76p-33, kSpotBgInvLn2 = 0x1.71547652b82fep+0;

FFS_SPOTBG_HD inline bool spotbg_glm_finite(double x) { return x - x == 0.0; }

// exp(x) for x in -745 < x < 709 (the callers stay within -512 .. 300): x = k ln 2 + r with |r| <= 0.35, the Taylor polynomial of degree
// 13 in r (its remainder is below 5e-18), times 2^k by exact multiplications.
FFS_SPOTBG_HD inline double spotbg_glm_exp(double x) {
    const double kf = __builtin_floor(x * kSpotBgInvLn2 + 0.5);
    const double r = (x - kf * kSpotBgLn2Hi) - kf * kSpotBgLn2Lo;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    int32_t k = (int32_t)kf;
    double step = 2.0;
    if (k < 0) {
        k = -k;
        step = 0.5;
    }
    double scale = 1.0;   // 2^k for |k| < 1024 by squaring: every product is a power of two, exact
    for (int bit = 0; bit < 10; ++bit) {
        if ((k >> bit) & 1) scale *= step;
        if (bit < 9) step *= step;
    }
    return p * scale;
}

// log(m) for an integer m in 1 .. 255: m = 2^e f with f in (sqrt(1/2), sqrt 2], log f = 2 atanh z with z = (f - 1) / (f + 1), |z| < 0.172,
// the series up to z^23 (the next term is below 1e-19).  log(1) is exactly 0.
FFS_SPOTBG_HD inline double spotbg_glm_log_int(int32_t m) {
    double f = (double)m;
    int32_t e = 0;
    while (f > 0x1.6a09e667f3bcdp+0) {
        f *= 0.5;
        ++e;
    }
    const double z = (f - 1.0) / (f + 1.0), w = z * z;
    double q = 1.0 / 23.0;
    q = q * w + 1.0 / 21.0;
    q = q * w + 1.0 / 19.0;
    q = q * w + 1.0 / 17.0;
    q = q * w + 1.0 / 15.0;
    q = q * w + 1.0 / 13.0;
    q = q * w + 1.0 / 11.0;
    q = q * w + 1.0 / 9.0;
    q = q * w + 1.0 / 7.0;
    q = q * w + 1.0 / 5.0;
    q = q * w + 1.0 / 3.0;
    q = q * w + 1.0;
    const double ef = (double)e;
    return ef * kSpotBgLn2Hi + (ef * kSpotBgLn2Lo + 2.0 * z * q);
}

// What is decided from the counts alone: kSpotBgNoPixels, kSpotBgFewPixels, kSpotBgOverflow, or kSpotBgOk for "go on"
FFS_SPOTBG_HD inline uint32_t spotbg_glm_status_of_counts(uint64_t n, uint64_t n_overflow) {
    if (n == 0) return kSpotBgNoPixels;
    if (n < kSpotBgGlmMinPixels) return kSpotBgFewPixels;
    if (4 * n_overflow > n) return kSpotBgOverflow;
    return kSpotBgOk;
}
// 1-based position of the seed's median among n sorted values (the reference's 0-based n / 2); inside the bins once the tail holds at most
// n / 4 of n >= 10 values
FFS_SPOTBG_HD inline uint64_t spotbg_glm_median_position(uint64_t n) { return n / 2 + 1; }
// The ring with no finite beta: nothing in the tail, nothing above bin 0
FFS_SPOTBG_HD inline bool spotbg_glm_all_zero(uint64_t n, uint64_t n_overflow, uint64_t bin0) { return n_overflow == 0 && bin0 == n; }

// The five doubles and the status that a fit ends in
struct SpotBgGlmFit {
    double beta = 0.0, mean = 0.0;
    uint32_t n_iter = 0, status = kSpotBgOk;
};

// One IRLS step's expectation values over Poisson(mu), s = sqrt(mu), j1 <= j2 the two floors: the reference's p1 .. p10, epsi1 and epsi2
// (glm_expectation), with the probabilities from the one recurrence.  Holds five terms and three partial sums, no array.
struct SpotBgGlmExpectation {
    double epsi1, epsi2;
};
FFS_SPOTBG_HD inline SpotBgGlmExpectation spotbg_glm_expectation(double mu, double s, int32_t j1, int32_t j2) {
    double pdf_j1m1 = 0.0, pdf_j1 = 0.0, pdf_j2m1 = 0.0, pdf_j2 = 0.0, pdf_j2p1 = 0.0;   // p7, p1, p8, p2, p4
    double cdf_j1 = 0.0, cdf_j2m1 = 0.0, cdf_j2p1 = 0.0;                                 // p3, p9, p5
    double t = spotbg_glm_exp(-mu), sum = t;
    const int32_t last = j2 + 1 < kSpotBgGlmMaxTerms ? j2 + 1 : kSpotBgGlmMaxTerms - 1;
    for (int32_t k = 0;; ++k) {
        if (k == j1 - 1) pdf_j1m1 = t;
        if (k == j1) {
            pdf_j1 = t;
            cdf_j1 = sum;
        }
        if (k == j2 - 1) {
            pdf_j2m1 = t;
            cdf_j2m1 = sum;
        }
        if (k == j2) pdf_j2 = t;
        if (k == j2 + 1) {
            pdf_j2p1 = t;
            cdf_j2p1 = sum;
        }
        if (k >= last) break;
        t = t * (mu / (double)(k + 1));
        sum = sum + t;
    }
    const double c = kSpotBgGlmC;
    const double p6 = 1.0 - cdf_j2p1 + pdf_j2p1;
    const double p10 = cdf_j2m1 - cdf_j1 + pdf_j1;
    SpotBgGlmExpectation e;
    e.epsi1 = c * (p6 - cdf_j1) + (mu / s) * (pdf_j1 - pdf_j2);
    e.epsi2 = c * (pdf_j1 + pdf_j2) + (mu * mu / (s * s * s)) * (p10 / mu + pdf_j1m1 - pdf_j1 - pdf_j2m1 + pdf_j2);
    return e;
}

// The seed and the loop, once the counts have said "go on" and the ring is not all zero.  `tables` answers count(j) = C(j) and sum(j) = S(j)
// as uint64_t for j in -1 .. 255 (0 for -1): arrays on the CPU, LDS in the kernel.  n is the ring's N, median the seed's bin.
template <typename Tables>
FFS_SPOTBG_HD inline SpotBgGlmFit spotbg_glm_fit(uint64_t n, int32_t median, const Tables& tables) {
    SpotBgGlmFit fit;
    const double c = kSpotBgGlmC, nf = (double)n;
    double beta = spotbg_glm_log_int(median > 0 ? median : 1);
    int iter = 0;
    for (; iter < kSpotBgGlmMaxIter; ++iter) {
        fit.beta = beta;
        fit.n_iter = (uint32_t)iter;
        if (!(beta > -700.0 && beta < 700.0)) {   // (outside the range of spotbg_glm_exp; mu would be 0 or beyond 512)
            fit.status = kSpotBgDegenerate;
            return fit;
        }
        const double mu = spotbg_glm_exp(beta), s = __builtin_sqrt(mu);
        if (!(mu > 0.0) || !(s > 0.0) || !(mu < kSpotBgGlmMaxMu)) {
            fit.status = kSpotBgDegenerate;
            return fit;
        }
        int32_t j1 = (int32_t)__builtin_floor(mu - c * s), j2 = (int32_t)__builtin_floor(mu + c * s);
        const SpotBgGlmExpectation e = spotbg_glm_expectation(mu, s, j1, j2);
        const double b = e.epsi2 * mu * mu / s;
        j1 = j1 < -1 ? -1 : j1 > kSpotBgBins - 1 ? kSpotBgBins - 1 : j1;
        j2 = j2 < -1 ? -1 : j2 > kSpotBgBins - 1 ? kSpotBgBins - 1 : j2;
        const uint64_t c1 = tables.count(j1), c2 = tables.count(j2), s1 = tables.sum(j1), s2 = tables.sum(j2);
        const uint64_t n_low = c1, n_in = c2 - c1, s_in = s2 - s1, n_high = n - n_low - n_in;
        const double clipped = (double)((int64_t)n_high - (int64_t)n_low);
        const double inside = ((double)s_in - (double)n_in * mu) / s;
        const double u = ((inside + c * clipped) - nf * e.epsi1) * mu / s;
        const double delta = u / (nf * b);
        if (!spotbg_glm_finite(b) || !spotbg_glm_finite(delta)) {
            fit.status = kSpotBgDegenerate;
            return fit;
        }
        const double d2 = delta * delta, b2 = beta * beta;
        beta = beta + delta;
        fit.beta = beta;
        fit.n_iter = (uint32_t)(iter + 1);
        if (__builtin_sqrt(d2 / (b2 > 1e-10 ? b2 : 1e-10)) < kSpotBgGlmTolerance) break;
    }
    if (iter >= kSpotBgGlmMaxIter) {
        fit.status = kSpotBgNotConverged;
        return fit;
    }
    if (!(beta > -300.0 && beta < 300.0)) {
        fit.status = kSpotBgDegenerate;
        return fit;
    }
    fit.mean = spotbg_glm_exp(beta);
    return fit;
}

// The fields of ffs_spot_background_glm
struct SpotBgGlmResult {
    uint32_t n_pixels = 0, n_overflow = 0;
    int32_t median = -1;
    uint32_t n_iter = 0;
    uint32_t status = kSpotBgNoPixels;
    double beta = 0.0, mean = 0.0;
};

// The prefix tables of a whole histogram on the CPU
struct SpotBgGlmHostTables {
    uint64_t c[kSpotBgBins], s[kSpotBgBins];
    uint64_t count(int32_t j) const { return j < 0 ? 0 : c[j]; }
    uint64_t sum(int32_t j) const { return j < 0 ? 0 : s[j]; }
};

// The whole model over one histogram, bin after bin: what the kernel's wave computes a few bins per lane (the CPU side)
inline SpotBgGlmResult spotbg_glm_from_histogram(const uint32_t* bins, uint32_t n_overflow) {
    SpotBgGlmResult r;
    SpotBgGlmHostTables t;
    uint64_t cum = 0, wsum = 0;
    for (int v = 0; v < kSpotBgBins; ++v) {
        cum += bins[v];
        wsum += (uint64_t)v * bins[v];
        t.c[v] = cum;
        t.s[v] = wsum;
    }
    const uint64_t n = cum + n_overflow;
    r.n_pixels = (uint32_t)n;
    r.n_overflow = n_overflow;
    r.status = spotbg_glm_status_of_counts(n, n_overflow);
    if (r.status != kSpotBgOk) return r;
    const uint64_t pos = spotbg_glm_median_position(n);
    for (int v = 0; v < kSpotBgBins && r.median < 0; ++v)
        if (t.c[v] >= pos) r.median = v;
    if (spotbg_glm_all_zero(n, n_overflow, bins[0])) {
        r.beta = -__builtin_inf();
        return r;
    }
    const SpotBgGlmFit fit = spotbg_glm_fit(n, r.median, t);
    r.beta = fit.beta;
    r.mean = fit.mean;
    r.n_iter = fit.n_iter;
    r.status = fit.status;
    return r;
}

}  // namespace ffsamd
