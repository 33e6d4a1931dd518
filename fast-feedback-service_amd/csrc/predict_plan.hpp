// predict_plan.hpp -- what the host decides about a scan prediction (ffs_ctx_predict / ffs_predict_scan_settings):
// which calls are refused and why, the candidate box, the constants every candidate reads, the scan-point settings (the one place libm's
// cos and sin enter) and the launch's shape.  No HIP header: ffs_predict.hip acts on these decisions, tools/ffs_hosttool.cc runs the same
// rule on the CPU through predict_all, and a plain C++ test program (tests/predict_plan_check.cc) asks the same text.  The rule itself is
// predict_model.hpp's.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "predict_model.hpp"
#include "shoebox_plan.hpp"

namespace ffsamd {

static_assert(kPredictMaxSide == kShoeboxMaxSide && kPredictPad == kShoeboxPad, "kPredictBoxRefused follows ffs_ctx_shoebox_begin's limits");
static_assert(sizeof(PredictCrystal) == 80 && sizeof(PredictRecord) == 96, "ffs_crystal and ffs_prediction");

constexpr uint32_t kPredictMaxImages = 65535u;
constexpr int64_t kPredictMaxCandidates = 0x7FFFFFFFll;
constexpr int kPredictThreads = 256;   // candidates a workgroup of either pass takes

// Why a call cannot be taken, or "" when it can; on "" `u` holds the constants of the call.  W, H: the context's image.
inline std::string predict_refusal(const ShoeboxGeometry& g, const PredictCrystal& x, uint32_t n_images, double dmin, double delta_b, double delta_m, int W, int H,
                                   PredictSetup& u) {
    double v[20];
    memcpy(v, &g, sizeof v);
    for (int i = 0; i < 20; ++i)
        if (!shoebox_finite(v[i])) return "the geometry has an entry that is not finite";
    for (int i = 0; i < 9; ++i)
        if (!shoebox_finite(x.a_matrix[i])) return "the crystal's a_matrix has an entry that is not finite";
    if (!shoebox_finite(dmin) || !(dmin > 0.0)) return "dmin must be finite and positive";
    if (!shoebox_finite(delta_b) || !(delta_b > 0.0)) return "delta_b must be finite and positive";
    if (!shoebox_finite(delta_m) || !(delta_m > 0.0)) return "delta_m must be finite and positive";
    if (!(g.wavelength > 0.0) || !(g.pixel_size_mm[0] > 0.0) || !(g.pixel_size_mm[1] > 0.0)) return "the geometry's wavelength and pixel sizes must be positive";
    if (g.osc_width_deg == 0.0) return "the geometry's osc_width_deg must not be 0";
    if (n_images == 0u || n_images > kPredictMaxImages) return "n_images must be 1 .. " + std::to_string(kPredictMaxImages) + ", got " + std::to_string(n_images);
    if (x.centring < 0 || x.centring >= kPredictCentrings) return "unknown centring " + std::to_string(x.centring) + " (0 P, 1 I, 2 F, 3 A, 4 B, 5 C, 6 R)";
    if (!(shoebox_dot(g.rot_axis, g.rot_axis) > 0.0) || !(shoebox_dot(g.s0, g.s0) > 0.0)) return "the geometry's rot_axis and s0 must not be zero";
    PredictSetup o{};
    if (!predict_inverse(g.d_matrix, o.d_inv)) return "the geometry's d_matrix is singular";
    double real[9];
    if (!predict_inverse(x.a_matrix, real)) return "the crystal's a_matrix is singular";
    int64_t total = 1;
    for (int i = 0; i < 3; ++i) {
        const double q = floor(sqrt(shoebox_dot(real + 3 * i, real + 3 * i)) / dmin);
        if (!(q < (double)kPredictMaxCandidates)) return "the candidate box has more than 2^31 - 1 indices";
        o.h_max[i] = (int32_t)q + 1;
        total *= 2 * (int64_t)o.h_max[i] + 1;
        if (total > kPredictMaxCandidates) return "the candidate box has more than 2^31 - 1 indices";
    }
    o.n_candidates = (uint32_t)total;
    for (int i = 0; i < 3; ++i) o.s0[i] = g.s0[i], o.rot_axis[i] = g.rot_axis[i];
    o.s0s0 = shoebox_dot(g.s0, g.s0);
    o.res_limit = 1.0 / (dmin * dmin);
    o.res_leave = o.res_limit * kPredictLeaveMargin;
    o.px[0] = g.pixel_size_mm[0], o.px[1] = g.pixel_size_mm[1];
    o.osc_start = g.osc_start_deg, o.osc_width = g.osc_width_deg;
    o.delta_b = delta_b, o.delta_m = delta_m;
    o.centring = x.centring;
    o.W = W, o.H = H;
    o.n_images = n_images;
    u = o;
    return "";
}

// Why the scan-point settings cannot be computed, or ""
inline std::string predict_settings_refusal(const ShoeboxGeometry& g, const PredictCrystal& x, uint32_t n_images) {
    double v[20];
    memcpy(v, &g, sizeof v);
    for (int i = 0; i < 20; ++i)
        if (!shoebox_finite(v[i])) return "the geometry has an entry that is not finite";
    for (int i = 0; i < 9; ++i)
        if (!shoebox_finite(x.a_matrix[i])) return "the crystal's a_matrix has an entry that is not finite";
    if (n_images == 0u || n_images > kPredictMaxImages) return "n_images must be 1 .. " + std::to_string(kPredictMaxImages) + ", got " + std::to_string(n_images);
    if (!(shoebox_dot(g.rot_axis, g.rot_axis) > 0.0)) return "the geometry's rot_axis and s0 must not be zero";
    return "";
}

// A_k for k = 0 .. n_images into out[(n_images + 1) * 9]: cos and sin from libm once per scan point, everything else predict_model.hpp's
inline void predict_scan_settings(const ShoeboxGeometry& g, const double* A, uint32_t n_images, double* out) {
    double u[3] = {g.rot_axis[0], g.rot_axis[1], g.rot_axis[2]};
    shoebox_normalize(u);
    // libm's cos and sin themselves, in every build: a compiler that sees both calls on one argument may merge them into sincos(), whose
    // results differ from theirs in the last place now and then (three of 3601 scan points of 0.1 degrees), and the library, the host tool
    // and the check programs are built by different compilers.  Calls through volatile pointers are not merged.
    double (*volatile libm_cos)(double) = cos;
    double (*volatile libm_sin)(double) = sin;
    for (uint32_t k = 0; k <= n_images; ++k) {
        const double phi = predict_scan_point_deg(g.osc_start_deg, g.osc_width_deg, k) * kShoeboxDegToRad;
        predict_scan_setting(u, A, libm_cos(phi), libm_sin(phi), out + 9 * (size_t)k);
    }
}

// The whole rule on the CPU, candidate by candidate: the records in the order of candidate number and image (tools/ffs_hosttool.cc,
// tests/predict_check.cc)
inline void predict_all(const PredictSetup& u, const double* settings, std::vector<PredictRecord>& out) {
    for (uint32_t q = 0; q < u.n_candidates; ++q) {
        int32_t h, k, l;
        predict_index_of(u.h_max, q, h, k, l);
        predict_walk(u, settings, h, k, l, [&](uint32_t n, const PredictRay& ray) { out.push_back(predict_record(u, h, k, l, n, ray)); });
    }
}

inline uint32_t predict_blocks(uint32_t n_candidates) { return (n_candidates + (uint32_t)kPredictThreads - 1u) / (uint32_t)kPredictThreads; }

}  // namespace ffsamd
