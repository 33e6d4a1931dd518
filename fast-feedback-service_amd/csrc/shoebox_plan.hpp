// shoebox_plan.hpp -- what the host decides about a summation-integration job (ffs_ctx_shoebox_begin / ffs_stream_shoebox_fold, DESIGN.md
// section 3.8c): which shoebox tables are taken, which boxes a fold of images [a, b) meets, the list its launch receives and the bytes of
// device state a shoebox costs.  No HIP header: ffs_shoebox.hip acts on these decisions and a plain C++ test program
// (tests/shoebox_plan_check.cc) asks the same text.  The rule itself is shoebox_model.hpp's.
#pragma once
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "shoebox_model.hpp"

namespace ffsamd {

constexpr int32_t kShoeboxMaxSide = 1024;   // pixels a box may be wide and high
constexpr int32_t kShoeboxPad = 1024;       // how far outside the image a box may reach: it must meet [-pad, W + pad) x [-pad, H + pad)

// Device state per shoebox: the accumulators and the 256 bins of its background histogram
constexpr size_t shoebox_state_bytes() { return sizeof(ShoeboxAcc) + (size_t)kSpotBgBins * sizeof(uint32_t); }

inline bool shoebox_finite(double x) { return x - x == 0.0; }

// Why entry i of a table cannot be taken, or "" when it can
inline std::string shoebox_entry_refusal(const ShoeboxEntry& b, const double* s0, int W, int H) {
    if (!(b.x_min < b.x_max) || !(b.y_min < b.y_max) || !(b.z_min < b.z_max)) return "is empty or reversed (x_min < x_max, y_min < y_max, z_min < z_max are needed; the ranges are half-open)";
    if ((int64_t)b.x_max - b.x_min > kShoeboxMaxSide) return "is wider than " + std::to_string(kShoeboxMaxSide) + " pixels";
    if ((int64_t)b.y_max - b.y_min > kShoeboxMaxSide) return "is higher than " + std::to_string(kShoeboxMaxSide) + " pixels";
    if (b.x_max <= -kShoeboxPad || b.x_min >= W + kShoeboxPad || b.y_max <= -kShoeboxPad || b.y_min >= H + kShoeboxPad)
        return "lies outside the image padded by " + std::to_string(kShoeboxPad) + " pixels";
    if (!shoebox_finite(b.s1[0]) || !shoebox_finite(b.s1[1]) || !shoebox_finite(b.s1[2])) return "has an s1 that is not finite";
    if (!shoebox_finite(b.phi)) return "has a phi that is not finite";
    double c[3];
    shoebox_cross(b.s1, s0, c);
    const double n = sqrt(shoebox_dot(c, c));
    if (!shoebox_finite(n) || !(n > 0.0)) return "has an s1 parallel to s0 (or zero): cross(s1, s0) must not vanish";
    return "";
}

// The first entry of a table that cannot be taken: its index and the reason in `why`; -1 when every entry can
inline int64_t shoebox_table_refusal(const ShoeboxEntry* t, uint32_t n, const double* s0, int W, int H, std::string& why) {
    for (uint32_t i = 0; i < n; ++i) {
        why = shoebox_entry_refusal(t[i], s0, W, H);
        if (!why.empty()) return (int64_t)i;
    }
    return -1;
}

// Why a geometry or a pair of deltas or an algorithm cannot be taken, or ""
inline std::string shoebox_job_refusal(const ShoeboxGeometry& g, int algorithm, double delta_b, double delta_m) {
    if (algorithm != kShoeboxEllipsoid && algorithm != kShoeboxDials) return "unknown algorithm " + std::to_string(algorithm) + " (0: ellipsoid, 1: dials)";
    if (!shoebox_finite(delta_b) || !(delta_b > 0.0)) return "delta_b must be finite and positive";
    if (!shoebox_finite(delta_m) || !(delta_m > 0.0)) return "delta_m must be finite and positive";
    double v[20];   // (the struct is twenty doubles, one behind the other)
    memcpy(v, &g, sizeof v);
    for (int i = 0; i < 20; ++i)
        if (!shoebox_finite(v[i])) return "the geometry has an entry that is not finite";
    if (!(g.wavelength > 0.0) || !(g.pixel_size_mm[0] > 0.0) || !(g.pixel_size_mm[1] > 0.0)) return "the geometry's wavelength and pixel sizes must be positive";
    return "";
}
static_assert(sizeof(ShoeboxGeometry) == 20 * sizeof(double), "ShoeboxGeometry is twenty doubles");

// The boxes in the order of z_min, with the running maximum of z_max: a fold of images [a, b) meets the boxes with z_min < b && z_max > a.
// Those with z_min < b are a prefix of the order (binary search); the running maximum never falls, so the boxes ahead of the first position
// where it exceeds a all end at or before a (binary search again); what lies between is filtered by its own z_max.
struct ShoeboxIndex {
    std::vector<uint32_t> order;      // table indices, by z_min (ties: by index)
    std::vector<int32_t> z_min;       // of order[k]
    std::vector<int32_t> z_max;       // of order[k]
    std::vector<int32_t> run_max;     // max of z_max over order[0 .. k]

    void build(const ShoeboxEntry* t, uint32_t n) {
        order.resize(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return t[a].z_min < t[b].z_min; });
        z_min.resize(n), z_max.resize(n), run_max.resize(n);
        for (uint32_t k = 0; k < n; ++k) {
            z_min[k] = t[order[k]].z_min, z_max[k] = t[order[k]].z_max;
            run_max[k] = k ? std::max(run_max[k - 1], z_max[k]) : z_max[k];
        }
    }
    // The range [lo, hi) of positions a window [a, b) has to look at (what query() filters)
    void span(int64_t a, int64_t b, size_t& lo, size_t& hi) const {
        hi = (size_t)(std::lower_bound(z_min.begin(), z_min.end(), b, [](int32_t z, int64_t lim) { return (int64_t)z < lim; }) - z_min.begin());
        lo = (size_t)(std::upper_bound(run_max.begin(), run_max.begin() + (ptrdiff_t)hi, a, [](int64_t lim, int32_t z) { return lim < (int64_t)z; }) - run_max.begin());
    }
    // The list a launch receives: the table indices of the boxes images [a, b) meet, in the order of z_min
    void query(int64_t a, int64_t b, std::vector<uint32_t>& list) const {
        list.clear();
        if (a >= b) return;
        size_t lo, hi;
        span(a, b, lo, hi);
        for (size_t k = lo; k < hi; ++k)
            if ((int64_t)z_max[k] > a) list.push_back(order[k]);
    }
};

}  // namespace ffsamd
