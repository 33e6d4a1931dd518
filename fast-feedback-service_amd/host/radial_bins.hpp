// radial_bins.hpp -- the bin map `spotfinder --radial-bins N` hands to ffs_ctx_set_radial_bins: N resolution shells of equal width in
// 1/d^2, from 0 to the largest 1/d^2 of any pixel centre.  Host only, no HIP, float64 throughout (the library never computes a
// resolution: ffs_hip.h); compiled on its own by tests/radial_bins_check.cc.  The geometry is the resolution mask's (kernels_mask.hpp,
// masking.cu:37-73): a flat detector normal to the beam, pixel centres at (x + 0.5, y + 0.5), d = wavelength / (2 sin(atan(r / D) / 2)).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ffshost {

struct RadialGeometry {
    double wavelength = 0;                            // A
    double distance = 0;                              // m
    double beam_center_x = 0, beam_center_y = 0;      // px
    double pixel_size_x = 0, pixel_size_y = 0;        // m
};

// 1/d^2 (A^-2) at the centre of pixel (x, y): increases with the distance from the beam centre
inline double radial_inv_d2(const RadialGeometry& g, uint32_t x, uint32_t y) {
    const double dx = (((double)x + 0.5) - g.beam_center_x) * g.pixel_size_x;
    const double dy = (((double)y + 0.5) - g.beam_center_y) * g.pixel_size_y;
    const double r = std::sqrt(dx * dx + dy * dy);
    const double s = 2.0 * std::sin(0.5 * std::atan(r / g.distance)) / g.wavelength;
    return s * s;
}

struct RadialBins {
    uint32_t n_bins = 0;
    std::vector<uint16_t> bin_of_pixel;   // W * H, row-major
    double inv_d2_max = 0;                // the largest 1/d^2 of any pixel centre: the outer edge of shell n_bins - 1
    // d (A) at the lower edge of shell k in 1/d^2, k = 0 .. n_bins: infinity first, then decreasing
    double d_edge(uint32_t k) const { return k == 0 ? INFINITY : 1.0 / std::sqrt(inv_d2_max * (double)k / (double)n_bins); }
};

// Shell of a pixel: floor(N * v / v_max), a pixel exactly on the last edge (the one furthest out) in shell N - 1.  Non-decreasing in v.
inline RadialBins radial_bins(const RadialGeometry& g, uint32_t width, uint32_t height, uint32_t n_bins) {
    RadialBins out;
    out.n_bins = n_bins;
    out.bin_of_pixel.assign((size_t)width * height, 0);
    std::vector<double> v((size_t)width * height);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const double s = radial_inv_d2(g, x, y);
            v[(size_t)y * width + x] = s;
            out.inv_d2_max = std::max(out.inv_d2_max, s);
        }
    if (!(out.inv_d2_max > 0)) return out;   // (one pixel on the beam centre: everything in shell 0)
    for (size_t i = 0; i < v.size(); ++i) {
        const double k = std::floor(v[i] / out.inv_d2_max * (double)n_bins);
        out.bin_of_pixel[i] = (uint16_t)std::min<double>(k, (double)(n_bins - 1));
    }
    return out;
}

}  // namespace ffshost
