// shoebox_geometry.hpp -- what spotfinder --integrate hands to ffs_ctx_shoebox_begin: the flat single-panel geometry that
// kabsch_space.hpp writes out (fast axis +x, slow axis -y, origin from the beam centre and the distance, s0 = (0, 0, -1/lambda), rotation
// axis (1, 0, 0)) as an ffs_scan_geometry, and a record of the --integrate file as an ffs_shoebox.  `ffs_hosttool shoeboxgeom` and
// `ffs_hosttool shoebox` call the same text, so a test can hold the driver to it.
//
// The file: raw little-endian records of 48 bytes -- three float64, the predicted centre x, y in pixels and z in images (z = 0 is the start
// of the scan's first image), then six int32, the half-open box x_min, x_max, y_min, y_max, z_min, z_max.
//   s1 = normalized(lab(x, y)) / lambda,  lab(x, y) = (x px_x - bx px_x, by px_y - y px_y, -distance)
//   phi = (osc_start + z * osc_width) * pi / 180
//   delta = n_sigma * sigma_deg * pi / 180
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "ffs_hip.h"
#include "kabsch_space.hpp"

namespace ffshost {

struct ShoeboxRecord {   // one record of the --integrate file
    double x, y, z;
    int32_t box[6];
};
static_assert(sizeof(ShoeboxRecord) == 48, "a record of the --integrate file is 48 bytes");

inline ffs_scan_geometry shoebox_flat_geometry(const KabschGeometry& g) {
    ffs_scan_geometry o{};
    const double D[9] = {1.0, 0.0, -g.beam_center_x_px * g.pixel_size_x_mm, 0.0, -1.0, g.beam_center_y_px * g.pixel_size_y_mm, 0.0, 0.0, -g.distance_mm};
    std::memcpy(o.d_matrix, D, sizeof D);
    o.pixel_size_mm[0] = g.pixel_size_x_mm, o.pixel_size_mm[1] = g.pixel_size_y_mm;
    o.wavelength = g.wavelength;
    o.s0[0] = 0.0, o.s0[1] = 0.0, o.s0[2] = -1.0 / g.wavelength;
    o.rot_axis[0] = 1.0, o.rot_axis[1] = 0.0, o.rot_axis[2] = 0.0;
    o.osc_start_deg = g.oscillation_start, o.osc_width_deg = g.oscillation_width;
    return o;
}

inline ffs_shoebox shoebox_from_record(const KabschGeometry& g, const ShoeboxRecord& r) {
    ffs_shoebox b{};
    const Vec3 s = normalized(lab_coord(g, r.x, r.y));
    b.s1[0] = s[0] / g.wavelength, b.s1[1] = s[1] / g.wavelength, b.s1[2] = s[2] / g.wavelength;
    b.phi = (g.oscillation_start + r.z * g.oscillation_width) * (M_PI / 180.0);
    b.x_min = r.box[0], b.x_max = r.box[1], b.y_min = r.box[2], b.y_max = r.box[3], b.z_min = r.box[4], b.z_max = r.box[5];
    return b;
}

inline double shoebox_delta(double n_sigma, double sigma_deg) { return n_sigma * sigma_deg * (M_PI / 180.0); }

// The summary line of a run: boxes, boxes with foreground, boxes with FFS_SHOEBOX_FG_INVALID, and background failures -- boxes with
// foreground whose background estimate was rejected (integrator.cc:1126)
inline std::string shoebox_summary_line(const ffs_shoebox_sum* sums, size_t n) {
    size_t n_fg = 0, n_invalid = 0, n_bg_failed = 0;
    for (size_t i = 0; i < n; ++i) {
        n_fg += sums[i].fg_count > 0;
        n_invalid += (sums[i].flags & FFS_SHOEBOX_FG_INVALID) != 0;
        n_bg_failed += sums[i].fg_count > 0 && sums[i].bg_status != 0;
    }
    return "shoeboxes: " + std::to_string(n) + " boxes, " + std::to_string(n_fg) + " with foreground, " + std::to_string(n_invalid) + " FG_INVALID, "
           + std::to_string(n_bg_failed) + " background failures";
}

inline std::vector<ShoeboxRecord> read_shoebox_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the shoebox file " + path);
    f.seekg(0, std::ios::end);
    const std::streamoff bytes = f.tellg();
    f.seekg(0);
    if (bytes < 0 || bytes % (std::streamoff)sizeof(ShoeboxRecord) != 0)
        throw std::runtime_error("the shoebox file " + path + " is not a whole number of 48-byte records (" + std::to_string((long long)bytes) + " bytes)");
    std::vector<ShoeboxRecord> recs((size_t)bytes / sizeof(ShoeboxRecord));
    if (!recs.empty()) f.read(reinterpret_cast<char*>(recs.data()), bytes);
    if (!f) throw std::runtime_error("short read of the shoebox file " + path);
    return recs;
}

}  // namespace ffshost
