// index_plan.hpp -- what the host decides about the indexer's basis-vector search (ffs_index_*, ffs_ctx_index_*):
// which calls are refused and why, the sizes of the device buffers per n_points and the launches' shapes.  No HIP header: ffs_index.hip acts
// on these decisions and a plain C++ test program (tests/index_plan_check.cc) asks the same text.  The rule itself is index_model.hpp's.
//
// Device memory a context keeps from its first index call at an n_points until it is destroyed (bytes, N = n_points):
//   the complex grid 16 N^3 and the power grid 8 N^3 (268 MB + 134 MB at 256), the line, plane and total sums 8 (N^2 + N + 1) twice,
//   the twiddle table 8 N; per call, grown when a call needs more: the (cell, weight) list 12 bytes an occupied cell, the selection's
//   counts and offsets 12 bytes a workgroup, and per SELECTED voxel 4 (list) + 4 (parent) + 4 (n_voxels) + 24 (sums) = 36 bytes, 56 bytes
//   a record fetched.  An all-equal grid at 256 selects 16.7 M voxels: 604 MB.
#pragma once
#include <string.h>

#include <string>

#include "index_model.hpp"
#include "predict_model.hpp"
#include "shoebox_plan.hpp"

namespace ffsamd {

static_assert(sizeof(IndexPeak) == 56 && sizeof(IndexGridStats) == 40 && sizeof(IndexVector) == 40 && sizeof(IndexComplex) == 16,
              "ffs_index_peak, ffs_index_grid_stats, ffs_index_vector");

constexpr uint32_t kIndexSlab = 8u;             // adjacent lines a workgroup of an FFT pass takes: 8 x 16 B = 128 contiguous bytes on the strided axes
constexpr uint32_t kIndexTilePitch = kIndexSlab + 1u;   // elements between two rows of the LDS tile (one of padding against bank conflicts)
constexpr int kIndexThreads = 256;
constexpr uint32_t kIndexSelectPerThread = 16u;   // consecutive voxels a lane of the selection examines
constexpr uint32_t kIndexSelectPerBlock = kIndexSelectPerThread * (uint32_t)kIndexThreads;   // 4096 = 16^3: every n_points is a multiple

inline size_t index_voxels(uint32_t n) { return (size_t)n * n * n; }
inline size_t index_complex_bytes(uint32_t n) { return index_voxels(n) * sizeof(IndexComplex); }
inline size_t index_power_bytes(uint32_t n) { return index_voxels(n) * sizeof(double); }
inline size_t index_sums_entries(uint32_t n) { return (size_t)n * n + n + 1u; }   // line sums | plane sums | the total
inline size_t index_tile_bytes(uint32_t n) { return ((size_t)n * kIndexTilePitch + n / 2u) * sizeof(IndexComplex); }   // the LDS tile and the twiddles
inline uint32_t index_fft_blocks(uint32_t n) { return n * n / kIndexSlab; }
inline uint32_t index_select_blocks(uint32_t n) { return (uint32_t)(index_voxels(n) / kIndexSelectPerBlock); }
inline uint32_t index_list_blocks(uint32_t n_selected) { return (n_selected + (uint32_t)kIndexThreads - 1u) / (uint32_t)kIndexThreads; }
static_assert(16u * 16u * 16u == kIndexSelectPerBlock, "the smallest grid is one workgroup of the selection");

inline std::string index_points_refusal(uint32_t n_points) {
    if (!index_points_ok(n_points)) return "n_points must be a power of two in 16 .. 256, got " + std::to_string(n_points);
    return "";
}
inline std::string index_finite_refusal(const double* v, size_t n, const char* what) {
    for (size_t i = 0; i < n; ++i)
        if (!shoebox_finite(v[i])) return std::string(what) + " has an entry that is not finite";
    return "";
}

inline std::string index_rlp_refusal(const ShoeboxGeometry* g, const double* xyz, uint32_t n, const double* rlp, const double* s1, const double* xyz_mm) {
    if (!g || (n > 0u && (!xyz || !rlp || !s1 || !xyz_mm))) return "geometry, xyz_px, rlp, s1 or xyz_mm is NULL";
    double v[20];
    memcpy(v, g, sizeof v);
    std::string why = index_finite_refusal(v, 20, "the geometry");
    if (!why.empty()) return why;
    if (!(g->wavelength > 0.0) || !(g->pixel_size_mm[0] > 0.0) || !(g->pixel_size_mm[1] > 0.0)) return "the geometry's wavelength and pixel sizes must be positive";
    if (!(shoebox_dot(g->rot_axis, g->rot_axis) > 0.0)) return "the geometry's rot_axis must not be zero";
    double inv[9];
    if (!predict_inverse(g->d_matrix, inv)) return "the geometry's d_matrix is singular";
    return index_finite_refusal(xyz, 3 * (size_t)n, "xyz_px");
}

inline std::string index_defaults_refusal(const double* rlp, uint32_t n, double max_cell, uint32_t n_points, const double* dmin, const double* b_iso) {
    if (!dmin || !b_iso || (!rlp && n > 0u)) return "rlp, dmin or b_iso is NULL";
    std::string why = index_points_refusal(n_points);
    if (!why.empty()) return why;
    if (!shoebox_finite(max_cell) || !(max_cell > 0.0)) return "max_cell must be finite and positive";
    if (!shoebox_finite(*dmin) || *dmin < 0.0) return "dmin must be finite and positive, or 0 to choose it";
    return index_finite_refusal(rlp, 3 * (size_t)n, "rlp");
}

// the arguments ffs_index_map and ffs_ctx_index_grid share
inline std::string index_map_refusal(const double* rlp, uint32_t n, double dmin, double b_iso, uint32_t n_points) {
    if (!rlp && n > 0u) return "rlp is NULL";
    std::string why = index_points_refusal(n_points);
    if (!why.empty()) return why;
    if (!shoebox_finite(dmin) || !(dmin > 0.0)) return "dmin must be finite and positive";
    if (!shoebox_finite(b_iso)) return "b_iso must be finite";
    return index_finite_refusal(rlp, 3 * (size_t)n, "rlp");
}

inline std::string index_load_refusal(const double* power, uint32_t n_points) {
    if (!power) return "power is NULL";
    std::string why = index_points_refusal(n_points);
    if (!why.empty()) return why;
    return index_finite_refusal(power, index_voxels(n_points), "power");
}

inline std::string index_peaks_refusal(double rmsd_cutoff, bool out_null, uint32_t cap, bool n_null, uint32_t resident_points) {
    if (n_null || (out_null && cap > 0u)) return "n is NULL, or out is NULL with cap > 0";
    if (!shoebox_finite(rmsd_cutoff) || rmsd_cutoff < 0.0) return "rmsd_cutoff must be finite and not negative";
    if (resident_points == 0u) return "no grid is resident (ffs_ctx_index_grid or ffs_ctx_index_load_grid first)";
    return "";
}

inline std::string index_basis_refusal(const IndexPeak* peaks, uint32_t n, uint32_t n_points, double dmin, double peak_volume_cutoff, double min_cell, double max_cell,
                                       bool out_null, uint32_t cap, bool n_out_null) {
    if ((!peaks && n > 0u) || n_out_null || (out_null && cap > 0u)) return "peaks or n_out is NULL, or out is NULL with cap > 0";
    std::string why = index_points_refusal(n_points);
    if (!why.empty()) return why;
    if (!shoebox_finite(dmin) || !(dmin > 0.0)) return "dmin must be finite and positive";
    if (!shoebox_finite(max_cell) || !(max_cell > 0.0)) return "max_cell must be finite and positive";
    if (!shoebox_finite(min_cell) || min_cell < 0.0) return "min_cell must be finite and not negative";
    if (!shoebox_finite(peak_volume_cutoff) || peak_volume_cutoff < 0.0) return "peak_volume_cutoff must be finite and not negative";
    for (uint32_t i = 0; i < n; ++i) {
        if (peaks[i].n_voxels == 0u) return "peak " + std::to_string(i) + " has no voxels";
        if (!index_finite_refusal(peaks[i].frac, 3, "a peak").empty()) return "peak " + std::to_string(i) + " has a frac that is not finite";
    }
    return "";
}

}  // namespace ffsamd
