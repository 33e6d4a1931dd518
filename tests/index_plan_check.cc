// index_plan_check.cc -- csrc/index_plan.hpp asked as a plain C++ program (tests/test_index_plan.py): every refusal with its text, the sizes
// of the device buffers and the launches' shapes per n_points.  Prints "ok" or the first failure.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "index_plan.hpp"

using namespace ffsamd;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        printf("FAILED: %s\n", what);
        ++failures;
    }
}
static void expect_text(const std::string& got, const char* want, const char* what) {
    if (got != want) {
        printf("FAILED: %s: got \"%s\", want \"%s\"\n", what, got.c_str(), want);
        ++failures;
    }
}

int main() {
    const double inf = INFINITY, nan = NAN;
    // n_points
    for (uint32_t n : {16u, 32u, 64u, 128u, 256u}) expect(index_points_refusal(n).empty(), "a power of two in 16 .. 256 is taken");
    for (uint32_t n : {0u, 1u, 8u, 24u, 100u, 255u, 257u, 512u, 0x80000000u})
        expect_text(index_points_refusal(n), ("n_points must be a power of two in 16 .. 256, got " + std::to_string(n)).c_str(), "n_points");
    // sizes
    expect(index_complex_bytes(256) == 268435456u && index_power_bytes(256) == 134217728u, "268 MB and 134 MB at 256");
    expect(index_complex_bytes(16) == 65536u && index_sums_entries(16) == 273u && index_sums_entries(256) == 65793u, "the sums");
    expect(index_tile_bytes(256) == 38912u && index_tile_bytes(256) <= 65536u && index_tile_bytes(16) == 2432u, "the LDS tile stays under 64 KB");
    for (uint32_t n : {16u, 32u, 64u, 128u, 256u}) {
        expect(index_fft_blocks(n) * kIndexSlab == n * n, "a pass's workgroups cover every line once");
        expect((size_t)index_select_blocks(n) * kIndexSelectPerBlock == index_voxels(n), "the selection's workgroups cover every voxel once");
        expect(index_list_blocks((uint32_t)index_voxels(n)) >= index_select_blocks(n), "the counts hold either count pass");
    }
    expect(index_select_blocks(16) == 1u && index_select_blocks(32) == 8u && index_select_blocks(256) == 4096u, "the selection's launch");
    expect(index_list_blocks(0) == 0u && index_list_blocks(1) == 1u && index_list_blocks(256) == 1u && index_list_blocks(257) == 2u, "the list passes' launch");
    expect(kIndexSlab * sizeof(IndexComplex) == 128u, "a slab row is 128 contiguous bytes");
    // the spot entries
    ShoeboxGeometry g{};
    const double D[9] = {1, 0, -200, 0, -1, 210, 0, 0, -150};
    memcpy(g.d_matrix, D, sizeof D);
    g.pixel_size_mm[0] = g.pixel_size_mm[1] = 0.172, g.wavelength = 1.0, g.s0[2] = -1.0, g.rot_axis[0] = 1.0, g.osc_width_deg = 0.25;
    double xyz[3] = {100, 200, 3}, o[3];
    expect(index_rlp_refusal(&g, xyz, 1, o, o, o).empty(), "a good geometry is taken");
    expect(index_rlp_refusal(&g, nullptr, 0, o, o, o).empty(), "no spots need no table");
    expect_text(index_rlp_refusal(nullptr, xyz, 1, o, o, o), "geometry, xyz_px, rlp, s1 or xyz_mm is NULL", "NULL geometry");
    expect_text(index_rlp_refusal(&g, nullptr, 1, o, o, o), "geometry, xyz_px, rlp, s1 or xyz_mm is NULL", "NULL xyz");
    expect_text(index_rlp_refusal(&g, xyz, 1, o, nullptr, o), "geometry, xyz_px, rlp, s1 or xyz_mm is NULL", "NULL s1");
    ShoeboxGeometry b = g;
    b.s0[1] = nan;
    expect_text(index_rlp_refusal(&b, xyz, 1, o, o, o), "the geometry has an entry that is not finite", "nan in the geometry");
    b = g, b.wavelength = 0.0;
    expect_text(index_rlp_refusal(&b, xyz, 1, o, o, o), "the geometry's wavelength and pixel sizes must be positive", "wavelength 0");
    b = g, b.pixel_size_mm[1] = -0.1;
    expect_text(index_rlp_refusal(&b, xyz, 1, o, o, o), "the geometry's wavelength and pixel sizes must be positive", "a negative pixel size");
    b = g, b.rot_axis[0] = 0.0;
    expect_text(index_rlp_refusal(&b, xyz, 1, o, o, o), "the geometry's rot_axis must not be zero", "a zero axis");
    b = g, b.d_matrix[8] = 0.0;
    expect_text(index_rlp_refusal(&b, xyz, 1, o, o, o), "the geometry's d_matrix is singular", "a singular d_matrix");
    double bad_xyz[3] = {1, inf, 2};
    expect_text(index_rlp_refusal(&g, bad_xyz, 1, o, o, o), "xyz_px has an entry that is not finite", "inf in xyz");
    // defaults
    double rlp[3] = {0.1, 0.02, -0.03}, dmin = 0.0, b_iso = 0.0;
    expect(index_defaults_refusal(rlp, 1, 45.0, 64, &dmin, &b_iso).empty() && index_defaults_refusal(nullptr, 0, 45.0, 64, &dmin, &b_iso).empty(), "defaults taken");
    expect_text(index_defaults_refusal(rlp, 1, 45.0, 64, nullptr, &b_iso), "rlp, dmin or b_iso is NULL", "NULL dmin");
    expect_text(index_defaults_refusal(nullptr, 1, 45.0, 64, &dmin, &b_iso), "rlp, dmin or b_iso is NULL", "NULL rlp");
    expect_text(index_defaults_refusal(rlp, 1, 45.0, 48, &dmin, &b_iso), "n_points must be a power of two in 16 .. 256, got 48", "48 points");
    for (double m : {0.0, -1.0, inf, nan}) expect_text(index_defaults_refusal(rlp, 1, m, 64, &dmin, &b_iso), "max_cell must be finite and positive", "max_cell");
    for (double d : {-1.0, inf, nan}) {
        double dd = d;
        expect_text(index_defaults_refusal(rlp, 1, 45.0, 64, &dd, &b_iso), "dmin must be finite and positive, or 0 to choose it", "dmin");
    }
    double bad_rlp[3] = {0.1, nan, 0.0};
    expect_text(index_defaults_refusal(bad_rlp, 1, 45.0, 64, &dmin, &b_iso), "rlp has an entry that is not finite", "nan in rlp");
    // the map and the grid
    expect(index_map_refusal(rlp, 1, 2.0, 10.0, 64).empty() && index_map_refusal(nullptr, 0, 2.0, 0.0, 16).empty(), "a map is taken");
    expect_text(index_map_refusal(nullptr, 1, 2.0, 10.0, 64), "rlp is NULL", "NULL rlp");
    expect_text(index_map_refusal(rlp, 1, 2.0, 10.0, 512), "n_points must be a power of two in 16 .. 256, got 512", "512 points");
    for (double d : {0.0, -1.0, inf, nan}) expect_text(index_map_refusal(rlp, 1, d, 10.0, 64), "dmin must be finite and positive", "dmin");
    for (double bi : {inf, nan}) expect_text(index_map_refusal(rlp, 1, 2.0, bi, 64), "b_iso must be finite", "b_iso");
    expect_text(index_map_refusal(bad_rlp, 1, 2.0, 10.0, 64), "rlp has an entry that is not finite", "nan in rlp");
    // a loaded grid
    std::vector<double> grid(4096, 1.0);
    expect(index_load_refusal(grid.data(), 16).empty(), "a grid is taken");
    expect_text(index_load_refusal(nullptr, 16), "power is NULL", "NULL power");
    expect_text(index_load_refusal(grid.data(), 20), "n_points must be a power of two in 16 .. 256, got 20", "20 points");
    grid[4095] = -inf;
    expect_text(index_load_refusal(grid.data(), 16), "power has an entry that is not finite", "inf in the grid");
    // the peaks
    expect(index_peaks_refusal(15.0, false, 10, false, 64).empty() && index_peaks_refusal(0.0, true, 0, false, 16).empty(), "peaks are taken");
    expect_text(index_peaks_refusal(15.0, false, 10, true, 64), "n is NULL, or out is NULL with cap > 0", "NULL n");
    expect_text(index_peaks_refusal(15.0, true, 1, false, 64), "n is NULL, or out is NULL with cap > 0", "NULL out");
    for (double r : {-1.0, inf, nan}) expect_text(index_peaks_refusal(r, false, 10, false, 64), "rmsd_cutoff must be finite and not negative", "rmsd_cutoff");
    expect_text(index_peaks_refusal(15.0, false, 10, false, 0), "no grid is resident (ffs_ctx_index_grid or ffs_ctx_index_load_grid first)", "no grid");
    // the vectors
    IndexPeak p{};
    p.n_voxels = 3, p.frac[0] = 0.1;
    expect(index_basis_refusal(&p, 1, 64, 2.0, 0.15, 3.0, 45.0, false, 4, false).empty() && index_basis_refusal(nullptr, 0, 64, 2.0, 0.15, 3.0, 45.0, true, 0, false).empty(), "vectors are taken");
    expect_text(index_basis_refusal(nullptr, 1, 64, 2.0, 0.15, 3.0, 45.0, false, 4, false), "peaks or n_out is NULL, or out is NULL with cap > 0", "NULL peaks");
    expect_text(index_basis_refusal(&p, 1, 64, 2.0, 0.15, 3.0, 45.0, true, 4, false), "peaks or n_out is NULL, or out is NULL with cap > 0", "NULL out");
    expect_text(index_basis_refusal(&p, 1, 64, 2.0, 0.15, 3.0, 45.0, false, 4, true), "peaks or n_out is NULL, or out is NULL with cap > 0", "NULL n_out");
    expect_text(index_basis_refusal(&p, 1, 8, 2.0, 0.15, 3.0, 45.0, false, 4, false), "n_points must be a power of two in 16 .. 256, got 8", "8 points");
    expect_text(index_basis_refusal(&p, 1, 64, 0.0, 0.15, 3.0, 45.0, false, 4, false), "dmin must be finite and positive", "dmin");
    expect_text(index_basis_refusal(&p, 1, 64, 2.0, 0.15, 3.0, nan, false, 4, false), "max_cell must be finite and positive", "max_cell");
    expect_text(index_basis_refusal(&p, 1, 64, 2.0, 0.15, -1.0, 45.0, false, 4, false), "min_cell must be finite and not negative", "min_cell");
    expect_text(index_basis_refusal(&p, 1, 64, 2.0, inf, 3.0, 45.0, false, 4, false), "peak_volume_cutoff must be finite and not negative", "peak_volume_cutoff");
    IndexPeak q = p;
    q.n_voxels = 0;
    expect_text(index_basis_refusal(&q, 1, 64, 2.0, 0.15, 3.0, 45.0, false, 4, false), "peak 0 has no voxels", "an empty peak");
    q = p, q.frac[2] = nan;
    expect_text(index_basis_refusal(&q, 1, 64, 2.0, 0.15, 3.0, 45.0, false, 4, false), "peak 0 has a frac that is not finite", "nan frac");
    if (failures == 0) printf("ok\n");
    return failures ? 1 : 0;
}
