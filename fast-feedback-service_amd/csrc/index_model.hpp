// index_model.hpp -- the rule of the indexer's basis-vector search (ffs_index_*, ffs_ctx_index_*): spot centres to
// reciprocal-lattice points, their map on a grid, the 3D FFT, the grid's statistics, the connected peaks and the candidate basis vectors.
// No HIP header: the kernels (kernels_index.hpp), the library's host side, tools/ffs_hosttool.cc and a plain C++ test program
// (tests/index_check.cc) compile the same text, all with -ffp-contract=off.
//
// It restates the reference's chain baseline/indexer/indexer.cc:171-245 (xyz_to_rlp -> fft3d -> flood_fill -> flood_fill_filter ->
// peaks_to_rlvs) for ONE FLAT PANEL WITHOUT PARALLAX CORRECTION AND IDENTITY SETTING AND SAMPLE ROTATIONS, the assumptions ffs_scan_geometry
// carries.  No parity with the reference's binaries is claimed: THIS TEXT IS THE CONTRACT.  Every operation is an IEEE float64 + - * / sqrt,
// a comparison or a conversion, each rounded on its own, in the order written.  libm enters on the HOST only (cos, sin, exp, log, acos,
// round), through volatile pointers so that no compiler folds or merges a call; the device evaluates none of them.
//
//   Spot -> rlp (xyz_to_rlp.cc:46-109), host: x = x_px * px[0], y = y_px * px[1]; L_i = (D[3i]*x + D[3i+1]*y) + D[3i+2];
//       s1 = normalized(L) / wavelength; angle = (osc_start + z * osc_width) * (M_PI / 180.0), z in images from the scan's first (the z of
//       ffs_prediction); S = s1 - s0, u = normalized(rot_axis), c = cos(-1.0 * angle), s = sin(-1.0 * angle), d = dot(u, S), X = cross(u, S):
//       rlp_i = (S_i * c + (u_i * d) * (1.0 - c)) + s * X_i.
//   Defaults (indexer.cc:184-206), host: dmin = max(5.0 * max_cell / n_points, min_i 1.0 / sqrt(dot(rlp_i, rlp_i))) when none is given;
//       b_iso = (-4.0 * (dmin * dmin)) * log(0.05).
//   Map (fft3d.cc:37-91), host: rlgrid = 2.0 / (dmin * n_points), q = 1.0 / rlgrid; len = sqrt(dot(v, v)); not used when 1.0 / len < dmin;
//       c_j = (int)round(v_j * q) + n_points / 2; not used when a c_j is outside 0 .. n_points - 1; weight = exp(((-b_iso * len) * len) / 4.0),
//       or 1 when b_iso == 0; cell = c_2 + N c_1 + N^2 c_0.  Where several spots meet in a cell the one with the HIGHEST SPOT NUMBER gives the
//       weight (the reference's last write wins, stated so that no scatter order can change it).
//   FFT: forward (exponent -2 pi i), complex float64, unnormalised, radix 2, decimation in time, in place, N = 2^m a power of two 16 .. 256.
//       Twiddle table, host: w[k] = (cos(a), -sin(a)), a = M_PI * ((double)(2 k) / (double)N), k = 0 .. N/2 - 1.
//       One line: element p moves to position bitrev_m(p); then stages s = 0 .. m - 1 with half = 2^s, and in a stage the butterflies
//       b = 0 .. N/2 - 1, independent of one another: j = b mod half, i0 = (b / half) * 2 half + j, i1 = i0 + half, w = w[j * (N / (2 half))],
//       t.re = w.re * x[i1].re - w.im * x[i1].im, t.im = w.re * x[i1].im + w.im * x[i1].re  (four products, one difference, one sum),
//       x[i1] = x[i0] - t, x[i0] = x[i0] + t.
//       The axes: every line along grid axis 0 (the slowest, stride N^2), then along axis 1 (stride N), then along axis 2 (contiguous).
//       power = re * re of the result.  (Lines that hold no spot are transformed like every other: the all-zero shortcut is not taken.)
//   Tree sum of n = 2^k values: for stride = n/2, n/4 .. 1: v[i] = v[i] + v[i + stride] for i < stride; the sum is v[0].
//   Grid statistics (flood_fill.cc:38-49): sum = the tree sum of each x-line (axis 2), then of a plane's N line sums, then of the N plane
//       sums; mean = sum / (double)N^3; ssq = the same tree over (v - mean) * (v - mean); rmsd = sqrt(ssq / (double)N^3);
//       cutoff = rmsd_cutoff * rmsd; a voxel is selected when v >= cutoff.
//   Components (flood_fill.cc:59-147): six-connected, periodic in all three axes; a component's number (root) is its smallest flat index.
//       Per component n_voxels and, per axis, the integer sum of c_root + ((c - c_root + N/2) mod N) - N/2; frac_j = (double)sum_j /
//       (double)(n_voxels * N), j = 0 the slowest grid axis (the order of the rlp's components).  Records in ascending order of root.
//       DEPARTURES: the reference unwraps along the fill's path from a seed its hash map chooses and orders peaks by that map's iteration,
//       both implementation-defined; ours agree with it modulo 1 whenever a component reaches less than N/2 from its root.
//   Filter (flood_fill.cc:158-192), host: volumes sorted; Q1 at n/4, Q3 at 3n/4, cut = 5 (Q3 - Q1) + Q3; max = the largest volume <= cut;
//       peak_cutoff = (int)(peak_volume_cutoff * max); a peak is dropped when volume <= peak_cutoff.
//   Basis vectors (peaks_to_rlvs.cc:74-186), host: val > 0.5 -> val - 1.0, times n_points * dmin / 2.0; kept when min_cell < length <
//       2 max_cell; grouping at 10 % length and 5 degrees against each group's mean (inverse pairs negated), group mean and maximum volume;
//       stable sort by volume (descending), then by length (ascending); a site is dropped when it is an approximate integer multiple
//       (0.2, 5 degrees) of a kept site of larger volume; a final stable sort by volume.  angle(a, b): n = dot(a, b) / (|a| * |b|), 0 when
//       |n - 1| < 1e-6, 180 when |n + 1| < 1e-6, else acos(n) * 180.0 / M_PI.  An empty peak list gives an empty result.
#pragma once
#include <math.h>
#include <stdint.h>

#include "shoebox_model.hpp"

#include <algorithm>
#include <utility>
#include <vector>

namespace ffsamd {

constexpr uint32_t kIndexMinPoints = 16u, kIndexMaxPoints = 256u;
constexpr uint32_t kIndexNotUsed = 0xFFFFFFFFu;
constexpr double kIndexRmsdCutoff = 15.0, kIndexPeakVolumeCutoff = 0.15, kIndexMinCell = 3.0;   // the reference's constants (indexer.cc:234-245)

struct IndexComplex {
    double re, im;
};
struct IndexPeak {        // = ffs_index_peak, 56 bytes
    uint32_t root, n_voxels;
    int64_t sum[3];
    double frac[3];
};
struct IndexGridStats {   // = ffs_index_grid_stats, 40 bytes
    double sum, mean, rmsd, cutoff;
    uint32_t n_selected, n_peaks;
};
struct IndexVector {      // = ffs_index_vector, 40 bytes
    double v[3], length;
    uint32_t volume, reserved;
};

FFS_SPOTBG_HD inline bool index_points_ok(uint32_t n) { return n >= kIndexMinPoints && n <= kIndexMaxPoints && (n & (n - 1u)) == 0u; }
FFS_SPOTBG_HD inline uint32_t index_log2(uint32_t n) {
    uint32_t m = 0u;
    while ((1u << m) < n) ++m;
    return m;
}
FFS_SPOTBG_HD inline uint32_t index_bitrev(uint32_t p, uint32_t m) {
    uint32_t r = 0u;
    for (uint32_t i = 0u; i < m; ++i) r |= ((p >> i) & 1u) << (m - 1u - i);
    return r;
}

// ---- the FFT's schedule ------------------------------------------------------------------------------------------------------------------
// Butterfly b of stage s on a line of N = 2^m elements: the two elements and the twiddle entry
struct IndexButterfly {
    uint32_t i0, i1, w;
};
FFS_SPOTBG_HD inline IndexButterfly index_butterfly(uint32_t m, uint32_t s, uint32_t b) {
    const uint32_t half = 1u << s, j = b & (half - 1u);
    IndexButterfly o;
    o.i0 = ((b >> s) << (s + 1u)) + j;
    o.i1 = o.i0 + half;
    o.w = j << (m - 1u - s);
    return o;
}
// x0, x1 <- x0 + w x1, x0 - w x1
FFS_SPOTBG_HD inline void index_butterfly_apply(double wre, double wim, double& x0re, double& x0im, double& x1re, double& x1im) {
    const double tre = wre * x1re - wim * x1im;
    const double tim = wre * x1im + wim * x1re;
    const double are = x0re, aim = x0im;
    x0re = are + tre, x0im = aim + tim;
    x1re = are - tre, x1im = aim - tim;
}
// where element p of line `line` (0 .. N^2 - 1) along `axis` lies in the flat grid
FFS_SPOTBG_HD inline uint64_t index_line_element(uint32_t n, int axis, uint32_t line, uint32_t p) {
    const uint64_t N = n, hi = line / n, lo = line % n;
    if (axis == 0) return (uint64_t)p * N * N + hi * N + lo;   // line = (c1, c2)
    if (axis == 1) return hi * N * N + (uint64_t)p * N + lo;   // line = (c0, c2)
    return (uint64_t)line * N + p;                             // line = (c0, c1)
}

// ---- components --------------------------------------------------------------------------------------------------------------------------
FFS_SPOTBG_HD inline void index_coords(uint32_t n, uint32_t flat, int32_t* c) {
    c[2] = (int32_t)(flat % n);
    c[1] = (int32_t)((flat / n) % n);
    c[0] = (int32_t)(flat / (n * n));
}
// the coordinate c of a voxel, unwrapped relative to its root's coordinate
FFS_SPOTBG_HD inline int32_t index_unwrap(int32_t c, int32_t c_root, int32_t n) { return c_root + ((c - c_root + n / 2 + n) % n) - n / 2; }
FFS_SPOTBG_HD inline void index_peak_finish(IndexPeak& p, uint32_t n) {
    const double div = (double)((uint64_t)p.n_voxels * (uint64_t)n);
    for (int j = 0; j < 3; ++j) p.frac[j] = (double)p.sum[j] / div;
}

// ---- the grid's statistics from the two tree sums ------------------------------------------------------------------------------------------
FFS_SPOTBG_HD inline double index_mean(double sum, uint32_t n) { return sum / (double)((uint64_t)n * n * n); }
FFS_SPOTBG_HD inline double index_sq_dev(double v, double mean) { return (v - mean) * (v - mean); }
inline void index_stats_finish(IndexGridStats& st, double sum, double ssq, uint32_t n, double rmsd_cutoff) {
    st.sum = sum;
    st.mean = index_mean(sum, n);
    st.rmsd = sqrt(ssq / (double)((uint64_t)n * n * n));
    st.cutoff = rmsd_cutoff * st.rmsd;
}

// ---- host only -----------------------------------------------------------------------------------------------------------------------------
// libm itself, in every build: through volatile pointers no call is folded at compile time or merged with another
struct IndexLibm {
    double (*volatile cos_)(double) = cos;
    double (*volatile sin_)(double) = sin;
    double (*volatile exp_)(double) = exp;
    double (*volatile log_)(double) = log;
    double (*volatile acos_)(double) = acos;
    double (*volatile round_)(double) = round;
};

inline double index_norm(const double* v) { return sqrt(shoebox_dot(v, v)); }

// xyz: (x_px, y_px, z); rlp, s1, xyz_mm: three doubles each (xyz_mm = x_mm, y_mm, angle in radians)
inline void index_rlp(const ShoeboxGeometry& g, const double* xyz, double* rlp, double* s1, double* xyz_mm) {
    IndexLibm lm;
    const double x = xyz[0] * g.pixel_size_mm[0], y = xyz[1] * g.pixel_size_mm[1];
    double L[3];
    for (int i = 0; i < 3; ++i) L[i] = (g.d_matrix[3 * i] * x + g.d_matrix[3 * i + 1] * y) + g.d_matrix[3 * i + 2];
    shoebox_normalize(L);
    for (int i = 0; i < 3; ++i) s1[i] = L[i] / g.wavelength;
    const double angle = (g.osc_start_deg + xyz[2] * g.osc_width_deg) * kShoeboxDegToRad;
    xyz_mm[0] = x, xyz_mm[1] = y, xyz_mm[2] = angle;
    double u[3] = {g.rot_axis[0], g.rot_axis[1], g.rot_axis[2]}, S[3], X[3];
    shoebox_normalize(u);
    for (int i = 0; i < 3; ++i) S[i] = s1[i] - g.s0[i];
    const double c = lm.cos_(-1.0 * angle), s = lm.sin_(-1.0 * angle), d = shoebox_dot(u, S);
    shoebox_cross(u, S, X);
    for (int i = 0; i < 3; ++i) rlp[i] = (S[i] * c + (u[i] * d) * (1.0 - c)) + s * X[i];
}

inline void index_defaults(const double* rlp, uint32_t n, double max_cell, uint32_t n_points, double& dmin, double& b_iso) {
    IndexLibm lm;
    if (dmin == 0.0) {
        dmin = 5.0 * max_cell / (double)n_points;
        double d_data = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const double d = 1.0 / index_norm(rlp + 3 * (size_t)i);
            if (i == 0 || d < d_data) d_data = d;
        }
        if (n > 0 && d_data > dmin) dmin = d_data;
    }
    b_iso = (-4.0 * (dmin * dmin)) * lm.log_(0.05);
}

inline void index_twiddles(uint32_t n_points, double* out) {   // n_points doubles: (re, im) of w[0 .. n_points/2 - 1]
    IndexLibm lm;
    for (uint32_t k = 0; k < n_points / 2u; ++k) {
        const double a = M_PI * ((double)(2u * k) / (double)n_points);
        out[2 * k] = lm.cos_(a);
        out[2 * k + 1] = -lm.sin_(a);
    }
}

// one spot: its cell (kIndexNotUsed: not used) and weight
inline uint32_t index_map_one(const double* v, double dmin, double b_iso, uint32_t n_points, double& weight) {
    IndexLibm lm;
    weight = 0.0;
    const double rlgrid = 2.0 / (dmin * (double)n_points), q = 1.0 / rlgrid;
    const double len = index_norm(v);
    if (1.0 / len < dmin) return kIndexNotUsed;
    int32_t c[3];
    for (int j = 0; j < 3; ++j) {
        const double r = lm.round_(v[j] * q);
        if (!(r >= -1.0e6 && r <= 1.0e6)) return kIndexNotUsed;
        c[j] = (int32_t)r + (int32_t)(n_points / 2u);
        if (c[j] < 0 || c[j] >= (int32_t)n_points) return kIndexNotUsed;
    }
    weight = b_iso != 0.0 ? lm.exp_(((-b_iso * len) * len) / 4.0) : 1.0;
    return (uint32_t)c[2] + n_points * (uint32_t)c[1] + n_points * n_points * (uint32_t)c[0];
}

// The list the device receives: one (cell, weight) per occupied cell, the weight of the highest spot number; in ascending order of that spot
inline void index_map_dedup(const uint32_t* cell, const double* weight, uint32_t n, std::vector<uint32_t>& cells, std::vector<double>& weights) {
    std::vector<std::pair<uint32_t, uint32_t>> by_cell;   // (cell, spot)
    for (uint32_t i = 0; i < n; ++i)
        if (cell[i] != kIndexNotUsed) by_cell.push_back({cell[i], i});
    std::sort(by_cell.begin(), by_cell.end());
    std::vector<uint32_t> winners;
    for (size_t i = 0; i < by_cell.size(); ++i)
        if (i + 1 == by_cell.size() || by_cell[i + 1].first != by_cell[i].first) winners.push_back(by_cell[i].second);
    std::sort(winners.begin(), winners.end());
    cells.clear(), weights.clear();
    for (uint32_t i : winners) cells.push_back(cell[i]), weights.push_back(weight[i]);
}

// The FFT of the whole grid, in place, walking the schedule butterfly by butterfly
inline void index_fft_line(IndexComplex* x, uint32_t n, uint32_t m, const double* tw) {
    for (uint32_t s = 0; s < m; ++s)
        for (uint32_t b = 0; b < n / 2u; ++b) {
            const IndexButterfly f = index_butterfly(m, s, b);
            index_butterfly_apply(tw[2 * f.w], tw[2 * f.w + 1], x[f.i0].re, x[f.i0].im, x[f.i1].re, x[f.i1].im);
        }
}
inline void index_fft3d(IndexComplex* grid, uint32_t n, const double* tw) {
    const uint32_t m = index_log2(n);
    std::vector<IndexComplex> line(n);
    for (int axis = 0; axis < 3; ++axis)
        for (uint32_t l = 0; l < n * n; ++l) {
            for (uint32_t p = 0; p < n; ++p) line[index_bitrev(p, m)] = grid[index_line_element(n, axis, l, p)];
            index_fft_line(line.data(), n, m, tw);
            for (uint32_t p = 0; p < n; ++p) grid[index_line_element(n, axis, l, p)] = line[p];
        }
}
// cells, weights: the deduplicated list; power: N^3 doubles
inline void index_power_grid(const uint32_t* cells, const double* weights, size_t n_cells, uint32_t n, const double* tw, double* power) {
    const size_t total = (size_t)n * n * n;
    std::vector<IndexComplex> grid(total, IndexComplex{0.0, 0.0});
    for (size_t i = 0; i < n_cells; ++i) grid[cells[i]] = IndexComplex{weights[i], 0.0};
    index_fft3d(grid.data(), n, tw);
    for (size_t i = 0; i < total; ++i) power[i] = grid[i].re * grid[i].re;
}

inline double index_tree_sum(double* v, uint32_t n) {   // destroys v
    for (uint32_t s = n / 2u; s >= 1u; s /= 2u)
        for (uint32_t i = 0; i < s; ++i) v[i] = v[i] + v[i + s];
    return v[0];
}
// the tree over the grid of f(v): lines, then the lines of a plane, then the planes
template <typename F>
inline double index_grid_tree(const double* power, uint32_t n, F&& f) {
    std::vector<double> line(n), lines(n), planes(n);
    for (uint32_t c0 = 0; c0 < n; ++c0) {
        for (uint32_t c1 = 0; c1 < n; ++c1) {
            const double* src = power + ((size_t)c0 * n + c1) * n;
            for (uint32_t c2 = 0; c2 < n; ++c2) line[c2] = f(src[c2]);
            lines[c1] = index_tree_sum(line.data(), n);
        }
        planes[c0] = index_tree_sum(lines.data(), n);
    }
    return index_tree_sum(planes.data(), n);
}
inline void index_grid_stats(const double* power, uint32_t n, double rmsd_cutoff, IndexGridStats& st) {
    const double sum = index_grid_tree(power, n, [](double v) { return v; });
    const double mean = index_mean(sum, n);
    const double ssq = index_grid_tree(power, n, [mean](double v) { return index_sq_dev(v, mean); });
    index_stats_finish(st, sum, ssq, n, rmsd_cutoff);
    st.n_selected = st.n_peaks = 0u;
}

// The peaks of a power grid: statistics, selection, components, records in ascending order of root
inline void index_peaks(const double* power, uint32_t n, double rmsd_cutoff, IndexGridStats& st, std::vector<IndexPeak>& peaks) {
    index_grid_stats(power, n, rmsd_cutoff, st);
    const size_t total = (size_t)n * n * n;
    std::vector<int32_t> label(total, -2);   // -2 not selected, -1 selected and not reached yet, else the index of its record
    for (size_t i = 0; i < total; ++i)
        if (power[i] >= st.cutoff) label[i] = -1, ++st.n_selected;
    peaks.clear();
    std::vector<uint32_t> stack;
    for (size_t i = 0; i < total; ++i) {
        if (label[i] != -1) continue;
        IndexPeak p{};
        p.root = (uint32_t)i;   // the first voxel met in ascending order is the component's smallest
        int32_t cr[3];
        index_coords(n, p.root, cr);
        label[i] = (int32_t)peaks.size();
        stack.push_back(p.root);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            stack.pop_back();
            int32_t c[3];
            index_coords(n, v, c);
            ++p.n_voxels;
            for (int j = 0; j < 3; ++j) p.sum[j] += index_unwrap(c[j], cr[j], (int32_t)n);
            for (int j = 0; j < 3; ++j)
                for (int d = -1; d <= 1; d += 2) {
                    int32_t e[3] = {c[0], c[1], c[2]};
                    e[j] = (e[j] + d + (int32_t)n) % (int32_t)n;
                    const uint32_t w = ((uint32_t)e[0] * n + (uint32_t)e[1]) * n + (uint32_t)e[2];
                    if (label[w] == -1) label[w] = label[i], stack.push_back(w);
                }
        }
        index_peak_finish(p, n);
        peaks.push_back(p);
    }
    st.n_peaks = (uint32_t)peaks.size();
}

// flood_fill_filter: which peaks stay
inline std::vector<IndexPeak> index_filter(const IndexPeak* peaks, uint32_t n, double peak_volume_cutoff) {
    std::vector<IndexPeak> out;
    if (n == 0u) return out;
    std::vector<int64_t> vol(n);
    for (uint32_t i = 0; i < n; ++i) vol[i] = peaks[i].n_voxels;
    std::sort(vol.begin(), vol.end());
    const int64_t q3 = vol[(size_t)n * 3 / 4], q1 = vol[n / 4], cut = (q3 - q1) * 5 + q3;
    while (vol.back() > cut) vol.pop_back();
    const int64_t peak_cutoff = (int64_t)(peak_volume_cutoff * (double)vol.back());
    for (uint32_t i = 0; i < n; ++i)
        if (!((int64_t)peaks[i].n_voxels <= peak_cutoff)) out.push_back(peaks[i]);
    return out;
}

inline double index_angle_deg(const double* a, const double* b) {
    IndexLibm lm;
    const double nd = shoebox_dot(a, b) / (index_norm(a) * index_norm(b));
    if (fabs(nd - 1.0) < 1e-6) return 0.0;
    if (fabs(nd + 1.0) < 1e-6) return 180.0;
    return lm.acos_(nd) * 180.0 / M_PI;
}
inline bool index_integer_multiple(const double* v1, const double* v2) {
    IndexLibm lm;
    const double angle = index_angle_deg(v1, v2);
    if (angle < 5.0 || fabs(180.0 - angle) < 5.0) {
        double l1 = index_norm(v1), l2 = index_norm(v2);
        if (l1 > l2) std::swap(l1, l2);
        const double k = l2 / l1;
        if (fabs(lm.round_(k) - k) < 0.2) return true;
    }
    return false;
}

// flood_fill_filter and peaks_to_rlvs
inline std::vector<IndexVector> index_basis_vectors(const IndexPeak* all, uint32_t n_all, uint32_t n_points, double dmin, double peak_volume_cutoff, double min_cell,
                                                    double max_cell) {
    const std::vector<IndexPeak> peaks = index_filter(all, n_all, peak_volume_cutoff);
    const double fft_cell_length = (double)n_points * dmin / 2.0;
    std::vector<IndexVector> sites;
    for (const IndexPeak& p : peaks) {
        IndexVector s{};
        for (int j = 0; j < 3; ++j) {
            double val = p.frac[j];
            if (val > 0.5) val -= 1.0;
            s.v[j] = val * fft_cell_length;
        }
        s.length = index_norm(s.v);
        s.volume = p.n_voxels;
        if (s.length > min_cell && s.length < 2.0 * max_cell) sites.push_back(s);
    }
    struct Group {
        std::vector<IndexVector> members;
        void mean(double* o) const {
            o[0] = o[1] = o[2] = 0.0;
            for (const IndexVector& s : members)
                for (int j = 0; j < 3; ++j) o[j] = o[j] + s.v[j];
            for (int j = 0; j < 3; ++j) o[j] = o[j] / (double)members.size();
        }
    };
    std::vector<Group> groups;
    for (const IndexVector& s : sites) {
        bool matched = false;
        for (Group& g : groups) {
            double mv[3];
            g.mean(mv);
            const double ml = index_norm(mv);
            if (fabs(ml - s.length) / std::max(ml, s.length) < 0.1) {
                const double angle = index_angle_deg(mv, s.v);
                if (angle < 5.0) {
                    g.members.push_back(s);
                    matched = true;
                    break;
                } else if (fabs(180.0 - angle) < 5.0) {
                    IndexVector t = s;
                    for (int j = 0; j < 3; ++j) t.v[j] = -1.0 * s.v[j];
                    g.members.push_back(t);
                    matched = true;
                    break;
                }
            }
        }
        if (!matched) groups.push_back(Group{{s}});
    }
    std::vector<IndexVector> grouped;
    for (const Group& g : groups) {
        IndexVector s{};
        g.mean(s.v);
        s.length = index_norm(s.v);
        for (const IndexVector& t : g.members) s.volume = std::max(s.volume, t.volume);
        grouped.push_back(s);
    }
    const auto by_volume = [](const IndexVector& a, const IndexVector& b) { return a.volume > b.volume; };
    const auto by_length = [](const IndexVector& a, const IndexVector& b) { return a.length < b.length; };
    std::stable_sort(grouped.begin(), grouped.end(), by_volume);
    std::stable_sort(grouped.begin(), grouped.end(), by_length);
    std::vector<IndexVector> unique;
    for (const IndexVector& s : grouped) {
        bool is_unique = true;
        for (const IndexVector& u : unique) {
            if (u.volume <= s.volume) continue;
            if (index_integer_multiple(u.v, s.v)) {
                is_unique = false;
                break;
            }
        }
        if (is_unique) unique.push_back(s);
    }
    std::stable_sort(unique.begin(), unique.end(), by_volume);
    return unique;
}
}  // namespace ffsamd
