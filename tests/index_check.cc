// index_check.cc -- csrc/index_model.hpp as a stand-alone program (tests/test_index_oracle.py builds it with g++ -ffp-contract=off, plain and
// under the address and undefined-behaviour sanitizers, and compares every byte it writes with tests/index_oracle.py).
//   index_check IN OUT
// IN:  uint32 n_points, n, mode, 0; double max_cell, dmin (0 = choose), rmsd_cutoff, 0;
//      mode 0: the geometry (20 doubles, ffs_scan_geometry), then n x 3 doubles (x_px, y_px, z);  mode 1: n_points^3 doubles, a power grid
// OUT: mode 0: double dmin, b_iso; rlp, s1, xyz_mm (n x 3 doubles each); cell (n uint32); weight (n doubles); the power grid;
//      both modes: the statistics (40 bytes); uint32 n_peaks, n_vectors; the peaks (56 bytes each); the vectors (40 bytes each, mode 0 only)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "index_model.hpp"

using namespace ffsamd;

template <typename T>
static void put(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "index_check: short write\n");
        exit(2);
    }
}
template <typename T>
static void get(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "index_check: short read\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[4];
    double par[4];
    get(in, head, 4);
    get(in, par, 4);
    const uint32_t N = head[0], n = head[1], mode = head[2];
    if (!index_points_ok(N)) return 3;
    const size_t total = (size_t)N * N * N;
    std::vector<double> power(total);
    double dmin = par[1], b_iso = 0.0;
    if (mode == 0u) {
        ShoeboxGeometry g;
        get(in, &g, 1);
        std::vector<double> xyz(3 * (size_t)n), rlp(3 * (size_t)n), s1(3 * (size_t)n), mm(3 * (size_t)n), weight(n), weights;
        std::vector<uint32_t> cell(n), cells;
        get(in, xyz.data(), xyz.size());
        for (uint32_t i = 0; i < n; ++i) index_rlp(g, &xyz[3 * (size_t)i], &rlp[3 * (size_t)i], &s1[3 * (size_t)i], &mm[3 * (size_t)i]);
        index_defaults(rlp.data(), n, par[0], N, dmin, b_iso);
        for (uint32_t i = 0; i < n; ++i) cell[i] = index_map_one(&rlp[3 * (size_t)i], dmin, b_iso, N, weight[i]);
        index_map_dedup(cell.data(), weight.data(), n, cells, weights);
        std::vector<double> tw(N);
        index_twiddles(N, tw.data());
        index_power_grid(cells.data(), weights.data(), cells.size(), N, tw.data(), power.data());
        put(out, &dmin, 1), put(out, &b_iso, 1);
        put(out, rlp.data(), rlp.size()), put(out, s1.data(), s1.size()), put(out, mm.data(), mm.size());
        put(out, cell.data(), cell.size()), put(out, weight.data(), weight.size());
        put(out, power.data(), power.size());
    } else {
        get(in, power.data(), total);
    }
    IndexGridStats st;
    std::vector<IndexPeak> peaks;
    index_peaks(power.data(), N, par[2], st, peaks);
    std::vector<IndexVector> vectors;
    if (mode == 0u) vectors = index_basis_vectors(peaks.data(), (uint32_t)peaks.size(), N, dmin, kIndexPeakVolumeCutoff, kIndexMinCell, par[0]);
    const uint32_t counts[2] = {(uint32_t)peaks.size(), (uint32_t)vectors.size()};
    put(out, &st, 1), put(out, counts, 2), put(out, peaks.data(), peaks.size()), put(out, vectors.data(), vectors.size());
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
