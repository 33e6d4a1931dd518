// index_assign.hpp -- what `spotfinder --index-assign` and `ffs_hosttool indexassign` share: the candidate settings (from basis vectors or from a
// file of raw rows of nine float64), the correction of every setting for a non-primitive basis (assign, detect, reindex, assign again: the
// loop of the reference's non_primitive_basis.cc:188-225 without its Niggli step, every setting of a round in ONE assignment call, at most 16
// reindexings a setting), the choice of the best setting, the lines printed and the three files.  EVERY centre is assigned: the selection
// of indexer.cc:266-276 (ffs_index_select) is not applied here, so M in `Indexed N/M reflections` is the number of centres.  The assignment itself, detect and reindex come from the caller: the
// driver passes the library's entries (the GPU), the host tool the same rule compiled from csrc/assign_model.hpp (the CPU).  Both run this
// text, so a test can hold the driver's files to the host tool's.
//
// PREFIX.settings: the 160-byte ffs_index_setting records as built (a settings file gives triple 0 and axes 0); PREFIX.assignments: the
// 472-byte ffs_index_assignment records after correction; PREFIX.hkl: n x 3 int32 of the best setting.  "Best" has the most indexed spots;
// ties go to the smaller cell volume 1 / |det A|, then to the lower number.
#pragma once
#include <math.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "ffs_hip.h"
#include "index_basis.hpp"

namespace ffshost {

constexpr int kIndexAssignMaxRounds = 16;

struct IndexAssignOps {
    // out: m records; hkl: NULL or m x n x 3.  Throws std::runtime_error with the refusal's text.
    std::function<void(const double* A, uint32_t m, ffs_index_assignment* out, int32_t* hkl)> assign;
    std::function<int32_t(const ffs_index_assignment&)> detect;
    std::function<bool(const double* A, int32_t test, double* out)> reindex;
};

// raw rows of nine float64
inline std::vector<ffs_index_setting> read_settings_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the settings file " + path);
    f.seekg(0, std::ios::end);
    const std::streamoff bytes = f.tellg();
    f.seekg(0);
    if (bytes < 0 || bytes % 72 != 0) throw std::runtime_error("the settings file " + path + " is not a whole number of rows of nine float64 (" + std::to_string((long long)bytes) + " bytes)");
    std::vector<double> rows((size_t)bytes / 8);
    if (!rows.empty()) f.read(reinterpret_cast<char*>(rows.data()), bytes);
    if (!f) throw std::runtime_error("short read of the settings file " + path);
    std::vector<ffs_index_setting> out(rows.size() / 9);
    for (size_t k = 0; k < out.size(); ++k) {
        std::memset(&out[k], 0, sizeof out[k]);
        for (int j = 0; j < 9; ++j) out[k].A[j] = rows[9 * k + (size_t)j];
    }
    return out;
}

// for the printed line only: the real-space cell of a setting (rows of inverse(A)) and its volume; zeros when A is singular
inline void index_assign_cell(const double* A, double* cell6, double& volume) {
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double det = (A[0] * c0 + A[1] * c1) + A[2] * c2;
    for (int k = 0; k < 6; ++k) cell6[k] = 0.0;
    volume = 0.0;
    if (det == 0.0 || !(det - det == 0.0)) return;
    const double d[9] = {c0 / det, (A[2] * A[7] - A[1] * A[8]) / det, (A[1] * A[5] - A[2] * A[4]) / det,
                         c1 / det, (A[0] * A[8] - A[2] * A[6]) / det, (A[2] * A[3] - A[0] * A[5]) / det,
                         c2 / det, (A[1] * A[6] - A[0] * A[7]) / det, (A[0] * A[4] - A[1] * A[3]) / det};
    volume = 1.0 / std::fabs(det);
    double len[3];
    for (int i = 0; i < 3; ++i) cell6[i] = len[i] = std::sqrt((d[3 * i] * d[3 * i] + d[3 * i + 1] * d[3 * i + 1]) + d[3 * i + 2] * d[3 * i + 2]);
    const int pair[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    for (int k = 0; k < 3; ++k) {
        const double* u = d + 3 * pair[k][0];
        const double* v = d + 3 * pair[k][1];
        const double c = ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) / (len[pair[k][0]] * len[pair[k][1]]);
        cell6[3 + k] = std::acos(c < -1.0 ? -1.0 : c > 1.0 ? 1.0 : c) * 180.0 / M_PI;
    }
}

// Runs the whole step for n spots and writes PREFIX.settings / .assignments / .hkl; returns the lines to print.
inline std::string index_assign_run(const IndexAssignOps& ops, const std::vector<ffs_index_setting>& settings, uint32_t n, const std::string& prefix) {
    const size_t m = settings.size();
    std::vector<double> A(9 * m);
    for (size_t k = 0; k < m; ++k)
        for (int j = 0; j < 9; ++j) A[9 * k + (size_t)j] = settings[k].A[j];
    std::vector<ffs_index_assignment> recs(m);
    std::vector<uint32_t> rounds(m, 0), pending(m);
    std::vector<uint8_t> stopped(m, 0);
    for (size_t k = 0; k < m; ++k) pending[k] = (uint32_t)k;
    // every round: the pending settings in one call; those with an absence detected are reindexed and stay pending
    for (int round = 0; !pending.empty(); ++round) {
        std::vector<double> batch(9 * pending.size());
        for (size_t p = 0; p < pending.size(); ++p)
            for (int j = 0; j < 9; ++j) batch[9 * p + (size_t)j] = A[9 * (size_t)pending[p] + (size_t)j];
        std::vector<ffs_index_assignment> got(pending.size());
        ops.assign(batch.data(), (uint32_t)pending.size(), got.data(), nullptr);
        std::vector<uint32_t> next;
        for (size_t p = 0; p < pending.size(); ++p) {
            const uint32_t k = pending[p];
            recs[k] = got[p];
            const int32_t t = ops.detect(got[p]);
            if (t < 0) continue;
            if (round == kIndexAssignMaxRounds) {   // (a setting that explains a handful of spots passes some absence test whatever its cell: it stays as it is)
                stopped[k] = 1;
                continue;
            }
            double out[9];
            if (!ops.reindex(&A[9 * (size_t)k], t, out)) continue;   // (a singular setting detects nothing: not reached)
            for (int j = 0; j < 9; ++j) A[9 * (size_t)k + (size_t)j] = out[j];
            ++rounds[k];
            next.push_back(k);
        }
        pending.swap(next);
    }
    std::string lines = "Candidate settings:\n";
    size_t best = 0;
    double best_volume = 0.0;
    for (size_t k = 0; k < m; ++k) {
        double cell[6], volume;
        index_assign_cell(&A[9 * k], cell, volume);
        char line[256];
        std::snprintf(line, sizeof line, "%zu cell %.3f %.3f %.3f %.3f %.3f %.3f volume %.1f indexed %u (%.2f%%)%s\n", k, cell[0], cell[1], cell[2], cell[3], cell[4], cell[5], volume,
                      recs[k].n_indexed, n ? 100.0 * (double)recs[k].n_indexed / (double)n : 0.0, rounds[k] ? (" reindexed " + std::to_string(rounds[k]) + (stopped[k] ? "x, an absence left" : "x")).c_str() : "");
        lines += line;
        if (k == 0 || recs[k].n_indexed > recs[best].n_indexed || (recs[k].n_indexed == recs[best].n_indexed && volume < best_volume)) best = k, best_volume = volume;
    }
    std::vector<int32_t> hkl(3 * (size_t)n, 0);
    uint32_t n_best = 0;
    if (m) {
        ffs_index_assignment again;
        ops.assign(&A[9 * best], 1, &again, hkl.data());
        n_best = again.n_indexed;
        char line[96];
        std::snprintf(line, sizeof line, "Best setting: %zu\n", best);
        lines += line;
    }
    write_raw_file(prefix + ".settings", settings.data(), settings.size() * sizeof(ffs_index_setting));
    write_raw_file(prefix + ".assignments", recs.data(), recs.size() * sizeof(ffs_index_assignment));
    write_raw_file(prefix + ".hkl", hkl.data(), hkl.size() * sizeof(int32_t));
    char last[128];
    std::snprintf(last, sizeof last, "Indexed %u/%u reflections (%.2f%% indexed)\n", n_best, n, n ? 100.0 * (double)n_best / (double)n : 0.0);   // indexer.cc:506-510
    return lines + last;
}

}  // namespace ffshost
