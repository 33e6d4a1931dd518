// assign_check.cc -- csrc/assign_model.hpp as a stand-alone program (tests/test_assign_oracle.py builds it with g++ -ffp-contract=off, plain and
// under the address and undefined-behaviour sanitizers, and compares every byte it writes with tests/assign_oracle.py).
//   assign_check IN OUT
// IN:  uint32 n, m (settings), has_selected, n_vectors; double tolerance, dmin, osc_start_deg, threshold; rlp (n x 3 doubles); phi (n doubles);
//      selected (n bytes, when has_selected); A (m x 9 doubles); vectors (n_vectors x 3 doubles)
// OUT: the absence table (111 x 56 bytes); ffs_index_select's bytes (n); per setting the record (472 bytes), hkl (n x 3 int32), lsq (n doubles);
//      per setting int32 the detected test; per setting A after that test's reindexing (9 doubles, zeros when none or singular);
//      uint32 the number of settings from the vectors, then the settings (160 bytes each)
// Before anything is read it holds assign_round to libm's round on the corner values and the constant directions to the constructed table
// (exit code 4 or 5).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "assign_model.hpp"

using namespace ffsamd;

template <typename T>
static void put(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "assign_check: short write\n");
        exit(2);
    }
}
template <typename T>
static void get(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "assign_check: short read\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    double (*volatile libm_round)(double) = round;
    const double corner[] = {0.5, -0.5, 2.5, -2.5, 1.5, -1.5, 0.49999999999999994, -0.49999999999999994, 0.0, -0.0, 0.25, -0.75, 524287.5, -524287.5, 524287.49999999994,
                             -524287.49999999994, 524287.0, 1.0, -1.0, 4503599627370495.5 / 8589934592.0};
    for (double x : corner)
        if ((double)assign_round(x) != libm_round(x)) {
            fprintf(stderr, "assign_check: assign_round(%.17g) = %d, round gives %.17g\n", x, assign_round(x), libm_round(x));
            return 4;
        }
    const std::vector<AssignAbsenceTest> table = assign_absence_table();
    if (table.size() != kAssignAbsenceTests) return 5;
    for (uint32_t t = 0; t < kAssignAbsenceTests; ++t)
        for (int k = 0; k < 3; ++k)
            if (table[t].v[k] != assign_direction(t / 3u, k) || table[t].modularity != assign_modularity(t % 3u)) {
                fprintf(stderr, "assign_check: test %u is not the constant's\n", t);
                return 5;
            }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[4];
    double par[4];
    get(in, head, 4);
    get(in, par, 4);
    const uint32_t n = head[0], m = head[1], n_vec = head[3];
    std::vector<double> rlp(3 * (size_t)n), phi(n), A(9 * (size_t)m), vectors(3 * (size_t)n_vec);
    std::vector<uint8_t> sel(n);
    get(in, rlp.data(), rlp.size()), get(in, phi.data(), phi.size());
    if (head[2]) get(in, sel.data(), sel.size());
    get(in, A.data(), A.size()), get(in, vectors.data(), vectors.size());
    put(out, table.data(), table.size());
    std::vector<uint8_t> chosen(n);
    for (uint32_t i = 0; i < n; ++i) chosen[i] = assign_selected(&rlp[3 * (size_t)i], phi[i], par[1], par[2]) ? 1 : 0;
    put(out, chosen.data(), chosen.size());
    std::vector<int32_t> hkl(3 * (size_t)n), detected(m);
    std::vector<double> lsq(n), reindexed(9 * (size_t)m, 0.0);
    for (uint32_t k = 0; k < m; ++k) {
        AssignRecord rec;
        assign_setting(rlp.data(), phi.data(), head[2] ? sel.data() : nullptr, n, &A[9 * (size_t)k], par[0], rec, hkl.data(), lsq.data());
        put(out, &rec, 1), put(out, hkl.data(), hkl.size()), put(out, lsq.data(), lsq.size());
        detected[k] = assign_detect(rec, par[3]);
        double next[9];
        if (detected[k] >= 0 && assign_reindex(&A[9 * (size_t)k], table[(size_t)detected[k]].transform, next))
            for (int j = 0; j < 9; ++j) reindexed[9 * (size_t)k + j] = next[j];
    }
    put(out, detected.data(), detected.size()), put(out, reindexed.data(), reindexed.size());
    const std::vector<AssignSetting> settings = assign_settings(vectors.data(), n_vec, kAssignMaxCombinations);
    const uint32_t n_settings = (uint32_t)settings.size();
    put(out, &n_settings, 1), put(out, settings.data(), settings.size());
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
