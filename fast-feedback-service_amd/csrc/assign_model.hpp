// assign_model.hpp -- the rule of index assignment for candidate crystal settings (ffs_index_select / settings / absence_table /
// absence_detect / reindex, ffs_ctx_index_assign): which Miller index a spot gets under a setting A, which of two
// spots on one index stays, and the integer counts per setting that detect a non-primitive basis.  No HIP header: the kernels
// (kernels_assign.hpp), the library's host side, tools/ffs_hosttool.cc and a plain C++ test program (tests/assign_check.cc) compile the same
// text, all with -ffp-contract=off.
//
// It restates the reference's assign_indices.cc:56-165, non_primitive_basis.cc:25-34, 43-146, 158-177, 214-217, indexer.cc:266-276 and
// combinations.cc.  No parity with the reference's binaries is claimed: THIS TEXT IS THE CONTRACT.  Every operation is an IEEE float64
// + - * /, a comparison or a conversion, each rounded on its own, in the order written; the device evaluates no libm function.  sqrt
// (selection, cell lengths) and acos (the settings' angle tests) enter on the HOST only.
//
//   Convention: A is 3x3 row-major in 1/Angstrom with r = A h at rotation angle 0 (ffs_ctx_predict's); rlp and phi (radians) are
//       ffs_index_rlp's rlp and column 2 of its xyz_mm.
//   Inverse: c00 = A4 A8 - A5 A7, c01 = A5 A6 - A3 A8, c02 = A3 A7 - A4 A6, det = (A0 c00 + A1 c01) + A2 c02; every entry of Ai is a
//       cofactor (two products and a difference) divided by det.  det == 0 or an entry of Ai that is not finite: the setting is SINGULAR,
//       all its counts and Miller indices are 0 and every lsq is -1.
//   Per selected spot and setting: hf_j = (Ai[3j] r0 + Ai[3j+1] r1) + Ai[3j+2] r2; any fabs(hf_j) >= 524288.0 (2^19): OUT OF RANGE, counted,
//       not accepted, lsq -1 (the reference's static_cast<int> is undefined there; three components biased by 2^19 fit one 64-bit key).
//       h_j = round half away from zero without libm: t = trunc(hf_j) (a conversion to integer and back), d = hf_j - t (exact),
//       d >= 0.5: t + 1, d <= -0.5: t - 1, else t.  d_j = (double)h_j - hf_j, lsq = (d0 d0 + d1 d1) + d2 d2.
//       ACCEPTED when lsq <= tolerance * tolerance and (h0, h1, h2) != 0.
//   Duplicates, per setting among accepted spots of equal (h0, h1, h2) in ascending spot number: for a in order, for b after a in order:
//       skip when a or b is dead (after a dies the rest of its row is skipped); skip when fabs(phi_a - phi_b) > M_PI / 4; otherwise
//       lsq_b < lsq_a kills a, else b dies (a tie kills the later spot).  A dead spot's index becomes (0, 0, 0); survivors are INDEXED.
//   Per setting, integers only: n_accepted (before duplicates), n_indexed (after), n_out_of_range, sum_lsq_q40 = the sum over indexed
//       spots of (uint64)(lsq * 1099511627776.0), absent0[t] = the number of indexed spots with (h . v_t) mod m_t == 0.
//   The absence table (host, integers): the 11^3 points of -5 .. 5 sorted by squared length, then larger component sum, then
//       reverse-lexicographic, without the origin; representatives: squared length <= 6 and not collinear with an earlier one (37, the
//       constant table of assign_direction, which the check program holds to this construction); times the modularities 2, 3, 5, representative
//       outer.  Transform rows: the first point with p . v % m == 0, the next such not collinear with it, the next not coplanar; rows 0 and
//       1 swapped when the determinant is negative.
//   Detect: the first t with (double)absent0[t] / (double)n_indexed > threshold; -1 when none or n_indexed == 0.
//   Reindex: direct = inverse(A), M = transpose(inverse(T)), new_direct = M direct with each entry (M[3i] d[j] + M[3i+1] d[3+j]) +
//       M[3i+2] d[6+j], A' = inverse(new_direct).  The reference's niggli_reduce() after it is NOT restated: same lattice, basis not reduced.
//   Selection: selected unless 1.0 / sqrt((r0 r0 + r1 r1) + r2 r2) <= dmin or phi * (180.0 / M_PI) > osc_start_deg + 360.0.  An rlp of
//       zero gives 1.0 / 0.0 = +inf, which is not <= dmin: the spot is selected, gets hf = 0 and h = 0 and is never accepted.
//   Settings from basis vectors (combinations.cc): the first min(n, 100) vectors, all i < j < k, stable-sorted by i i + j j + k k, the first
//       max_combinations; the reference's angle tests in its order with min_angle 20 degrees (index_angle_deg of index_model.hpp: host acos
//       through a volatile pointer), its sign flips of v2, v3 and the handedness flip; the volume test V > a b c / 100 ON THE CELL AS BUILT
//       (the reference applies it after Niggli reduction, under which a b c can only shrink for a valid basis: the test here is the stricter).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "index_model.hpp"

#include <algorithm>
#include <array>
#include <map>
#include <vector>

namespace ffsamd {

constexpr uint32_t kAssignAbsenceTests = 111u, kAssignDirectionCount = 37u;   // FFS_INDEX_ABSENCE_TESTS
constexpr uint32_t kAssignSingular = 1u;                                      // FFS_INDEX_ASSIGN_SINGULAR
constexpr double kAssignLimit = 524288.0;         // 2^19
constexpr int32_t kAssignBias = 1 << 19;
constexpr double kAssignQ40 = 1099511627776.0;    // 2^40
constexpr double kAssignPhiWindow = M_PI / 4;
constexpr double kAssignRadToDeg = 180.0 / M_PI;
constexpr double kAssignMinAngle = 20.0;
constexpr uint32_t kAssignMaxVectors = 100u, kAssignMaxCombinations = 1000u;
constexpr double kAssignThreshold = 0.9, kAssignTolerance = 0.3;

// The word a (spot, setting) pair is kept as: three components biased by 2^19 in 21 bits each (h0 highest, so that words order like the
// reference's lexicographic map; |h_j| <= 2^19 needs all 21), and the accepted bit on top.  A spot that is not accepted, is out of range, is
// not selected or has died among duplicates has the bit clear; nothing else fits, and nothing else is needed.
constexpr uint64_t kAssignAccepted = 1ull << 63;

struct AssignRecord {    // = ffs_index_assignment, 472 bytes
    uint32_t status, n_accepted, n_indexed, n_out_of_range;
    uint64_t sum_lsq_q40;
    uint32_t absent0[kAssignAbsenceTests];
    uint32_t reserved;
};
struct AssignAbsenceTest {   // = ffs_index_absence_test, 56 bytes
    int32_t v[3], modularity, transform[9], reserved;
};
struct AssignSetting {   // = ffs_index_setting, 160 bytes
    uint32_t triple[3], reserved;
    double axes[9], A[9];
};
static_assert(sizeof(AssignRecord) == 472 && sizeof(AssignAbsenceTest) == 56 && sizeof(AssignSetting) == 160, "ffs_index_assignment, _absence_test, _setting");

// the 37 representatives, in the table's order (assign_absence_table constructs them; tests/assign_check.cc compares)
FFS_SPOTBG_HD inline int32_t assign_direction(uint32_t dir, int k) {
    constexpr int8_t t[kAssignDirectionCount][3] = {
        {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 0, -1}, {1, -1, 0}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {-1, 1, 1},
        {2, 1, 0}, {2, 0, 1}, {1, 2, 0}, {1, 0, 2}, {0, 2, 1}, {0, 1, 2}, {2, 0, -1}, {2, -1, 0}, {0, 2, -1}, {0, -1, 2}, {-1, 2, 0}, {-1, 0, 2},
        {2, 1, 1}, {1, 2, 1}, {1, 1, 2}, {2, 1, -1}, {2, -1, 1}, {1, 2, -1}, {1, -1, 2}, {-1, 2, 1}, {-1, 1, 2}, {2, -1, -1}, {1, 1, -2}, {1, -2, 1}};
    return (int32_t)t[dir][k];
}
FFS_SPOTBG_HD inline int32_t assign_modularity(uint32_t mi) { return mi == 0u ? 2 : mi == 1u ? 3 : 5; }

FFS_SPOTBG_HD inline bool assign_finite(double x) { return x - x == 0.0; }

// Ai = inverse(A); false (Ai zeroed) when the setting is singular
FFS_SPOTBG_HD inline bool assign_inverse(const double* A, double* Ai) {
    const double c00 = A[4] * A[8] - A[5] * A[7];
    const double c01 = A[5] * A[6] - A[3] * A[8];
    const double c02 = A[3] * A[7] - A[4] * A[6];
    const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
    bool ok = det == 0.0 ? false : true;
    if (ok) {
        Ai[0] = c00 / det;
        Ai[1] = (A[2] * A[7] - A[1] * A[8]) / det;
        Ai[2] = (A[1] * A[5] - A[2] * A[4]) / det;
        Ai[3] = c01 / det;
        Ai[4] = (A[0] * A[8] - A[2] * A[6]) / det;
        Ai[5] = (A[2] * A[3] - A[0] * A[5]) / det;
        Ai[6] = c02 / det;
        Ai[7] = (A[1] * A[6] - A[0] * A[7]) / det;
        Ai[8] = (A[0] * A[4] - A[1] * A[3]) / det;
        for (int k = 0; k < 9; ++k) ok = ok && assign_finite(Ai[k]);
    }
    if (!ok)
        for (int k = 0; k < 9; ++k) Ai[k] = 0.0;
    return ok;
}

// round half away from zero of |hf| < 2^19, without libm
FFS_SPOTBG_HD inline int32_t assign_round(double hf) {
    const int32_t ti = (int32_t)hf;   // truncation toward zero
    const double d = hf - (double)ti;
    if (d >= 0.5) return ti + 1;
    if (d <= -0.5) return ti - 1;
    return ti;
}

FFS_SPOTBG_HD inline uint64_t assign_key(const int32_t* h) {
    return kAssignAccepted | ((uint64_t)(uint32_t)(h[0] + kAssignBias) << 42) | ((uint64_t)(uint32_t)(h[1] + kAssignBias) << 21) | (uint64_t)(uint32_t)(h[2] + kAssignBias);
}
FFS_SPOTBG_HD inline void assign_unkey(uint64_t w, int32_t* h) {
    h[0] = (int32_t)((w >> 42) & 0x1FFFFFull) - kAssignBias;
    h[1] = (int32_t)((w >> 21) & 0x1FFFFFull) - kAssignBias;
    h[2] = (int32_t)(w & 0x1FFFFFull) - kAssignBias;
}

// One selected spot under one setting: its word (the biased components, with the accepted bit when accepted; 0 when out of range) and its
// lsq (-1 when out of range, and only then negative)
FFS_SPOTBG_HD inline uint64_t assign_one(const double* Ai, double r0, double r1, double r2, double tol_sq, double& lsq) {
    double hf[3];
    for (int j = 0; j < 3; ++j) hf[j] = (Ai[3 * j] * r0 + Ai[3 * j + 1] * r1) + Ai[3 * j + 2] * r2;
    lsq = -1.0;
    if (fabs(hf[0]) >= kAssignLimit || fabs(hf[1]) >= kAssignLimit || fabs(hf[2]) >= kAssignLimit) return 0ull;
    int32_t h[3];
    double d[3];
    for (int j = 0; j < 3; ++j) {
        h[j] = assign_round(hf[j]);
        d[j] = (double)h[j] - hf[j];
    }
    lsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const uint64_t key = assign_key(h);
    const bool accepted = lsq <= tol_sq && (h[0] != 0 || h[1] != 0 || h[2] != 0);
    return accepted ? key : key & ~kAssignAccepted;
}
FFS_SPOTBG_HD inline uint64_t assign_lsq_q40(double lsq) { return (uint64_t)(lsq * kAssignQ40); }
// absence test t = 3 * direction + modularity's position, on an indexed spot
FFS_SPOTBG_HD inline int32_t assign_direction_dot(uint32_t dir, const int32_t* h) {
    return h[0] * assign_direction(dir, 0) + h[1] * assign_direction(dir, 1) + h[2] * assign_direction(dir, 2);
}

// ---- host only -----------------------------------------------------------------------------------------------------------------------------
inline bool assign_selected(const double* r, double phi, double dmin, double osc_start_deg) {
    const double norm = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    return !(1.0 / norm <= dmin || phi * kAssignRadToDeg > osc_start_deg + 360.0);
}

// The pair rule over one group's members (ascending spot number): dead[k] for member k
inline void assign_resolve_group(const std::vector<uint32_t>& members, const double* lsq, const double* phi, std::vector<uint8_t>& dead) {
    for (size_t x = 0; x < members.size(); ++x)
        for (size_t y = x + 1; y < members.size(); ++y) {
            const uint32_t a = members[x], b = members[y];
            if (dead[a] || dead[b]) continue;
            if (fabs(phi[a] - phi[b]) > kAssignPhiWindow) continue;
            if (lsq[b] < lsq[a])
                dead[a] = 1;
            else
                dead[b] = 1;
        }
}

// One setting on the host: the record, and hkl (n x 3) and lsq (n) when not NULL.  selected may be NULL (all).
inline void assign_setting(const double* rlp, const double* phi, const uint8_t* selected, uint32_t n, const double* A, double tolerance, AssignRecord& rec, int32_t* hkl,
                           double* lsq_out) {
    memset(&rec, 0, sizeof rec);
    if (hkl) memset(hkl, 0, 3 * (size_t)n * sizeof(int32_t));
    if (lsq_out)
        for (uint32_t i = 0; i < n; ++i) lsq_out[i] = -1.0;
    double Ai[9];
    if (!assign_inverse(A, Ai)) {
        rec.status = kAssignSingular;
        return;
    }
    const double tol_sq = tolerance * tolerance;
    std::vector<uint64_t> word(n, 0ull);
    std::vector<double> lsq(n, -1.0);
    std::map<uint64_t, std::vector<uint32_t>> groups;
    for (uint32_t i = 0; i < n; ++i) {
        if (selected && !selected[i]) continue;
        word[i] = assign_one(Ai, rlp[3 * (size_t)i], rlp[3 * (size_t)i + 1], rlp[3 * (size_t)i + 2], tol_sq, lsq[i]);
        if (lsq[i] < 0.0) ++rec.n_out_of_range;
        if (word[i] & kAssignAccepted) ++rec.n_accepted, groups[word[i]].push_back(i);
    }
    std::vector<uint8_t> dead(n, 0);
    for (const auto& g : groups)
        if (g.second.size() > 1) assign_resolve_group(g.second, lsq.data(), phi, dead);
    for (uint32_t i = 0; i < n; ++i) {
        if (lsq_out) lsq_out[i] = lsq[i];
        if (!(word[i] & kAssignAccepted) || dead[i]) continue;
        int32_t h[3];
        assign_unkey(word[i], h);
        if (hkl) hkl[3 * (size_t)i] = h[0], hkl[3 * (size_t)i + 1] = h[1], hkl[3 * (size_t)i + 2] = h[2];
        ++rec.n_indexed;
        rec.sum_lsq_q40 += assign_lsq_q40(lsq[i]);
        for (uint32_t dir = 0; dir < kAssignDirectionCount; ++dir) {
            const int32_t dv = assign_direction_dot(dir, h);
            for (uint32_t m = 0; m < 3u; ++m)
                if (dv % assign_modularity(m) == 0) ++rec.absent0[3u * dir + m];
        }
    }
}

// The absence table: 111 entries
inline std::vector<AssignAbsenceTest> assign_absence_table() {
    typedef std::array<int32_t, 3> P;
    const auto dot = [](const P& a, const P& b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const auto cross = [](const P& a, const P& b) { return P{a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}; };
    const P zero{0, 0, 0};
    std::vector<P> points;
    for (int32_t i = 5; i > -6; --i)
        for (int32_t j = 5; j > -6; --j)
            for (int32_t k = 5; k > -6; --k) points.push_back(P{i, j, k});
    std::sort(points.begin(), points.end(), [&](const P& a, const P& b) {
        const int32_t da = dot(a, a), db = dot(b, b), sa = a[0] + a[1] + a[2], sb = b[0] + b[1] + b[2];
        if (da != db) return da < db;
        if (sa != sb) return sa > sb;
        return b < a;   // reverse-lexicographic: (1,0,0) before (0,1,0) before (0,0,1)
    });
    points.erase(points.begin());   // the origin
    std::vector<P> reps;
    for (const P& p : points) {
        if (dot(p, p) > 6) break;
        bool collinear = false;
        for (const P& r : reps) collinear = collinear || cross(p, r) == zero;
        if (!collinear) reps.push_back(p);
    }
    std::vector<AssignAbsenceTest> out;
    for (const P& v : reps)
        for (uint32_t mi = 0; mi < 3u; ++mi) {
            const int32_t m = assign_modularity(mi);
            std::vector<P> cand;
            for (const P& p : points)
                if (dot(p, v) % m == 0) cand.push_back(p);
            size_t at = 0;
            const P first = cand[at++];
            while (cross(cand[at], first) == zero) ++at;
            const P second = cand[at++];
            while (dot(cross(second, first), cand[at]) == 0) ++at;
            const P third = cand[at];
            const bool swap = dot(cross(first, second), third) < 0;   // the determinant of the rows (first, second, third)
            const P& r0 = swap ? second : first;
            const P& r1 = swap ? first : second;
            AssignAbsenceTest t{};
            for (int k = 0; k < 3; ++k) t.v[k] = v[k], t.transform[k] = r0[k], t.transform[3 + k] = r1[k], t.transform[6 + k] = third[k];
            t.modularity = m;
            out.push_back(t);
        }
    return out;
}

inline int32_t assign_detect(const AssignRecord& rec, double threshold) {
    if (rec.n_indexed == 0u) return -1;
    for (uint32_t t = 0; t < kAssignAbsenceTests; ++t)
        if ((double)rec.absent0[t] / (double)rec.n_indexed > threshold) return (int32_t)t;
    return -1;
}

inline void assign_matmul(const double* M, const double* D, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (M[3 * i] * D[j] + M[3 * i + 1] * D[3 + j]) + M[3 * i + 2] * D[6 + j];
}
// A' = the setting after the integer transform T of an absence test; false when an inverse on the way is singular
inline bool assign_reindex(const double* A, const int32_t* T, double* out) {
    double direct[9], Td[9], Ti[9], M[9], nd[9];
    if (!assign_inverse(A, direct)) return false;
    for (int k = 0; k < 9; ++k) Td[k] = (double)T[k];
    if (!assign_inverse(Td, Ti)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = Ti[3 * j + i];
    assign_matmul(M, direct, nd);
    return assign_inverse(nd, out);
}

// combinations.cc without the Niggli reduction; vectors: n x 3 doubles (Angstrom)
inline std::vector<AssignSetting> assign_settings(const double* vectors, uint32_t n_vectors, uint32_t max_combinations) {
    const uint32_t n = std::min(n_vectors, kAssignMaxVectors);
    std::vector<std::array<uint32_t, 3>> triples;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j)
            for (uint32_t k = j + 1; k < n; ++k) triples.push_back({i, j, k});
    std::stable_sort(triples.begin(), triples.end(), [](const std::array<uint32_t, 3>& a, const std::array<uint32_t, 3>& b) {
        return a[0] * a[0] + a[1] * a[1] + a[2] * a[2] < b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
    });
    if (triples.size() > max_combinations) triples.resize(max_combinations);
    std::vector<AssignSetting> out;
    for (const auto& t : triples) {
        double v1[3], v2[3], v3[3], cp[3];
        for (int k = 0; k < 3; ++k) v1[k] = vectors[3 * (size_t)t[0] + k], v2[k] = vectors[3 * (size_t)t[1] + k], v3[k] = vectors[3 * (size_t)t[2] + k];
        const double gamma = index_angle_deg(v1, v2);
        if (gamma < kAssignMinAngle || (180.0 - gamma) < kAssignMinAngle) continue;
        shoebox_cross(v1, v2, cp);
        if (gamma < 90.0)
            for (int k = 0; k < 3; ++k) v2[k] = -1.0 * v2[k], cp[k] = -1.0 * cp[k];
        if (fabs(90.0 - index_angle_deg(cp, v3)) < kAssignMinAngle) continue;
        if (index_angle_deg(v2, v3) < 90.0)
            for (int k = 0; k < 3; ++k) v3[k] = -1.0 * v3[k];
        if (shoebox_dot(cp, v3) < 0.0)
            for (int k = 0; k < 3; ++k) v1[k] = -1.0 * v1[k], v2[k] = -1.0 * v2[k], v3[k] = -1.0 * v3[k];
        AssignSetting s{};
        for (int k = 0; k < 3; ++k) s.triple[k] = t[k], s.axes[k] = v1[k], s.axes[3 + k] = v2[k], s.axes[6 + k] = v3[k];
        if (!assign_inverse(s.axes, s.A)) continue;
        const double* X = s.axes;
        const double c00 = X[4] * X[8] - X[5] * X[7], c01 = X[5] * X[6] - X[3] * X[8], c02 = X[3] * X[7] - X[4] * X[6];
        const double vol = fabs((X[0] * c00 + X[1] * c01) + X[2] * c02);
        if (!(vol > index_norm(v1) * index_norm(v2) * index_norm(v3) / 100.0)) continue;
        out.push_back(s);
    }
    return out;
}

}  // namespace ffsamd
