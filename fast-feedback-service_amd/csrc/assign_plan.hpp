// assign_plan.hpp -- what the host decides about index assignment (ffs_ctx_index_assign): which calls are refused and
// why, how many settings one pass takes under workspace_bytes, the launches' shapes and the bytes of device state.  No HIP header:
// ffs_assign.hip acts on these decisions and a plain C++ test program (tests/assign_plan_check.cc) asks the same text.  The rule itself is
// assign_model.hpp's.
//
// Device state per setting of a pass, n spots, T = assign_table_slots(n) (the power of two >= 2 n, at least 256):
//   the pairs' words 8 n; the key table 8 T, its counts 4 T and its groups' places 4 T; the groups' members, as met and sorted, 4 n + 4 n;
//   the members' cursor 4; and when the caller asked, hkl 12 n and lsq 8 n.  16 n + 16 T + 4 is between 48 and 80 bytes a (spot, setting).
// Kept for the whole call beside the passes (not counted against workspace_bytes): rlp as three planes and phi 32 n, selected n, the
// settings' inverses 72 and records 472 a candidate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "assign_model.hpp"

namespace ffsamd {

constexpr uint32_t kAssignMaxSpots = 1u << 20, kAssignMaxCandidates = 4096u;
constexpr size_t kAssignDefaultWorkspace = (size_t)256 << 20;
constexpr int kAssignThreads = 256;
constexpr uint32_t kAssignMinSlots = 256u;

inline uint32_t assign_table_slots(uint32_t n) {
    uint32_t t = kAssignMinSlots;
    while (t < 2u * n) t *= 2u;
    return t;
}
inline size_t assign_setting_bytes(uint32_t n, bool want_hkl, bool want_lsq) {
    return 16u * (size_t)n + 16u * (size_t)assign_table_slots(n) + 4u + (want_hkl ? 12u * (size_t)n : 0u) + (want_lsq ? 8u * (size_t)n : 0u);
}
// settings a pass takes: as many as fit, at most n_candidates, at least one; 0 when not even one fits
inline uint32_t assign_pass_settings(uint32_t n, uint32_t n_candidates, size_t workspace_bytes, bool want_hkl, bool want_lsq) {
    const size_t room = workspace_bytes ? workspace_bytes : kAssignDefaultWorkspace;
    const size_t fit = room / assign_setting_bytes(n, want_hkl, want_lsq);
    if (fit == 0u) return 0u;
    return (uint32_t)(fit < (size_t)n_candidates ? fit : (size_t)n_candidates);
}
inline uint32_t assign_passes(uint32_t n_candidates, uint32_t per_pass) { return per_pass ? (n_candidates + per_pass - 1u) / per_pass : 0u; }
inline uint32_t assign_spot_blocks(uint32_t n) { return (n + (uint32_t)kAssignThreads - 1u) / (uint32_t)kAssignThreads; }   // grid x of the stages with a lane a pair
inline uint32_t assign_slot_blocks(uint32_t n) { return assign_table_slots(n) / (uint32_t)kAssignThreads; }                 // grid x of the stages with a lane a slot

inline std::string assign_finite_refusal(const double* v, size_t n, const char* what) {
    for (size_t i = 0; i < n; ++i)
        if (!assign_finite(v[i])) return std::string(what) + " has an entry that is not finite";
    return "";
}

inline std::string assign_refusal(const double* rlp, const double* phi, uint32_t n, const double* A, uint32_t n_candidates, double tolerance, bool out_null) {
    if (n > 0u && (!rlp || !phi)) return "rlp or phi is NULL";
    if (n_candidates > 0u && (!A || out_null)) return "A or out is NULL";
    if (n > kAssignMaxSpots) return "n must be at most 1048576, got " + std::to_string(n);
    if (n_candidates > kAssignMaxCandidates) return "n_candidates must be at most 4096, got " + std::to_string(n_candidates);
    if (!assign_finite(tolerance) || !(tolerance > 0.0) || tolerance > 0.5) return "tolerance must be in (0, 0.5]";
    std::string why = assign_finite_refusal(rlp, 3 * (size_t)n, "rlp");
    if (why.empty()) why = assign_finite_refusal(phi, (size_t)n, "phi");
    if (why.empty()) why = assign_finite_refusal(A, 9 * (size_t)n_candidates, "A");
    return why;
}
inline std::string assign_select_refusal(const double* rlp, const double* phi, uint32_t n, double dmin, double osc_start_deg, bool out_null) {
    if (n > 0u && (!rlp || !phi || out_null)) return "rlp, phi or selected is NULL";
    if (!assign_finite(dmin) || dmin < 0.0) return "dmin must be finite and not negative";
    if (!assign_finite(osc_start_deg)) return "osc_start_deg must be finite";
    std::string why = assign_finite_refusal(rlp, 3 * (size_t)n, "rlp");
    if (why.empty()) why = assign_finite_refusal(phi, (size_t)n, "phi");
    return why;
}
inline std::string assign_settings_refusal(const double* vectors, uint32_t n, uint32_t max_combinations, bool out_null, uint32_t cap, bool n_out_null) {
    if ((!vectors && n > 0u) || n_out_null || (out_null && cap > 0u)) return "vectors or n_out is NULL, or out is NULL with cap > 0";
    if (max_combinations == 0u) return "max_combinations must be positive";
    return assign_finite_refusal(vectors, 3 * (size_t)n, "vectors");
}
inline std::string assign_detect_refusal(const AssignRecord* rec, double threshold, bool out_null) {
    if (!rec || out_null) return "assignment or test is NULL";
    if (!assign_finite(threshold) || threshold < 0.0 || threshold > 1.0) return "threshold must be in [0, 1]";
    return "";
}
inline std::string assign_reindex_refusal(const double* A, int32_t test, bool out_null) {
    if (!A || out_null) return "A or out is NULL";
    if (test < 0 || test >= (int32_t)kAssignAbsenceTests) return "test must be in 0 .. 110, got " + std::to_string(test);
    return assign_finite_refusal(A, 9, "A");
}

}  // namespace ffsamd
