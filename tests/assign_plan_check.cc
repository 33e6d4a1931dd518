// assign_plan_check.cc -- csrc/assign_plan.hpp as a stand-alone program (tests/test_assign_plan.py builds it under the address and
// undefined-behaviour sanitizers): every refusal with its text, the key table's size, the bytes of a setting, the settings a pass takes at
// the boundaries (1, one less than a pass, a pass, one more), and the launches' shapes, all against values computed by hand.
#include <math.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "assign_plan.hpp"

using namespace ffsamd;

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                             \
        }                                                           \
    } while (0)

static bool has(const std::string& s, const char* needle) { return s.find(needle) != std::string::npos; }

int main() {
    // the key table: the power of two >= 2 n, at least 256
    CHECK(assign_table_slots(0) == 256u && assign_table_slots(1) == 256u && assign_table_slots(128) == 256u && assign_table_slots(129) == 512u);
    CHECK(assign_table_slots(709) == 2048u && assign_table_slots(4093) == 8192u && assign_table_slots(4096) == 8192u && assign_table_slots(4097) == 16384u);
    CHECK(assign_table_slots(kAssignMaxSpots) == (1u << 21));
    // bytes of a setting: 16 n + 16 T + 4, hkl 12 n, lsq 8 n
    CHECK(assign_setting_bytes(709, false, false) == 44116u);
    CHECK(assign_setting_bytes(709, true, false) == 44116u + 8508u);
    CHECK(assign_setting_bytes(709, false, true) == 44116u + 5672u);
    CHECK(assign_setting_bytes(709, true, true) == 58296u);
    CHECK(assign_setting_bytes(0, true, true) == 4100u);
    CHECK(assign_setting_bytes(kAssignMaxSpots, true, true) == 36u * 1048576u + 16u * 2097152u + 4u);
    // settings a pass: a workspace of exactly ten settings of 709 spots
    const size_t ten = 441160u;
    CHECK(assign_pass_settings(709, 1, ten, false, false) == 1u && assign_passes(1, 1) == 1u);
    CHECK(assign_pass_settings(709, 9, ten, false, false) == 9u && assign_passes(9, 9) == 1u);
    CHECK(assign_pass_settings(709, 10, ten, false, false) == 10u && assign_passes(10, 10) == 1u);
    CHECK(assign_pass_settings(709, 11, ten, false, false) == 10u && assign_passes(11, 10) == 2u);
    CHECK(assign_pass_settings(709, 20, ten, false, false) == 10u && assign_passes(20, 10) == 2u && assign_passes(21, 10) == 3u);
    CHECK(assign_pass_settings(709, 11, ten - 1u, false, false) == 9u);
    CHECK(assign_pass_settings(709, 11, ten, true, true) == 7u);          // 441160 / 58296 = 7.56
    CHECK(assign_pass_settings(709, 5, 44116u, false, false) == 1u);      // the floor: one setting a pass
    CHECK(assign_pass_settings(709, 5, 44115u, false, false) == 0u);      // not even one
    CHECK(assign_pass_settings(709, 5, 1u, false, false) == 0u);
    CHECK(assign_pass_settings(709, 4096, 0u, false, false) == 4096u);    // the default, 256 MiB: 268435456 / 44116 = 6084
    CHECK(assign_pass_settings(709, 0, 0u, false, false) == 0u && assign_passes(0, 0) == 0u);
    CHECK(assign_pass_settings(kAssignMaxSpots, 4096, 0u, false, false) == 5u);   // 268435456 / 50331652 = 5.33
    CHECK(kAssignDefaultWorkspace == 268435456u);
    // the launches
    CHECK(assign_spot_blocks(0) == 0u && assign_spot_blocks(1) == 1u && assign_spot_blocks(256) == 1u && assign_spot_blocks(257) == 2u && assign_spot_blocks(709) == 3u);
    CHECK(assign_slot_blocks(1) == 1u && assign_slot_blocks(709) == 8u && assign_slot_blocks(kAssignMaxSpots) == 8192u);
    CHECK(kAssignThreads == 256 && kAssignMaxCandidates == 4096u && kAssignMaxSpots == 1048576u);

    // the refusals of ffs_ctx_index_assign
    const double rlp[6] = {0.1, 0.2, 0.3, 0.0, 0.0, 0.0}, phi[2] = {0.0, 1.0}, A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(assign_refusal(rlp, phi, 2, A, 1, 0.3, false).empty());
    CHECK(assign_refusal(nullptr, nullptr, 0, nullptr, 0, 0.3, true).empty());   // n = 0 and n_candidates = 0 are allowed
    CHECK(assign_refusal(nullptr, nullptr, 0, A, 1, 0.3, false).empty());
    CHECK(assign_refusal(rlp, phi, 2, nullptr, 0, 0.3, true).empty());
    CHECK(has(assign_refusal(nullptr, phi, 2, A, 1, 0.3, false), "rlp or phi is NULL"));
    CHECK(has(assign_refusal(rlp, nullptr, 2, A, 1, 0.3, false), "rlp or phi is NULL"));
    CHECK(has(assign_refusal(rlp, phi, 2, nullptr, 1, 0.3, false), "A or out is NULL"));
    CHECK(has(assign_refusal(rlp, phi, 2, A, 1, 0.3, true), "A or out is NULL"));
    CHECK(has(assign_refusal(rlp, phi, kAssignMaxSpots + 1u, A, 1, 0.3, false), "n must be at most 1048576, got 1048577"));
    CHECK(has(assign_refusal(rlp, phi, 2, A, 4097, 0.3, false), "n_candidates must be at most 4096, got 4097"));
    for (double bad : {0.0, -0.1, 0.5000000000000001, 1.0, (double)INFINITY, (double)NAN}) CHECK(has(assign_refusal(rlp, phi, 2, A, 1, bad, false), "tolerance must be in (0, 0.5]"));
    CHECK(assign_refusal(rlp, phi, 2, A, 1, 0.5, false).empty() && assign_refusal(rlp, phi, 2, A, 1, 5e-324, false).empty());
    for (double bad : {(double)INFINITY, -(double)INFINITY, (double)NAN}) {
        double r[6] = {0.1, 0.2, 0.3, 0.0, bad, 0.0}, p[2] = {0.0, bad}, a[9] = {1, 0, 0, 0, 1, 0, 0, 0, bad};
        CHECK(has(assign_refusal(r, phi, 2, A, 1, 0.3, false), "rlp has an entry that is not finite"));
        CHECK(has(assign_refusal(rlp, p, 2, A, 1, 0.3, false), "phi has an entry that is not finite"));
        CHECK(has(assign_refusal(rlp, phi, 2, a, 1, 0.3, false), "A has an entry that is not finite"));
        CHECK(has(assign_select_refusal(r, phi, 2, 2.0, 0.0, false), "rlp has an entry"));
        CHECK(has(assign_select_refusal(rlp, p, 2, 2.0, 0.0, false), "phi has an entry"));
        CHECK(has(assign_select_refusal(rlp, phi, 2, bad, 0.0, false), "dmin must be finite and not negative"));
        CHECK(has(assign_select_refusal(rlp, phi, 2, 2.0, bad, false), "osc_start_deg must be finite"));
        CHECK(has(assign_settings_refusal(r, 2, 1000, false, 4, false), "vectors has an entry that is not finite"));
        CHECK(has(assign_reindex_refusal(a, 0, false), "A has an entry that is not finite"));
    }
    // ... and of the host-only entries
    CHECK(assign_select_refusal(rlp, phi, 2, 0.0, 0.0, false).empty() && assign_select_refusal(nullptr, nullptr, 0, 2.0, 0.0, true).empty());
    CHECK(has(assign_select_refusal(rlp, phi, 2, 2.0, 0.0, true), "NULL") && has(assign_select_refusal(rlp, phi, 2, -1.0, 0.0, false), "dmin"));
    CHECK(assign_settings_refusal(rlp, 2, 1000, false, 4, false).empty() && assign_settings_refusal(rlp, 2, 1000, true, 0, false).empty());
    CHECK(has(assign_settings_refusal(rlp, 2, 1000, true, 4, false), "NULL") && has(assign_settings_refusal(rlp, 2, 1000, false, 4, true), "NULL"));
    CHECK(has(assign_settings_refusal(nullptr, 2, 1000, false, 4, false), "NULL") && has(assign_settings_refusal(rlp, 2, 0, false, 4, false), "max_combinations must be positive"));
    AssignRecord rec{};
    CHECK(assign_detect_refusal(&rec, 0.9, false).empty() && has(assign_detect_refusal(nullptr, 0.9, false), "NULL") && has(assign_detect_refusal(&rec, 0.9, true), "NULL"));
    CHECK(has(assign_detect_refusal(&rec, 1.5, false), "threshold must be in [0, 1]") && has(assign_detect_refusal(&rec, (double)NAN, false), "threshold"));
    CHECK(assign_reindex_refusal(A, 0, false).empty() && assign_reindex_refusal(A, 110, false).empty());
    CHECK(has(assign_reindex_refusal(A, 111, false), "test must be in 0 .. 110, got 111") && has(assign_reindex_refusal(A, -1, false), "got -1"));
    CHECK(has(assign_reindex_refusal(nullptr, 0, false), "NULL") && has(assign_reindex_refusal(A, 0, true), "NULL"));
    if (failures == 0) printf("ok\n");
    return failures ? 1 : 0;
}
