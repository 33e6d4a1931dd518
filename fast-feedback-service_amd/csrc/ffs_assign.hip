// ffs_assign.hip -- index assignment for candidate crystal settings: the host-only entries ffs_index_select / settings / absence_table /
// absence_detect / reindex and the device entry ffs_ctx_index_assign (include/ffs_hip.h has the definition, DESIGN.md section 3.8f the
// design, assign_model.hpp the rule, assign_plan.hpp the host's decisions and the bytes, kernels_assign.hpp the kernels).  The call is
// synchronous and owns what it uses: a non-blocking HIP stream and four events kept on the context, and device buffers that live for the
// call, under the context's assign_mu, so two calls never overlap.  Nothing of a batch is read or written: no plan, no stream of the
// context's ffs_streams, no setting.
#include "ffs_internal.hpp"
#include "kernels_assign.hpp"

static_assert(sizeof(ffs_index_assignment) == sizeof(AssignRecord) && offsetof(ffs_index_assignment, sum_lsq_q40) == offsetof(AssignRecord, sum_lsq_q40) &&
                  offsetof(ffs_index_assignment, absent0) == offsetof(AssignRecord, absent0),
              "the model's record is ffs_index_assignment");
static_assert(sizeof(ffs_index_absence_test) == sizeof(AssignAbsenceTest) && offsetof(ffs_index_absence_test, transform) == offsetof(AssignAbsenceTest, transform),
              "the model's test is ffs_index_absence_test");
static_assert(sizeof(ffs_index_setting) == sizeof(AssignSetting) && offsetof(ffs_index_setting, A) == offsetof(AssignSetting, A), "the model's setting is ffs_index_setting");
static_assert(FFS_INDEX_ABSENCE_TESTS == kAssignAbsenceTests && FFS_INDEX_ASSIGN_SINGULAR == kAssignSingular, "ffs_hip.h's constants");

struct AssignState {
    hipStream_t st = nullptr;
    hipEvent_t lap[4] = {nullptr, nullptr, nullptr, nullptr};   // around the three stages of a pass
    float launch_ms[3] = {0.0f, 0.0f, 0.0f};                    // of the last call, over its passes
};

void assign_free_ctx(ffs_ctx* c) {
    AssignState* p = c->assign;
    if (!p) return;
    if (p->st) {
        (void)hipStreamSynchronize(p->st);   // (every call has waited for its launches already)
        (void)hipStreamDestroy(p->st);
    }
    for (hipEvent_t& e : p->lap)
        if (e) (void)hipEventDestroy(e);
    delete p;
    c->assign = nullptr;
}

// ---- host only, no context -------------------------------------------------------------------------------------------------------------------
extern "C" int ffs_index_select(const double* rlp, const double* phi, uint32_t n, double dmin, double osc_start_deg, uint8_t* selected) {
    return guarded(nullptr, [&] {
        const std::string why = assign_select_refusal(rlp, phi, n, dmin, osc_start_deg, !selected);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_select: " + why);
        for (uint32_t i = 0; i < n; ++i) selected[i] = assign_selected(rlp + 3 * (size_t)i, phi[i], dmin, osc_start_deg) ? 1 : 0;
        return FFS_OK;
    });
}

extern "C" int ffs_index_settings(const double* vectors, uint32_t n, uint32_t max_combinations, ffs_index_setting* out, uint32_t cap, uint32_t* n_out) {
    return guarded(nullptr, [&] {
        const std::string why = assign_settings_refusal(vectors, n, max_combinations, !out, cap, !n_out);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_settings: " + why);
        const std::vector<AssignSetting> v = assign_settings(vectors, n, max_combinations);
        *n_out = (uint32_t)v.size();
        const size_t take = std::min<size_t>(v.size(), cap);
        if (take) std::memcpy(out, v.data(), take * sizeof(AssignSetting));
        if (v.size() > cap) return refuse(g_create_error, FFS_ERR_OVERFLOW, "ffs_index_settings: " + std::to_string(v.size()) + " settings do not fit cap " + std::to_string(cap));
        return FFS_OK;
    });
}

extern "C" int ffs_index_absence_table(ffs_index_absence_test* out) {
    return guarded(nullptr, [&] {
        if (!out) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_absence_table: out is NULL");
        const std::vector<AssignAbsenceTest> t = assign_absence_table();
        std::memcpy(out, t.data(), t.size() * sizeof(AssignAbsenceTest));
        return FFS_OK;
    });
}

extern "C" int ffs_index_absence_detect(const ffs_index_assignment* assignment, double threshold, int32_t* test) {
    return guarded(nullptr, [&] {
        const AssignRecord* rec = reinterpret_cast<const AssignRecord*>(assignment);
        const std::string why = assign_detect_refusal(rec, threshold, !test);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_absence_detect: " + why);
        *test = assign_detect(*rec, threshold);
        return FFS_OK;
    });
}

extern "C" int ffs_index_reindex(const double* A, int32_t test, double* A_out) {
    return guarded(nullptr, [&] {
        const std::string why = assign_reindex_refusal(A, test, !A_out);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_reindex: " + why);
        const std::vector<AssignAbsenceTest> t = assign_absence_table();
        double out[9];
        if (!assign_reindex(A, t[(size_t)test].transform, out)) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_reindex: A is singular");
        std::memcpy(A_out, out, sizeof out);
        return FFS_OK;
    });
}

// ---- device ------------------------------------------------------------------------------------------------------------------------------------
namespace {
// device buffers of one call: freed when the call returns, whichever way
struct AssignBuffers {
    std::vector<void*> all;
    ~AssignBuffers() {
        for (void* d : all)
            if (d) (void)hipFree(d);
    }
    template <typename T>
    int room(ffs_ctx* c, T** p, size_t entries, const char* what) {
        *p = nullptr;
        if (entries == 0u) entries = 1u;
        if (dmalloc(p, entries * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            return refuse(c->err, FFS_ERR_NOMEM, std::string("ffs_ctx_index_assign: ") + what + " (" + std::to_string((entries * sizeof(T)) >> 20) + " MB) do not fit");
        }
        all.push_back(*p);
        return FFS_OK;
    }
};
}  // namespace

static int index_assign_impl(ffs_ctx* c, const double* rlp, const double* phi, const uint8_t* selected, uint32_t n, const double* A, uint32_t n_candidates, double tolerance,
                             size_t workspace_bytes, ffs_index_assignment* out, int32_t* hkl, double* lsq) {
    static const char* who = "ffs_ctx_index_assign: ";
    const std::string why = assign_refusal(rlp, phi, n, A, n_candidates, tolerance, !out);
    if (!why.empty()) return refuse(c->err, FFS_ERR_INVALID, who + why);
    const bool want_hkl = hkl != nullptr, want_lsq = lsq != nullptr;
    const uint32_t per_pass = assign_pass_settings(n, n_candidates, workspace_bytes, want_hkl, want_lsq);
    if (n_candidates > 0u && per_pass == 0u)
        return refuse(c->err, FFS_ERR_NOMEM, who + std::string("one setting of ") + std::to_string(n) + " spots needs " + std::to_string(assign_setting_bytes(n, want_hkl, want_lsq)) +
                                                 " bytes of device state, workspace_bytes is " + std::to_string(workspace_bytes));
    std::lock_guard<std::mutex> lock(c->assign_mu);
    if (!c->assign) c->assign = new AssignState;
    AssignState* p = c->assign;
    for (float& v : p->launch_ms) v = 0.0f;
    if (n_candidates == 0u) return FFS_OK;

    // the settings' inverses and status, by the header's text on the host: wave-uniform constants of the launches
    std::vector<AssignRecord> recs(n_candidates);
    std::vector<double> inv(9 * (size_t)n_candidates);
    std::memset(recs.data(), 0, recs.size() * sizeof(AssignRecord));
    for (uint32_t k = 0; k < n_candidates; ++k)
        if (!assign_inverse(A + 9 * (size_t)k, &inv[9 * (size_t)k])) recs[k].status = kAssignSingular;
    if (n == 0u) {   // nothing to launch: every count is zero
        std::memcpy(out, recs.data(), recs.size() * sizeof(AssignRecord));
        return FFS_OK;
    }
    std::vector<double> planes(4 * (size_t)n);
    std::vector<uint8_t> sel(n, 1);
    for (uint32_t i = 0; i < n; ++i) {
        planes[i] = rlp[3 * (size_t)i], planes[(size_t)n + i] = rlp[3 * (size_t)i + 1], planes[2 * (size_t)n + i] = rlp[3 * (size_t)i + 2], planes[3 * (size_t)n + i] = phi[i];
        if (selected) sel[i] = selected[i] ? 1 : 0;
    }

    HIP_TRY(c, hipSetDevice(c->device));
    if (!p->st) HIP_TRY(c, hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
    for (hipEvent_t& e : p->lap)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    (void)hipGetLastError();
    const uint32_t T = assign_table_slots(n);
    AssignBuffers buf;
    double *d_planes = nullptr, *d_inv = nullptr, *d_lsq = nullptr;
    uint8_t* d_sel = nullptr;
    AssignRecord* d_rec = nullptr;
    unsigned long long *d_words = nullptr, *d_keys = nullptr;
    uint32_t *d_counts = nullptr, *d_places = nullptr, *d_cursor = nullptr, *d_met = nullptr, *d_sorted = nullptr;
    int32_t* d_hkl = nullptr;
    FFS_TRY(buf.room(c, &d_planes, 4 * (size_t)n, "the spots"));
    FFS_TRY(buf.room(c, &d_sel, (size_t)n, "the selection"));
    FFS_TRY(buf.room(c, &d_inv, inv.size(), "the settings"));
    FFS_TRY(buf.room(c, &d_rec, recs.size(), "the records"));
    FFS_TRY(buf.room(c, &d_words, (size_t)per_pass * n, "the pairs' words"));
    FFS_TRY(buf.room(c, &d_keys, (size_t)per_pass * T, "the key tables"));
    FFS_TRY(buf.room(c, &d_counts, (size_t)per_pass * T, "the key tables' counts"));
    FFS_TRY(buf.room(c, &d_places, (size_t)per_pass * T, "the groups' places"));
    FFS_TRY(buf.room(c, &d_cursor, (size_t)per_pass, "the cursors"));
    FFS_TRY(buf.room(c, &d_met, (size_t)per_pass * n, "the groups' members"));
    FFS_TRY(buf.room(c, &d_sorted, (size_t)per_pass * n, "the groups' sorted members"));
    if (want_hkl) FFS_TRY(buf.room(c, &d_hkl, 3 * (size_t)per_pass * n, "the indices"));
    if (want_lsq) FFS_TRY(buf.room(c, &d_lsq, (size_t)per_pass * n, "the lsq"));

    HIP_TRY(c, hipMemcpyAsync(d_planes, planes.data(), planes.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIP_TRY(c, hipMemcpyAsync(d_sel, sel.data(), sel.size(), hipMemcpyHostToDevice, p->st));
    HIP_TRY(c, hipMemcpyAsync(d_inv, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    HIP_TRY(c, hipMemcpyAsync(d_rec, recs.data(), recs.size() * sizeof(AssignRecord), hipMemcpyHostToDevice, p->st));

    AssignArgs a{};
    a.r0 = d_planes, a.r1 = d_planes + n, a.r2 = d_planes + 2 * (size_t)n, a.phi = d_planes + 3 * (size_t)n, a.sel = d_sel, a.inv = d_inv, a.rec = d_rec;
    a.n = n, a.slots = T, a.tol_sq = tolerance * tolerance;
    a.words = d_words, a.keys = d_keys, a.counts = d_counts, a.places = d_places, a.cursor = d_cursor, a.met = d_met, a.sorted = d_sorted, a.hkl = d_hkl, a.lsq = d_lsq;
    const dim3 threads(kAssignThreads);
    for (uint32_t first = 0; first < n_candidates; first += per_pass) {
        const uint32_t P = std::min(per_pass, n_candidates - first);
        a.first = first;
        const dim3 pairs(assign_spot_blocks(n), P), slots(assign_slot_blocks(n), P);
        HIP_TRY(c, hipMemsetAsync(d_keys, 0, (size_t)P * T * sizeof(unsigned long long), p->st));
        HIP_TRY(c, hipMemsetAsync(d_counts, 0, (size_t)P * T * sizeof(uint32_t), p->st));
        HIP_TRY(c, hipMemsetAsync(d_cursor, 0, (size_t)P * sizeof(uint32_t), p->st));
        HIP_TRY(c, hipEventRecord(p->lap[0], p->st));
        hipLaunchKernelGGL(k_assign, pairs, threads, 0, p->st, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(p->lap[1], p->st));
        hipLaunchKernelGGL(k_assign_place, slots, threads, 0, p->st, a);
        hipLaunchKernelGGL(k_assign_fill, pairs, threads, 0, p->st, a);
        hipLaunchKernelGGL(k_assign_resolve, slots, threads, 0, p->st, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(p->lap[2], p->st));
        hipLaunchKernelGGL(k_assign_reduce, pairs, threads, 0, p->st, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(p->lap[3], p->st));
        if (want_hkl) HIP_TRY(c, hipMemcpyAsync(hkl + 3 * (size_t)first * n, d_hkl, 3 * (size_t)P * n * sizeof(int32_t), hipMemcpyDeviceToHost, p->st));
        if (want_lsq) HIP_TRY(c, hipMemcpyAsync(lsq + (size_t)first * n, d_lsq, (size_t)P * n * sizeof(double), hipMemcpyDeviceToHost, p->st));
        HIP_TRY(c, hipStreamSynchronize(p->st));
        for (int k = 0; k < 3; ++k) {
            float ms = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms, p->lap[k], p->lap[k + 1]));
            p->launch_ms[k] += ms;
        }
    }
    HIP_TRY(c, hipMemcpyAsync(recs.data(), d_rec, recs.size() * sizeof(AssignRecord), hipMemcpyDeviceToHost, p->st));
    HIP_TRY(c, hipStreamSynchronize(p->st));
    std::memcpy(out, recs.data(), recs.size() * sizeof(AssignRecord));
    return FFS_OK;
}

extern "C" int ffs_ctx_index_assign(ffs_ctx* c, const double* rlp, const double* phi, const uint8_t* selected, uint32_t n, const double* A, uint32_t n_candidates,
                                    double tolerance, size_t workspace_bytes, ffs_index_assignment* out, int32_t* hkl, double* lsq) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return index_assign_impl(c, rlp, phi, selected, n, A, n_candidates, tolerance, workspace_bytes, out, hkl, lsq); });
}

extern "C" int ffs_ctx_index_assign_launch_ms(ffs_ctx* c, float* out) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] {
        if (!out) return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_index_assign_launch_ms: out is NULL");
        std::lock_guard<std::mutex> lock(c->assign_mu);
        for (int k = 0; k < 3; ++k) out[k] = c->assign ? c->assign->launch_ms[k] : 0.0f;
        return FFS_OK;
    });
}
