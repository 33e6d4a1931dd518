// ffs_predict.hip -- scan prediction for a rotation sweep: ffs_predict_scan_settings and ffs_ctx_predict (include/ffs_hip.h has the
// definition, DESIGN.md section 3.8d the design, predict_model.hpp the rule, predict_plan.hpp the host's decisions, kernels_predict.hpp the
// kernels).  A call is synchronous and owns what it uses: a non-blocking HIP stream, six events and four device buffers that the context
// keeps between calls (grown when a call needs more, freed with the context), all under the context's predict_mu, so two calls never
// overlap.  Nothing of a batch is read or written: no plan, no stream of the context's ffs_streams, no setting.
#include "ffs_internal.hpp"
#include "kernels_predict.hpp"
#include "predict_plan.hpp"

static_assert(sizeof(ffs_crystal) == 80 && sizeof(PredictCrystal) == sizeof(ffs_crystal) && offsetof(ffs_crystal, centring) == offsetof(PredictCrystal, centring),
              "the model's crystal is ffs_crystal");
static_assert(sizeof(ffs_prediction) == 96 && sizeof(PredictRecord) == sizeof(ffs_prediction) && offsetof(ffs_prediction, x_px) == offsetof(PredictRecord, x_px)
                  && offsetof(ffs_prediction, z) == offsetof(PredictRecord, z) && offsetof(ffs_prediction, h) == offsetof(PredictRecord, h)
                  && offsetof(ffs_prediction, flags) == offsetof(PredictRecord, flags),
              "the model's record is ffs_prediction");
static_assert(FFS_PREDICT_ENTERING == kPredictEntering && FFS_PREDICT_CORNER_LOST == kPredictCornerLost && FFS_PREDICT_ZETA_SMALL == kPredictZetaSmall
                  && FFS_PREDICT_BOX_REFUSED == kPredictBoxRefused && FFS_CENTRING_R == kPredictCentrings - 1,
              "the constants of the header are the model's");

struct PredictState {
    hipStream_t st = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double* d_settings = nullptr;
    uint32_t* d_counts = nullptr;
    uint64_t* d_offsets = nullptr;
    PredictRecord* d_out = nullptr;
    size_t settings_room = 0, counts_room = 0, offsets_room = 0, out_room = 0;   // in entries
};

void predict_free_ctx(ffs_ctx* c) {
    PredictState* p = c->predict;
    if (!p) return;
    if (p->st) {
        (void)hipStreamSynchronize(p->st);   // (every call has waited for its launches already)
        (void)hipStreamDestroy(p->st);
    }
    for (hipEvent_t& e : p->ev)
        if (e) (void)hipEventDestroy(e);
    if (p->d_settings) (void)hipFree(p->d_settings);
    if (p->d_counts) (void)hipFree(p->d_counts);
    if (p->d_offsets) (void)hipFree(p->d_offsets);
    if (p->d_out) (void)hipFree(p->d_out);
    delete p;
    c->predict = nullptr;
}

extern "C" int ffs_predict_scan_settings(const ffs_scan_geometry* geometry, const ffs_crystal* crystal, uint32_t n_images, double* out) {
    static const std::string who = "ffs_predict_scan_settings: ";
    return guarded(nullptr, [&] {
        if (!geometry || !crystal || !out) return refuse(g_create_error, FFS_ERR_INVALID, who + "geometry, crystal or out is NULL");
        ShoeboxGeometry g;
        PredictCrystal x;
        std::memcpy(&g, geometry, sizeof g);
        std::memcpy(&x, crystal, sizeof x);
        const std::string why = predict_settings_refusal(g, x, n_images);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, who + why);
        predict_scan_settings(g, x.a_matrix, n_images, out);
        return FFS_OK;
    });
}

// room for `want` entries behind *p (kept when it is there already)
template <typename T>
static int predict_room(ffs_ctx* c, T** p, size_t& room, size_t want, const char* what) {
    if (want <= room) return FFS_OK;
    if (*p) HIP_TRY(c, hipFree(*p));
    *p = nullptr, room = 0;
    if (dmalloc(p, want * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return refuse(c->err, FFS_ERR_NOMEM, std::string("ffs_ctx_predict: ") + what + " (" + std::to_string((want * sizeof(T)) >> 20) + " MB) do not fit");
    }
    room = want;
    return FFS_OK;
}

static int predict_impl(ffs_ctx* c, const ffs_scan_geometry* geometry, const ffs_crystal* crystal, uint32_t n_images, double dmin, double delta_b, double delta_m,
                        ffs_prediction* out, uint32_t cap, uint32_t* n, float* kernel_ms) {
    static const std::string who = "ffs_ctx_predict: ";
    if (kernel_ms) *kernel_ms = 0.0f;
    if (!geometry || !crystal || !n || (!out && cap > 0)) return refuse(c->err, FFS_ERR_INVALID, who + "geometry, crystal or n is NULL, or out is NULL with cap > 0");
    ShoeboxGeometry g;
    PredictCrystal x;
    std::memcpy(&g, geometry, sizeof g);
    std::memcpy(&x, crystal, sizeof x);
    PredictArgs a{};
    const std::string why = predict_refusal(g, x, n_images, dmin, delta_b, delta_m, c->L.W, c->L.H, a.u);
    if (!why.empty()) return refuse(c->err, FFS_ERR_INVALID, who + why);
    std::vector<double> settings(((size_t)n_images + 1) * 9);
    predict_scan_settings(g, x.a_matrix, n_images, settings.data());

    std::lock_guard<std::mutex> lock(c->predict_mu);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->predict) c->predict = new PredictState;
    PredictState* p = c->predict;
    if (!p->st) HIP_TRY(c, hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
    for (hipEvent_t& e : p->ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    a.n_blocks = predict_blocks(a.u.n_candidates);
    FFS_TRY(predict_room(c, &p->d_settings, p->settings_room, settings.size(), "the scan-point settings"));
    FFS_TRY(predict_room(c, &p->d_counts, p->counts_room, (size_t)a.n_blocks, "the workgroups' counts"));
    FFS_TRY(predict_room(c, &p->d_offsets, p->offsets_room, (size_t)a.n_blocks + 1, "the workgroups' offsets"));
    a.settings = p->d_settings;
    a.counts = p->d_counts;
    a.offsets = p->d_offsets;
    (void)hipGetLastError();
    HIP_TRY(c, hipMemcpyAsync(p->d_settings, settings.data(), settings.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    hipExtLaunchKernelGGL(k_predict_count, dim3(a.n_blocks), dim3(kPredictThreads), 0, p->st, p->ev[0], p->ev[1], 0, a);
    HIP_TRY(c, hipGetLastError());
    hipExtLaunchKernelGGL(k_predict_scan, dim3(1), dim3(kPredictScanThreads), 0, p->st, p->ev[2], p->ev[3], 0, a);
    HIP_TRY(c, hipGetLastError());
    uint64_t total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, p->d_offsets + a.n_blocks, sizeof total, hipMemcpyDeviceToHost, p->st));
    HIP_TRY(c, hipStreamSynchronize(p->st));
    float ms[3] = {0.0f, 0.0f, 0.0f};
    if (kernel_ms) {
        HIP_TRY(c, hipEventElapsedTime(&ms[0], p->ev[0], p->ev[1]));
        HIP_TRY(c, hipEventElapsedTime(&ms[1], p->ev[2], p->ev[3]));
    }
    if (total > 0xFFFFFFFFull) return refuse(c->err, FFS_ERR_OVERFLOW, who + std::to_string(total) + " predictions do not fit a 32-bit count");
    *n = (uint32_t)total;
    const size_t take = (size_t)std::min<uint64_t>(total, cap);
    if (take) {
        FFS_TRY(predict_room(c, &p->d_out, p->out_room, take, "the records"));
        a.out = p->d_out;
        a.cap = take;
        hipExtLaunchKernelGGL(k_predict_write, dim3(a.n_blocks), dim3(kPredictThreads), 0, p->st, p->ev[4], p->ev[5], 0, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(out, p->d_out, take * sizeof(PredictRecord), hipMemcpyDeviceToHost, p->st));
        HIP_TRY(c, hipStreamSynchronize(p->st));
        if (kernel_ms) HIP_TRY(c, hipEventElapsedTime(&ms[2], p->ev[4], p->ev[5]));
    }
    if (kernel_ms) *kernel_ms = (ms[0] + ms[1]) + ms[2];
    if (total > cap) return refuse(c->err, FFS_ERR_OVERFLOW, who + std::to_string(total) + " records do not fit cap " + std::to_string(cap));
    return FFS_OK;
}

extern "C" int ffs_ctx_predict(ffs_ctx* c, const ffs_scan_geometry* geometry, const ffs_crystal* crystal, uint32_t n_images, double dmin, double delta_b, double delta_m,
                               ffs_prediction* out, uint32_t cap, uint32_t* n, float* kernel_ms) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return predict_impl(c, geometry, crystal, n_images, dmin, delta_b, delta_m, out, cap, n, kernel_ms); });
}
