// ffs_shoebox.hip -- summation integration of shoeboxes in Kabsch space, from begin to end (include/ffs_hip.h has the definition, DESIGN.md
// section 3.8c the design, shoebox_model.hpp the rule, shoebox_plan.hpp the host's decisions, kernels_shoebox.hpp the kernel).  A job lives on
// a context: the table, the index over its z-ranges, the accumulators on the device and a non-blocking HIP stream of the job's own.  A fold
// runs after ffs_wait on the frames where the batch left them (cur_img, cur_pitch, cur_fstride), like ffs_stream_spot_backgrounds: it needs
// nothing from the batch's plan and changes none.  It is synchronous -- the list's copy and one launch in the job's stream, an event wait --
// and the whole of it is one step under the context's shoebox_mu, so two folds never overlap and a launch's waves own their shoeboxes.  The
// HIP streams a context shares between its ffs_streams are never touched.
#include "ffs_internal.hpp"
#include "kernels_shoebox.hpp"
#include "shoebox_plan.hpp"

static_assert(sizeof(ffs_scan_geometry) == 160 && sizeof(ShoeboxGeometry) == sizeof(ffs_scan_geometry), "ffs_scan_geometry is twenty doubles");
static_assert(offsetof(ffs_scan_geometry, pixel_size_mm) == offsetof(ShoeboxGeometry, pixel_size_mm) && offsetof(ffs_scan_geometry, wavelength) == offsetof(ShoeboxGeometry, wavelength)
                  && offsetof(ffs_scan_geometry, s0) == offsetof(ShoeboxGeometry, s0) && offsetof(ffs_scan_geometry, rot_axis) == offsetof(ShoeboxGeometry, rot_axis)
                  && offsetof(ffs_scan_geometry, osc_start_deg) == offsetof(ShoeboxGeometry, osc_start_deg)
                  && offsetof(ffs_scan_geometry, osc_width_deg) == offsetof(ShoeboxGeometry, osc_width_deg),
              "the model's geometry is ffs_scan_geometry");
static_assert(sizeof(ffs_shoebox) == 56 && sizeof(ShoeboxEntry) == sizeof(ffs_shoebox) && offsetof(ffs_shoebox, phi) == offsetof(ShoeboxEntry, phi)
                  && offsetof(ffs_shoebox, x_min) == offsetof(ShoeboxEntry, x_min) && offsetof(ffs_shoebox, z_max) == offsetof(ShoeboxEntry, z_max),
              "the model's table entry is ffs_shoebox");
static_assert(sizeof(ffs_shoebox_sum) == 80 && sizeof(ShoeboxSum) == sizeof(ffs_shoebox_sum) && offsetof(ffs_shoebox_sum, fg_count) == offsetof(ShoeboxSum, fg_count)
                  && offsetof(ffs_shoebox_sum, n_background) == offsetof(ShoeboxSum, n_background) && offsetof(ffs_shoebox_sum, n_overflow) == offsetof(ShoeboxSum, n_overflow)
                  && offsetof(ffs_shoebox_sum, flags) == offsetof(ShoeboxSum, flags) && offsetof(ffs_shoebox_sum, bg_status) == offsetof(ShoeboxSum, bg_status)
                  && offsetof(ffs_shoebox_sum, bg_mean) == offsetof(ShoeboxSum, bg_mean) && offsetof(ffs_shoebox_sum, intensity) == offsetof(ShoeboxSum, intensity)
                  && offsetof(ffs_shoebox_sum, variance) == offsetof(ShoeboxSum, variance),
              "the model's record is ffs_shoebox_sum");
static_assert(sizeof(ShoeboxAcc) == 48 && shoebox_state_bytes() == 1072, "1072 bytes of device state a shoebox");
static_assert(FFS_SHOEBOX_ELLIPSOID == kShoeboxEllipsoid && FFS_SHOEBOX_DIALS == kShoeboxDials && FFS_SHOEBOX_FG_INVALID == kShoeboxFgInvalid,
              "the constants of the header are the model's");

struct ShoeboxJob {
    ShoeboxGeometry geom{};
    int algorithm = kShoeboxEllipsoid;
    double ib = 0.0, im = 0.0;
    std::vector<ShoeboxEntry> table;
    ShoeboxIndex index;
    std::vector<uint32_t> list;        // the last fold's list (kept for its capacity)
    ShoeboxEntry* d_boxes = nullptr;
    ShoeboxAcc* d_acc = nullptr;
    uint32_t* d_hist = nullptr;
    uint32_t *d_list = nullptr, *h_list = nullptr;   // room for the whole table; h_list is pinned
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

// (the caller holds shoebox_mu, or is the context's destroy)
static void shoebox_job_free(ShoeboxJob* j) {
    if (!j) return;
    if (j->st) {
        (void)hipStreamSynchronize(j->st);   // (every fold has waited for its launch already)
        (void)hipStreamDestroy(j->st);
    }
    for (hipEvent_t& e : j->ev)
        if (e) (void)hipEventDestroy(e);
    if (j->d_boxes) (void)hipFree(j->d_boxes);
    if (j->d_acc) (void)hipFree(j->d_acc);
    if (j->d_hist) (void)hipFree(j->d_hist);
    if (j->d_list) (void)hipFree(j->d_list);
    if (j->h_list) (void)hipHostFree(j->h_list);
    delete j;
}

void shoebox_free_ctx(ffs_ctx* c) {
    shoebox_job_free(c->shoebox);
    c->shoebox = nullptr;
}

static int shoebox_begin_impl(ffs_ctx* c, const ffs_scan_geometry* geometry, const ffs_shoebox* shoeboxes, uint32_t n, int algorithm, double delta_b, double delta_m) {
    static const std::string who = "ffs_ctx_shoebox_begin: ";
    if (!geometry || (!shoeboxes && n > 0)) return refuse(c->err, FFS_ERR_INVALID, who + "geometry is NULL, or shoeboxes is NULL with n > 0");
    FFS_TRY(refuse_in_flight(c, "ffs_ctx_shoebox_begin", ""));
    std::lock_guard<std::mutex> lock(c->shoebox_mu);
    if (c->shoebox) return refuse(c->err, FFS_ERR_INVALID, who + "a job is open on this context (ffs_ctx_shoebox_end first)");
    ShoeboxGeometry g;
    std::memcpy(&g, geometry, sizeof g);
    const std::string job_why = shoebox_job_refusal(g, algorithm, delta_b, delta_m);
    if (!job_why.empty()) return refuse(c->err, FFS_ERR_INVALID, who + job_why);
    const ShoeboxEntry* table = reinterpret_cast<const ShoeboxEntry*>(shoeboxes);
    std::string why;
    const int64_t bad = shoebox_table_refusal(table, n, g.s0, c->L.W, c->L.H, why);
    if (bad >= 0) return refuse(c->err, FFS_ERR_INVALID, who + "shoebox " + std::to_string(bad) + " " + why);

    HIP_TRY(c, hipSetDevice(c->device));
    ShoeboxJob* j = new ShoeboxJob;
    j->geom = g;
    j->algorithm = algorithm;
    j->ib = shoebox_inverse_square(delta_b), j->im = shoebox_inverse_square(delta_m);
    j->table.assign(table, table + n);
    j->index.build(j->table.data(), n);
    const size_t rooms = std::max<size_t>(n, 1);
    auto fail = [&](int rc, const std::string& text) {
        (void)hipGetLastError();
        shoebox_job_free(j);
        return refuse(c->err, rc, who + text);
    };
    if (hipStreamCreateWithFlags(&j->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&j->ev[0]) != hipSuccess || hipEventCreate(&j->ev[1]) != hipSuccess)
        return fail(FFS_ERR_DEVICE, "the job's HIP stream and events could not be made");
    if (dmalloc(&j->d_boxes, rooms * sizeof(ShoeboxEntry)) != hipSuccess || dmalloc(&j->d_acc, rooms * sizeof(ShoeboxAcc)) != hipSuccess
        || dmalloc(&j->d_hist, rooms * (size_t)kSpotBgBins * sizeof(uint32_t)) != hipSuccess || dmalloc(&j->d_list, rooms * sizeof(uint32_t)) != hipSuccess
        || hipHostMalloc(reinterpret_cast<void**>(&j->h_list), rooms * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
        return fail(FFS_ERR_NOMEM, "the accumulators of " + std::to_string(n) + " shoeboxes (" + std::to_string((rooms * (shoebox_state_bytes() + sizeof(ShoeboxEntry) + 8)) >> 20)
                                       + " MB) do not fit");
    hipError_t e = hipSuccess;
    if (n) e = hipMemcpyAsync(j->d_boxes, j->table.data(), (size_t)n * sizeof(ShoeboxEntry), hipMemcpyHostToDevice, j->st);
    if (e == hipSuccess) e = hipMemsetAsync(j->d_acc, 0, rooms * sizeof(ShoeboxAcc), j->st);
    if (e == hipSuccess) e = hipMemsetAsync(j->d_hist, 0, rooms * (size_t)kSpotBgBins * sizeof(uint32_t), j->st);
    if (e == hipSuccess) e = hipStreamSynchronize(j->st);   // (the table's copy read the job's own vector)
    if (e != hipSuccess) return fail(FFS_ERR_DEVICE, std::string("the table's copy or the zeroing failed: ") + hipGetErrorString(e));
    c->shoebox = j;
    return FFS_OK;
}

extern "C" int ffs_ctx_shoebox_begin(ffs_ctx* c, const ffs_scan_geometry* geometry, const ffs_shoebox* shoeboxes, uint32_t n, int algorithm, double delta_b,
                                     double delta_m) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return shoebox_begin_impl(c, geometry, shoeboxes, n, algorithm, delta_b, delta_m); });
}

extern "C" int ffs_ctx_shoebox_end(ffs_ctx* c) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] {
        std::lock_guard<std::mutex> lock(c->shoebox_mu);
        if (!c->shoebox) return FFS_OK;
        HIP_TRY(c, hipSetDevice(c->device));
        shoebox_free_ctx(c);
        return FFS_OK;
    });
}

template <typename PixelT>
static void shoebox_launch(const ShoeboxJob* j, const ShoeboxArgs& a, dim3 grid) {
    if (j->algorithm == kShoeboxDials) hipExtLaunchKernelGGL((k_shoebox_fold<PixelT, kShoeboxDials>), grid, dim3(kShoeboxThreads), 0, j->st, j->ev[0], j->ev[1], 0, a);
    else hipExtLaunchKernelGGL((k_shoebox_fold<PixelT, kShoeboxEllipsoid>), grid, dim3(kShoeboxThreads), 0, j->st, j->ev[0], j->ev[1], 0, a);
}

static int shoebox_fold_impl(ffs_stream* s, int64_t first_image, float* kernel_ms) {
    static const std::string who = "ffs_stream_shoebox_fold: ";
    ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (s->busy) return refuse(c->err, FFS_ERR_INVALID, who + "a batch is in flight on this stream (its frames replace the last batch's): call it between ffs_wait and the next submit");
    if (!s->waited_ok) return refuse(c->err, FFS_ERR_INVALID, who + "no batch has been waited for on this stream yet, or its last ffs_wait failed");
    std::lock_guard<std::mutex> lock(c->shoebox_mu);
    ShoeboxJob* j = c->shoebox;
    if (!j) return refuse(c->err, FFS_ERR_INVALID, who + "no job is open on the context (ffs_ctx_shoebox_begin first; ffs_ctx_shoebox_end frees it)");
    if (first_image < 0 || first_image + (int64_t)s->n_frames > 0x7FFFFFFFll)
        return refuse(c->err, FFS_ERR_INVALID, who + "first_image must not be negative and the batch's last image must stay below 2^31, got " + std::to_string(first_image));
    if (!s->cur_img || s->n_frames == 0) return refuse(c->err, FFS_ERR_INVALID, who + "the stream does not hold the last batch's frames");
    j->index.query(first_image, first_image + (int64_t)s->n_frames, j->list);
    const size_t n_list = j->list.size();
    if (n_list == 0) return FFS_OK;

    HIP_TRY(c, hipSetDevice(c->device));
    std::memcpy(j->h_list, j->list.data(), n_list * sizeof(uint32_t));
    ShoeboxArgs a{};
    a.image = s->cur_img;
    a.frame_stride = s->cur_fstride;
    a.pitch = (uint32_t)s->cur_pitch;
    a.maskbits = c->d_maskbits;
    a.mpitch = L.mpitch;
    a.W = L.W;
    a.H = L.H;
    a.limit = counting_limit(s->batch.params.max_valid);
    a.n_frames = s->n_frames;
    a.first_image = first_image;
    a.n_list = (uint32_t)n_list;
    a.list = j->d_list;
    a.boxes = j->d_boxes;
    a.acc = j->d_acc;
    a.hist = j->d_hist;
    a.ib = j->ib;
    a.im = j->im;
    a.geom = j->geom;
    (void)hipGetLastError();
    HIP_TRY(c, hipMemcpyAsync(j->d_list, j->h_list, n_list * sizeof(uint32_t), hipMemcpyHostToDevice, j->st));
    const dim3 grid((uint32_t)((n_list + kShoeboxWaves - 1) / kShoeboxWaves));
    if (c->settings.pixel_bytes == 2) shoebox_launch<uint16_t>(j, a, grid);
    else shoebox_launch<uint32_t>(j, a, grid);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventSynchronize(j->ev[1]));
    if (kernel_ms) HIP_TRY(c, hipEventElapsedTime(kernel_ms, j->ev[0], j->ev[1]));
    return FFS_OK;
}

extern "C" int ffs_stream_shoebox_fold(ffs_stream* s, int64_t first_image, float* kernel_ms) {
    if (!s) {
        g_create_error = "ffs_stream_shoebox_fold: NULL stream handle";
        return FFS_ERR_INVALID;
    }
    if (!stream_handle_ok(s)) return FFS_ERR_INVALID;
    return guarded(s->ctx, [&] { return shoebox_fold_impl(s, first_image, kernel_ms); });
}

static int shoebox_sums_impl(ffs_ctx* c, int background_model, ffs_shoebox_sum* out, uint32_t cap, uint32_t* n) {
    static const std::string who = "ffs_ctx_get_shoebox_sums: ";
    if (!n || (!out && cap > 0)) return refuse(c->err, FFS_ERR_INVALID, who + "n is NULL, or out is NULL with cap > 0");
    if (background_model != kShoeboxBgTukey && background_model != kShoeboxBgGlm)
        return refuse(c->err, FFS_ERR_INVALID, who + "background_model must be 0 (Tukey fence) or 1 (robust Poisson GLM), got " + std::to_string(background_model));
    std::lock_guard<std::mutex> lock(c->shoebox_mu);
    const ShoeboxJob* j = c->shoebox;
    if (!j) return refuse(c->err, FFS_ERR_INVALID, who + "no job is open on the context (ffs_ctx_shoebox_begin first; ffs_ctx_shoebox_end frees it)");
    const size_t total = j->table.size(), take = std::min<size_t>(total, cap);
    *n = (uint32_t)total;
    if (take) {
        HIP_TRY(c, hipSetDevice(c->device));
        std::vector<ShoeboxAcc> acc(take);
        std::vector<uint32_t> hist(take * (size_t)kSpotBgBins);
        HIP_TRY(c, hipMemcpy(acc.data(), j->d_acc, take * sizeof(ShoeboxAcc), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(hist.data(), j->d_hist, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < take; ++i) {
            const ShoeboxSum r = shoebox_sum(acc[i], hist.data() + i * (size_t)kSpotBgBins, background_model);
            std::memcpy(&out[i], &r, sizeof r);
        }
    }
    if (total > cap) return refuse(c->err, FFS_ERR_OVERFLOW, who + std::to_string(total) + " records do not fit cap " + std::to_string(cap));
    return FFS_OK;
}

extern "C" int ffs_ctx_get_shoebox_sums(ffs_ctx* c, int background_model, ffs_shoebox_sum* out, uint32_t cap, uint32_t* n) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return shoebox_sums_impl(c, background_model, out, cap, n); });
}

extern "C" int ffs_ctx_get_shoebox_histogram(ffs_ctx* c, uint32_t index, uint32_t bins[256]) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] {
        static const std::string who = "ffs_ctx_get_shoebox_histogram: ";
        if (!bins) return refuse(c->err, FFS_ERR_INVALID, who + "bins is NULL");
        std::lock_guard<std::mutex> lock(c->shoebox_mu);
        const ShoeboxJob* j = c->shoebox;
        if (!j) return refuse(c->err, FFS_ERR_INVALID, who + "no job is open on the context (ffs_ctx_shoebox_begin first; ffs_ctx_shoebox_end frees it)");
        if (index >= j->table.size()) return refuse(c->err, FFS_ERR_INVALID, who + "index " + std::to_string(index) + " is outside the table of " + std::to_string(j->table.size()));
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMemcpy(bins, j->d_hist + (size_t)index * (size_t)kSpotBgBins, (size_t)kSpotBgBins * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return FFS_OK;
    });
}
