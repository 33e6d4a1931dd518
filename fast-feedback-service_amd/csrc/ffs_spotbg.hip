// ffs_spotbg.hip -- ffs_stream_spot_backgrounds: the per-spot constant background of the last batch ffs_wait returned on a stream
// (include/ffs_hip.h has the definition, DESIGN.md section 3.8 the design, kernels_spotbg.hpp the kernel).  The call runs after ffs_wait on
// what the host already holds -- the stream's reflections and per-frame counts -- and on the frames where the batch left them (cur_img,
// cur_pitch, cur_fstride), so it needs nothing from the batch's plan and changes none.  It is synchronous: one copy of the boxes to the
// device and one launch in a non-blocking HIP stream of the ffs_stream's own, an event wait, the means divided on the host.  The HIP streams
// a context shares between its ffs_streams are never touched.  The reference estimates the same model per 3D shoebox at integration time
// (integrator/background.hpp); it has no counterpart at spot-finding time.
// ffs_stream_spot_backgrounds_glm is the same call under the reference's second model, the robust Poisson GLM (DESIGN.md section 3.8b,
// spot_background_glm_model.hpp): the preconditions, the boxes, the launch and the wait are one function for both, spot_backgrounds_run;
// the GLM kernel stores whole records into a pinned buffer of the GLM call's own, and the host computes nothing afterwards.
#include "ffs_internal.hpp"
#include "kernels_spotbg.hpp"

static_assert(sizeof(ffs_spot_background) == 48 && sizeof(SpotBgOut) == sizeof(ffs_spot_background), "ffs_spot_background is 48 bytes");
static_assert(offsetof(ffs_spot_background, n_pixels) == offsetof(SpotBgOut, n_pixels) && offsetof(ffs_spot_background, q1) == offsetof(SpotBgOut, q1)
                  && offsetof(ffs_spot_background, n_inliers) == offsetof(SpotBgOut, n_inliers)
                  && offsetof(ffs_spot_background, inlier_sum) == offsetof(SpotBgOut, inlier_sum) && offsetof(ffs_spot_background, status) == offsetof(SpotBgOut, status)
                  && offsetof(ffs_spot_background, mean) == offsetof(SpotBgOut, mean),
              "the kernel's record is ffs_spot_background");
static_assert(sizeof(SpotBgBox) == 16, "a box is one 16-byte load");
static_assert(FFS_SPOT_BG_OK == kSpotBgOk && FFS_SPOT_BG_NO_PIXELS == kSpotBgNoPixels && FFS_SPOT_BG_OVERFLOW == kSpotBgOverflow
                  && FFS_SPOT_BG_RANGE == kSpotBgRange && FFS_SPOT_BG_NO_INLIERS == kSpotBgNoInliers,
              "the status codes of the header are the model's");
static_assert(sizeof(ffs_spot_background_glm) == 40 && sizeof(SpotBgGlmOut) == sizeof(ffs_spot_background_glm), "ffs_spot_background_glm is 40 bytes");
static_assert(offsetof(ffs_spot_background_glm, n_pixels) == offsetof(SpotBgGlmOut, n_pixels) && offsetof(ffs_spot_background_glm, median) == offsetof(SpotBgGlmOut, median)
                  && offsetof(ffs_spot_background_glm, n_iter) == offsetof(SpotBgGlmOut, n_iter) && offsetof(ffs_spot_background_glm, status) == offsetof(SpotBgGlmOut, status)
                  && offsetof(ffs_spot_background_glm, beta) == offsetof(SpotBgGlmOut, beta) && offsetof(ffs_spot_background_glm, mean) == offsetof(SpotBgGlmOut, mean),
              "the GLM kernel's record is ffs_spot_background_glm");
static_assert(FFS_SPOT_BG_FEW_PIXELS == kSpotBgFewPixels && FFS_SPOT_BG_DEGENERATE == kSpotBgDegenerate && FFS_SPOT_BG_NOT_CONVERGED == kSpotBgNotConverged,
              "the GLM status codes of the header are the model's");

void spotbg_free(ffs_stream* s) {
    if (s->bg_st) {
        (void)hipStreamSynchronize(s->bg_st);   // (the ffs_stream's own; every call has waited for its launch already)
        (void)hipStreamDestroy(s->bg_st);
    }
    for (hipEvent_t& e : s->bg_ev)
        if (e) (void)hipEventDestroy(e);
    if (s->h_bg_boxes) (void)hipHostFree(s->h_bg_boxes);
    if (s->h_bg_out) (void)hipHostFree(s->h_bg_out);
    if (s->d_bg_boxes) (void)hipFree(s->d_bg_boxes);
    if (s->h_bg_glm_out) (void)hipHostFree(s->h_bg_glm_out);
    s->h_bg_glm_out = s->h_bg_glm_out_dev = nullptr;
    s->bg_glm_cap = 0;
    s->bg_st = nullptr;
    s->bg_ev[0] = s->bg_ev[1] = nullptr;
    s->h_bg_boxes = s->d_bg_boxes = nullptr;
    s->h_bg_out = s->h_bg_out_dev = nullptr;
    s->bg_cap = 0;
}

// The stream's own HIP stream and events (first call), and room for n reflections (first call, or a batch with more than any before: what
// the previous call handed out is freed here, as the header allows)
static int spotbg_ensure(ffs_stream* s, uint32_t n, const char* who) {
    ffs_ctx* c = s->ctx;
    if (!s->bg_st) HIP_TRY(c, hipStreamCreateWithFlags(&s->bg_st, hipStreamNonBlocking));
    for (hipEvent_t& e : s->bg_ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    if (n <= s->bg_cap) return FFS_OK;
    if (s->h_bg_boxes) (void)hipHostFree(s->h_bg_boxes);
    if (s->h_bg_out) (void)hipHostFree(s->h_bg_out);
    if (s->d_bg_boxes) (void)hipFree(s->d_bg_boxes);
    s->h_bg_boxes = s->d_bg_boxes = nullptr;
    s->h_bg_out = s->h_bg_out_dev = nullptr;
    s->bg_cap = 0;
    const uint32_t cap = std::max<uint32_t>(1024u, n + n / 4);
    if (hipHostMalloc(&s->h_bg_boxes, (size_t)cap * sizeof(SpotBgBox), hipHostMallocDefault) != hipSuccess
        || hipHostMalloc(reinterpret_cast<void**>(&s->h_bg_out), (size_t)cap * sizeof(ffs_spot_background), hipHostMallocDefault) != hipSuccess
        || hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_bg_out_dev), s->h_bg_out, 0) != hipSuccess
        || hipMalloc(&s->d_bg_boxes, (size_t)cap * sizeof(SpotBgBox)) != hipSuccess) {
        (void)hipGetLastError();
        c->err = std::string(who) + ": allocation of the box and result buffers failed";
        return FFS_ERR_NOMEM;
    }
    s->bg_cap = cap;
    return FFS_OK;
}

// The GLM call's result buffer is its own, so that a caller may hold both models' records of one batch: room for n records, grown like the
// others and only by the GLM call
static int spotbg_ensure_glm(ffs_stream* s, uint32_t n, const char* who) {
    ffs_ctx* c = s->ctx;
    if (n <= s->bg_glm_cap) return FFS_OK;
    if (s->h_bg_glm_out) (void)hipHostFree(s->h_bg_glm_out);
    s->h_bg_glm_out = s->h_bg_glm_out_dev = nullptr;
    s->bg_glm_cap = 0;
    const uint32_t cap = std::max<uint32_t>(1024u, n + n / 4);
    if (hipHostMalloc(reinterpret_cast<void**>(&s->h_bg_glm_out), (size_t)cap * sizeof(ffs_spot_background_glm), hipHostMallocDefault) != hipSuccess
        || hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_bg_glm_out_dev), s->h_bg_glm_out, 0) != hipSuccess) {
        (void)hipGetLastError();
        c->err = std::string(who) + ": allocation of the result buffer failed";
        return FFS_ERR_NOMEM;
    }
    s->bg_glm_cap = cap;
    return FFS_OK;
}

enum class SpotBgModel { Tukey, Glm };

// What both calls share: the preconditions, the boxes, the launch and the wait.  FFS_OK with *n_out = 0: a batch without reflections,
// nothing launched.  `who` is the entry point's name in every message.
static int spot_backgrounds_run(ffs_stream* s, uint32_t border, SpotBgModel model, const char* who, uint32_t* n_out, float* kernel_ms) {
    ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    const std::string name(who);
    *n_out = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (border < 1 || border > kSpotBgMaxBorder) {
        c->err = name + ": border must be in 1..16, got " + std::to_string(border);
        return FFS_ERR_INVALID;
    }
    if (s->busy) {
        c->err = name + ": a batch is in flight on this stream (its frames replace the last batch's): call it between ffs_wait and the next submit";
        return FFS_ERR_INVALID;
    }
    if (!s->waited_ok) {
        c->err = name + ": no batch has been waited for on this stream yet, or its last ffs_wait failed";
        return FFS_ERR_INVALID;
    }
    if (!s->batch.params.want_reflections) {
        c->err = name + ": the last batch was submitted without want_reflections: there are no reflections to measure";
        return FFS_ERR_INVALID;
    }
    if (L.W > 65536 || L.H > 65536) {
        c->err = name + ": frames wider or higher than 65536 pixels are not supported";
        return FFS_ERR_INVALID;
    }
    const size_t n = s->refls.size();
    if (n == 0) return FFS_OK;
    if (n > 0xFFFFFFFFull || !s->cur_img) {
        c->err = name + ": the stream does not hold the last batch's frames";
        return FFS_ERR_INVALID;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = spotbg_ensure(s, (uint32_t)n, who);
    if (rc == FFS_OK && model == SpotBgModel::Glm) rc = spotbg_ensure_glm(s, (uint32_t)n, who);
    if (rc != FFS_OK) return rc;

    // the boxes, in the order of the batch's reflections, each with its frame; nothing outside a frame gets to the device
    SpotBgBox* boxes = static_cast<SpotBgBox*>(s->h_bg_boxes);
    size_t at = 0;
    for (uint32_t f = 0; f < s->n_frames && f < s->results.size(); ++f) {
        const uint32_t nr = s->results[f].n_reflections;
        for (uint32_t k = 0; k < nr && at < n; ++k, ++at) {
            const ffs_reflection& r = s->refls[at];
            if (r.x_min > r.x_max || r.x_max >= (uint32_t)L.W || r.y_min > r.y_max || r.y_max >= (uint32_t)L.H) {
                c->err = name + ": reflection " + std::to_string(at) + " has a bounding box outside its frame";
                return FFS_ERR_INVALID;
            }
            boxes[at] = SpotBgBox{(uint16_t)r.x_min, (uint16_t)r.x_max, (uint16_t)r.y_min, (uint16_t)r.y_max, f, 0u};
        }
    }
    if (at != n) {
        c->err = name + ": the per-frame reflection counts do not add up to the batch's reflections";
        return FFS_ERR_INVALID;
    }

    SpotBgArgs a{};
    a.image = s->cur_img;
    a.frame_stride = s->cur_fstride;
    a.pitch = (uint32_t)s->cur_pitch;
    a.maskbits = c->d_maskbits;
    a.mpitch = L.mpitch;
    a.W = L.W;
    a.H = L.H;
    a.limit = counting_limit(s->batch.params.max_valid);
    a.border = (int)border;
    a.n = (uint32_t)n;
    a.boxes = static_cast<const SpotBgBox*>(s->d_bg_boxes);
    a.out = reinterpret_cast<SpotBgOut*>(s->h_bg_out_dev);
    (void)hipGetLastError();
    HIP_TRY(c, hipMemcpyAsync(s->d_bg_boxes, s->h_bg_boxes, n * sizeof(SpotBgBox), hipMemcpyHostToDevice, s->bg_st));
    const dim3 grid((uint32_t)((n + kSpotBgWaves - 1) / kSpotBgWaves));
    const bool u16 = c->settings.pixel_bytes == 2;
    if (model == SpotBgModel::Glm) {
        SpotBgGlmOut* glm_out = reinterpret_cast<SpotBgGlmOut*>(s->h_bg_glm_out_dev);
        if (u16) hipExtLaunchKernelGGL(k_spot_background_glm<uint16_t>, grid, dim3(kSpotBgThreads), 0, s->bg_st, s->bg_ev[0], s->bg_ev[1], 0, a, glm_out);
        else hipExtLaunchKernelGGL(k_spot_background_glm<uint32_t>, grid, dim3(kSpotBgThreads), 0, s->bg_st, s->bg_ev[0], s->bg_ev[1], 0, a, glm_out);
    } else if (u16) {
        hipExtLaunchKernelGGL(k_spot_background<uint16_t>, grid, dim3(kSpotBgThreads), 0, s->bg_st, s->bg_ev[0], s->bg_ev[1], 0, a);
    } else {
        hipExtLaunchKernelGGL(k_spot_background<uint32_t>, grid, dim3(kSpotBgThreads), 0, s->bg_st, s->bg_ev[0], s->bg_ev[1], 0, a);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventSynchronize(s->bg_ev[1]));
    if (kernel_ms) HIP_TRY(c, hipEventElapsedTime(kernel_ms, s->bg_ev[0], s->bg_ev[1]));
    *n_out = (uint32_t)n;
    return FFS_OK;
}

static int spot_backgrounds_impl(ffs_stream* s, uint32_t border, const ffs_spot_background** out, uint32_t* n_out, float* kernel_ms) {
    *out = nullptr;
    const int rc = spot_backgrounds_run(s, border, SpotBgModel::Tukey, "ffs_stream_spot_backgrounds", n_out, kernel_ms);
    if (rc != FFS_OK || *n_out == 0) return rc;
    for (uint32_t i = 0; i < *n_out; ++i) {
        ffs_spot_background& b = s->h_bg_out[i];
        b.mean = (b.status == FFS_SPOT_BG_OK && b.n_inliers) ? (double)b.inlier_sum / (double)b.n_inliers : 0.0;
    }
    *out = s->h_bg_out;
    return FFS_OK;
}

// The GLM records are complete as the kernel stored them: the host computes nothing
static int spot_backgrounds_glm_impl(ffs_stream* s, uint32_t border, const ffs_spot_background_glm** out, uint32_t* n_out, float* kernel_ms) {
    *out = nullptr;
    const int rc = spot_backgrounds_run(s, border, SpotBgModel::Glm, "ffs_stream_spot_backgrounds_glm", n_out, kernel_ms);
    if (rc != FFS_OK || *n_out == 0) return rc;
    *out = s->h_bg_glm_out;
    return FFS_OK;
}

extern "C" int ffs_stream_spot_backgrounds(ffs_stream* s, uint32_t border, const ffs_spot_background** out, uint32_t* n, float* kernel_ms) {
    if (!s) {
        g_create_error = "ffs_stream_spot_backgrounds: NULL stream handle";
        return FFS_ERR_INVALID;
    }
    if (!stream_handle_ok(s)) return FFS_ERR_INVALID;
    if (!out || !n) {
        s->ctx->err = "ffs_stream_spot_backgrounds: out and n must not be NULL";
        return FFS_ERR_INVALID;
    }
    return guarded(s->ctx, [&] { return spot_backgrounds_impl(s, border, out, n, kernel_ms); });
}

extern "C" int ffs_stream_spot_backgrounds_glm(ffs_stream* s, uint32_t border, const ffs_spot_background_glm** out, uint32_t* n, float* kernel_ms) {
    if (!s) {
        g_create_error = "ffs_stream_spot_backgrounds_glm: NULL stream handle";
        return FFS_ERR_INVALID;
    }
    if (!stream_handle_ok(s)) return FFS_ERR_INVALID;
    if (!out || !n) {
        s->ctx->err = "ffs_stream_spot_backgrounds_glm: out and n must not be NULL";
        return FFS_ERR_INVALID;
    }
    return guarded(s->ctx, [&] { return spot_backgrounds_glm_impl(s, border, out, n, kernel_ms); });
}
