// ffs_products.hip -- the per-frame products that ride on a batch beside its spots, each from its setter to its accessor: the radial
// profile, the radial-profile threshold (section 3.9) and the per-pixel statistics (section 3.7).  Their kernels are
// included here and nowhere else (see ffs_internal.hpp); ffs_submit.hip decides where in a batch their launches go and calls them from there.
#include "ffs_internal.hpp"
#include "kernels_radial.hpp"
#include "kernels_radthr.hpp"
#include "kernels_pixstats.hpp"

static_assert(kRadialBinsMax == kRadialMaxBins, "ffs_ctx_set_radial_bins accepts what k_radial's LDS holds");

// ---- the radial profile (kernels_radial.hpp) -----------------------------------------------------------------
// The bin map.  Everything is checked before anything changes; like the gain map, the device copy is written only while no batch of the
// context is in flight, and NULL only switches the map off (a batch in flight took its bins at submit and its profile kernels read the
// device copy, which stays).
static int ffs_ctx_set_radial_bins_impl(ffs_ctx* c, const uint16_t* bin_of_pixel, uint32_t n_bins) {
    if (const std::string why = set_radial_bins(c->settings, bin_of_pixel != nullptr, n_bins); !why.empty()) return refuse(c->err, FFS_ERR_INVALID, why);
    if (!bin_of_pixel) {
        c->settings.radial_bins = 0;
        return FFS_OK;
    }
    FFS_TRY(refuse_in_flight(c, "ffs_ctx_set_radial_bins", ": a batch keeps the map it was submitted with"));
    const size_t W = (size_t)c->L.W, n = W * c->L.H;
    for (size_t i = 0; i < n; ++i)
        if (bin_of_pixel[i] >= n_bins && bin_of_pixel[i] != 0xFFFFu)
            return refuse(c->err, FFS_ERR_INVALID,
                          "ffs_ctx_set_radial_bins: " + entry_text(i, W, bin_of_pixel[i]) + ": every entry must be below n_bins = " + std::to_string(n_bins) + " or 0xFFFF (in no bin)");
    std::vector<uint16_t> rows;   // (the entries beyond W are in no bin; the one-byte rows lie behind the two-byte ones)
    const bool first = !c->d_radial_map;
    FFS_TRY(upload_pixel_table(c, "ffs_ctx_set_radial_bins", "bin map", bin_of_pixel, (uint16_t)0xFFFFu, 1, &c->d_radial_map, rows));
    if (first) c->d_radial_map8 = reinterpret_cast<uint8_t*>(c->d_radial_map + rows.size());
    if (n_bins <= 255) {   // the one-byte form (tuning "radial_map8"): what a batch's launch takes is decided from n_bins and the tuning alone
        std::vector<uint8_t> rows8(rows.size());
        for (size_t i = 0; i < rows.size(); ++i) rows8[i] = (uint8_t)rows[i];   // (0xFFFF -> 0xFF; every other entry is below 255)
        HIP_TRY(c, hipMemcpy(c->d_radial_map8, rows8.data(), rows8.size(), hipMemcpyHostToDevice));
    }
    c->settings.radial_bins = n_bins;
    return FFS_OK;
}
extern "C" int ffs_ctx_set_radial_bins(ffs_ctx* c, const uint16_t* bin_of_pixel, uint32_t n_bins) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return ffs_ctx_set_radial_bins_impl(c, bin_of_pixel, n_bins); });
}

// Few fat workgroups over contiguous row bands: about 2048 workgroups a launch (eight per CU) and at most 64 bands a frame, which bounds
// the partials at 64 x n_bins x 20 B a frame -- 1.3 MB at 1024 bins, under 4 % of an Eiger frame.
constexpr uint32_t kRadialTargetGroups = 2048, kRadialMaxBands = 64;

void radial_free(ffs_stream* s) {
    if (s->d_radial_part) (void)hipFree(s->d_radial_part);
    for (uint8_t* p : s->h_radial)
        if (p) (void)hipHostFree(p);
    for (uint8_t* p : s->radial_retired) (void)hipHostFree(p);
    s->d_radial_part = nullptr;
    s->h_radial[0] = s->h_radial[1] = nullptr;
    s->radial_retired.clear();
    s->radial_part_entries = 0;
    s->h_radial_bins = 0;
}

// Room for the profile of a batch of up to max_batch frames under a map of `bins` bins.  Only on a stream with no batch in flight.
int radial_ensure_buffers(ffs_stream* s, uint32_t bins) {
    ffs_ctx* c = s->ctx;
    const size_t slots = max_uniform_band_slots(c->L.H, s->max_batch, kRadialTargetGroups, kRadialMaxBands);   // the most (frame, band) pairs a batch of this stream can have
    if (slots * bins > s->radial_part_entries) {
        if (s->d_radial_part) (void)hipFree(s->d_radial_part);
        s->d_radial_part = nullptr;
        s->radial_part_entries = 0;
        if (hipMalloc(reinterpret_cast<void**>(&s->d_radial_part), slots * bins * 20u) != hipSuccess) {
            (void)hipGetLastError();
            return refuse(c->err, FFS_ERR_NOMEM, "radial profile: hipMalloc(partials) failed");
        }
        s->radial_part_entries = slots * bins;
    }
    if (bins > s->h_radial_bins) {
        // (the buffer the last wait handed out may still be read: it is freed at the next wait; the other one nobody reads)
        for (int i = 0; i < 2; ++i) {
            if (!s->h_radial[i]) continue;
            if (s->h_radial[i] == s->radial_out) s->radial_retired.push_back(s->h_radial[i]);
            else (void)hipHostFree(s->h_radial[i]);
            s->h_radial[i] = nullptr;
        }
        s->h_radial_bins = 0;
        const size_t bytes = (size_t)s->max_batch * bins * 20u;   // sums, sums of squares, counts, [max_batch][bins] each
        for (int i = 0; i < 2; ++i) {
            if (hipHostMalloc(reinterpret_cast<void**>(&s->h_radial[i]), bytes, hipHostMallocDefault) != hipSuccess
                || hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_radial_dev[i]), s->h_radial[i], 0) != hipSuccess) {
                (void)hipGetLastError();
                return refuse(c->err, FFS_ERR_NOMEM, "radial profile: hipHostMalloc(results) failed");
            }
        }
        s->h_radial_bins = bins;
    }
    return FFS_OK;
}

// What a band walk reads: the frames, the context's mask and two-byte map, n_bins of it, the limit of max_valid; the caller sets the bands
static RadialIn make_radial_in(const ffs_ctx* c, const void* d_img, size_t pitch, size_t fstride, uint32_t n_bins, long long max_valid) {
    const Layout& L = c->L;
    RadialIn in{};
    in.image = d_img;
    in.frame_stride = fstride;
    in.pitch = (uint32_t)pitch;
    in.maskbits = c->d_maskbits;
    in.mpitch = L.mpitch;
    in.bins = c->d_radial_map;
    in.bin_pitch = (uint32_t)L.pitch_px;
    in.W = L.W;
    in.H = L.H;
    in.n_bins = n_bins;
    in.limit = counting_limit(max_valid);
    return in;
}

int radial_launch(ffs_stream* s, const void* d_img, size_t pitch, size_t fstride, uint32_t n_frames, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    ffs_ctx* c = s->ctx;
    const uint32_t bins = s->batch.radial_bins;
    const size_t B = s->max_batch;
    RadialArgs a{};
    a.in = make_radial_in(c, d_img, pitch, fstride, bins, s->batch.params.max_valid);
    uniform_row_bands(c->L.H, n_frames, kRadialTargetGroups, kRadialMaxBands, 0, a.in.n_bands, a.in.band_rows);
    const size_t part = s->radial_part_entries;
    a.p_sum = reinterpret_cast<uint64_t*>(s->d_radial_part);
    a.p_sq = a.p_sum + part;
    a.p_count = reinterpret_cast<uint32_t*>(a.p_sq + part);
    uint8_t* out = s->h_radial_dev[s->radial_turn];
    a.r_sum = reinterpret_cast<uint64_t*>(out);
    a.r_sq = a.r_sum + B * bins;
    a.r_count = reinterpret_cast<uint32_t*>(a.r_sq + B * bins);
    if ((size_t)n_frames * a.in.n_bands * bins > part || bins > s->h_radial_bins || !a.in.bins) return refuse(c->err, FFS_ERR_INVALID, "radial profile: the stream's buffers do not hold this batch");
    const dim3 grid(n_frames, a.in.n_bands);
    // (the one-byte form of the map: tuning "radial_map8", for maps of at most 255 bins -- ffs_ctx_set_radial_bins keeps both forms then)
    a.in.bins8 = (c->tune.radial_map8 && bins <= 255) ? c->d_radial_map8 : nullptr;
    using RadialKernel = void (*)(RadialArgs);
    const RadialKernel k = c->settings.pixel_bytes == 2 ? (a.in.bins8 ? k_radial<uint16_t, true> : k_radial<uint16_t, false>)
                                               : (a.in.bins8 ? k_radial<uint32_t, true> : k_radial<uint32_t, false>);
    hipExtLaunchKernelGGL(k, grid, dim3(kRadialThreads), radial_lds_bytes(bins), st, start, nullptr, 0, a);
    hipExtLaunchKernelGGL(k_radial_sum, dim3((bins + 255) / 256, n_frames), dim3(256), 0, st, nullptr, stop, 0, a);
    HIP_TRY(c, hipGetLastError());
    return FFS_OK;
}

// The batch's profile, once: launched by the batch's first enqueue (radial_todo: the re-runs of ffs_wait find it off), for frames that are in
// place in `st`.  Where: tuning "radial_stream".  0 (default): in the batch's SPARSE stream behind the sparse launch and ahead of the batch's
// last event -- the stream has waited for the threshold stage there.  1: in the DENSE stream behind the threshold stage's kernels; the sparse
// stream then waits for ev[5], recorded behind it, ahead of the batch's last event (ffs_wait records ev[5] anew only after that event).
static int launch_radial(ffs_stream* s, uint32_t n, hipStream_t st) {
    s->radial_todo = false;
    FFS_TRY(radial_ensure_buffers(s, s->batch.radial_bins));   // (first use, or a map with more bins: the stream has no batch in flight yet)
    return radial_launch(s, s->cur_img, s->cur_pitch, s->cur_fstride, n, st, nullptr, nullptr);
}
static inline bool radial_wanted(const ffs_stream* s) { return s->radial_todo && s->batch.radial_bins != 0; }
int launch_radial_dense(ffs_stream* s, uint32_t n) {
    if (!radial_wanted(s) || s->ctx->tune.radial_stream != 1 || s->st2 == s->st || s->ctx->tune.dense_overlap != 0) return FFS_OK;   // (dense_overlap: the stage's kernel may be in the partner stream)
    FFS_TRY(launch_radial(s, n, s->st));
    HIP_TRY(s->ctx, hipEventRecord(s->ev[5], s->st));
    HIP_TRY(s->ctx, hipStreamWaitEvent(s->st2, s->ev[5], 0));
    return FFS_OK;
}
int launch_radial_stage(ffs_stream* s, uint32_t n) {
    if (!radial_wanted(s)) return FFS_OK;
    return launch_radial(s, n, s->st2);
}

// ffs_wait's side: the profile of the batch the wait returns becomes what ffs_stream_radial_profile reads (once per batch: a re-run's wait
// finds nothing pending).  The two host buffers take turns, so the next batch writes the other one.
void radial_publish(ffs_stream* s) {
    if (!s->radial_pending) return;
    s->radial_pending = false;
    for (uint8_t* p : s->radial_retired) (void)hipHostFree(p);   // (what the previous wait had handed out before the buffers grew)
    s->radial_retired.clear();
    s->radial_out = nullptr;
    if (s->batch.radial_bins) {
        s->radial_out = s->h_radial[s->radial_turn];
        s->radial_turn ^= 1;
    }
    s->radial_out_bins = s->batch.radial_bins;
    s->radial_out_frames = s->n_frames;
}

extern "C" int ffs_stream_radial_profile(ffs_stream* s, uint32_t frame_in_batch, ffs_radial_profile* out) {
    if (!s || !out || !stream_handle_ok(s)) return FFS_ERR_INVALID;
    ffs_ctx* c = s->ctx;
    if (!s->radial_out || s->radial_out_bins == 0)
        return refuse(c->err, FFS_ERR_INVALID,
                      "ffs_stream_radial_profile: the last batch ffs_wait returned on this stream was submitted without a bin map (ffs_ctx_set_radial_bins)");
    if (frame_in_batch >= s->radial_out_frames)
        return refuse(c->err, FFS_ERR_INVALID,
                      "ffs_stream_radial_profile: frame_in_batch " + std::to_string(frame_in_batch) + " is out of range: the batch had " + std::to_string(s->radial_out_frames) + " frames");
    // (the layout k_radial_sum writes: sums, sums of squares, counts, [max_batch][bins] each)
    const size_t bins = s->radial_out_bins, plane = (size_t)s->max_batch * bins;
    const uint64_t* sum = reinterpret_cast<const uint64_t*>(s->radial_out);
    out->n_bins = s->radial_out_bins;
    out->sum = sum + (size_t)frame_in_batch * bins;
    out->sum_sq = sum + plane + (size_t)frame_in_batch * bins;
    out->count = reinterpret_cast<const uint32_t*>(sum + 2 * plane) + (size_t)frame_in_batch * bins;
    return FFS_OK;
}

// ---- the radial-profile threshold (kernels_radthr.hpp) --------------------------------------------------------
extern "C" int ffs_ctx_set_radial_threshold(ffs_ctx* c, double n_iqr) {
    if (!c) return FFS_ERR_INVALID;
    if (const std::string why = set_radial_threshold(c->settings, n_iqr); !why.empty()) return refuse(c->err, FFS_ERR_INVALID, why);
    c->settings.n_iqr = n_iqr;
    return FFS_OK;
}

extern "C" int ffs_ctx_set_radial_blur(ffs_ctx* c, int blur) {
    if (!c) return FFS_ERR_INVALID;
    if (const std::string why = set_radial_blur(c->settings, blur); !why.empty()) return refuse(c->err, FFS_ERR_INVALID, why);
    c->settings.radial_blur = blur;
    return FFS_OK;
}

// The histogram's workgroups hold a whole CU's LDS each, so a launch aims at two per CU and at most 64 bands a frame; tuning "radthr_bands"
// sets the bands instead (clamped to 1..H).
constexpr uint32_t kRadThrTargetGroups = 512, kRadThrMaxBands = 64;
using RadThrKernel = void (*)(RadThrArgs);
// form: tuning "radthr_form" -- 1 = one LDS add per counting pixel, 2 = a run kept in registers, 0 = the faster of the two as measured
// (DESIGN.md section 3.9): the run for 16-bit pixels, the plain add for 32-bit
static RadThrKernel radthr_hist_kernel(int pixel_bytes, int form) {
    const bool run = form == 0 ? pixel_bytes == 2 : form == 2;
    return pixel_bytes == 2 ? (run ? k_radthr_hist<uint16_t, true> : k_radthr_hist<uint16_t, false>)
                            : (run ? k_radthr_hist<uint32_t, true> : k_radthr_hist<uint32_t, false>);
}
// The blurred forms (ffs_ctx_set_radial_blur; blur = the kernel's radius, 1 or 2): one histogram kernel a pixel size and radius -- the
// plain LDS add: tuning "radthr_form" has no meaning here -- and one strong kernel.
static RadThrKernel radthr_hist_blur_kernel(int pixel_bytes, int blur) {
    return pixel_bytes == 2 ? (blur == kRadBlurNarrow ? k_radthr_hist_blur<uint16_t, 1> : k_radthr_hist_blur<uint16_t, 2>)
                            : (blur == kRadBlurNarrow ? k_radthr_hist_blur<uint32_t, 1> : k_radthr_hist_blur<uint32_t, 2>);
}
static RadThrKernel radthr_strong_blur_kernel(int pixel_bytes, int blur) {
    return pixel_bytes == 2 ? (blur == kRadBlurNarrow ? k_radthr_strong_blur<uint16_t, 1> : k_radthr_strong_blur<uint16_t, 2>)
                            : (blur == kRadBlurNarrow ? k_radthr_strong_blur<uint32_t, 1> : k_radthr_strong_blur<uint32_t, 2>);
}

void radthr_free(ffs_stream* s) {
    if (s->d_radthr_hist) (void)hipFree(s->d_radthr_hist);
    for (ffs_radial_shell* p : s->h_radthr)
        if (p) (void)hipHostFree(p);
    s->d_radthr_hist = s->d_radthr_cut = nullptr;
    s->h_radthr[0] = s->h_radthr[1] = nullptr;
    s->radthr_out = nullptr;
}

// Histograms and cutoffs (one allocation) and the two record buffers, for max_batch frames of kRadThrMaxBins shells: made by the stream's
// first batch of the algorithm and kept.  A table of more than 64 KB of dynamic LDS has to be asked for, per device (chain_prepare_device):
// a device that refuses cannot run the algorithm, and says so.
int radthr_ensure_buffers(ffs_stream* s) {
    if (s->d_radthr_hist) return FFS_OK;
    ffs_ctx* c = s->ctx;
    for (int k = 1; k <= 4; ++k)   // the two forms, then the two blurred kernels
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k <= 2 ? radthr_hist_kernel(c->settings.pixel_bytes, k) : radthr_hist_blur_kernel(c->settings.pixel_bytes, k - 2)),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)radthr_lds_bytes(kRadThrMaxBins)) != hipSuccess) {
            (void)hipGetLastError();
            return refuse(c->err, FFS_ERR_DEVICE, "radial_profile threshold: the device refuses the histogram's " + std::to_string(radthr_lds_bytes(kRadThrMaxBins)) + " bytes of LDS");
        }
    const size_t shells = (size_t)s->max_batch * kRadThrMaxBins;
    uint32_t* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), shells * (kRadThrCounters + 1) * 4u) != hipSuccess) {
        (void)hipGetLastError();
        return refuse(c->err, FFS_ERR_NOMEM, "radial_profile threshold: hipMalloc(histograms) failed");
    }
    for (int i = 0; i < 2; ++i)
        if (hipHostMalloc(reinterpret_cast<void**>(&s->h_radthr[i]), shells * sizeof(ffs_radial_shell), hipHostMallocDefault) != hipSuccess
            || hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_radthr_dev[i]), s->h_radthr[i], 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(d);
            for (ffs_radial_shell*& p : s->h_radthr) {
                if (p) (void)hipHostFree(p);
                p = nullptr;
            }
            return refuse(c->err, FFS_ERR_NOMEM, "radial_profile threshold: hipHostMalloc(records) failed");
        }
    s->d_radthr_hist = d;
    s->d_radthr_cut = d + shells * kRadThrCounters;
    return FFS_OK;
}

// The stage's arguments from the threshold stage's (buffers, pitches, threshold, what the sparse stage wants) and the batch's snapshot
static RadThrArgs make_radthr_args(const ffs_stream* s, const ThresholdArgs& t, uint32_t n_frames) {
    const ffs_ctx* c = s->ctx;
    RadThrArgs a{};
    a.in = make_radial_in(c, t.image, t.pitch, t.frame_stride, s->batch.radthr_bins, t.max_valid);
    uniform_row_bands(c->L.H, n_frames, kRadThrTargetGroups, kRadThrMaxBands, c->tune.radthr_bands, a.in.n_bands, a.in.band_rows);
    a.hist = s->d_radthr_hist;
    a.cut = s->d_radthr_cut;
    a.shells = s->h_radthr_dev[s->radthr_turn];
    a.n_iqr = s->batch.n_iqr;
    a.threshold = t.threshold;
    a.bits = t.bits;
    a.strong_bytes = t.strong_bytes;
    a.tile_counts = t.tile_counts;
    a.occ = t.occ;
    a.occ_frame_words = t.occ_frame_words;
    a.occ_spr = t.occ_spr;
    a.bpitch = t.bpitch;
    a.plane_frame_stride = t.plane_frame_stride;
    a.bytes_frame_stride = t.bytes_frame_stride;
    a.n_tiles = t.n_tiles;
    a.dense_mask = t.dense_mask;
    a.s_strips = ((uint32_t)(t.W + 7) / 8u + 63u) / 64u;
    return a;
}
// The histogram: the frames' tables are zeroed ahead of the launch, outside its events (radthr_ensure_buffers has run)
void launch_radthr_hist(ffs_stream* s, const ThresholdArgs& t, uint32_t n_frames, hipEvent_t start, hipEvent_t stop) {
    const RadThrArgs a = make_radthr_args(s, t, n_frames);
    (void)hipMemsetAsync(a.hist, 0, (size_t)n_frames * a.in.n_bins * kRadThrCounters * 4u, s->st);
    const int blur = s->batch.radial_blur;
    hipExtLaunchKernelGGL(blur ? radthr_hist_blur_kernel(s->ctx->settings.pixel_bytes, blur) : radthr_hist_kernel(s->ctx->settings.pixel_bytes, s->ctx->tune.radthr_form),
                          dim3(n_frames, a.in.n_bands), dim3(kRadThrHistThreads), radthr_lds_bytes(a.in.n_bins), s->st, start, stop, 0, a);
}
// ... and the cutoffs and the strong pixels behind it; `stop` rides on the last dispatch
void launch_radthr_rest(ffs_stream* s, const ThresholdArgs& t, uint32_t n_frames, hipEvent_t stop) {
    const RadThrArgs a = make_radthr_args(s, t, n_frames);
    hipLaunchKernelGGL(k_radthr_cut, dim3(a.in.n_bins, n_frames), dim3(64), 0, s->st, a);
    if (const int blur = s->batch.radial_blur) {   // a wave per run of rows of a strip of kRadBlurOwners groups (the kernel's radblur_strips)
        const uint32_t strips = ((uint32_t)(a.in.W + 7) / 8u + kRadBlurOwners - 1u) / kRadBlurOwners;
        const uint32_t runs = ((uint32_t)a.in.H + kRadBlurRunRows - 1u) / kRadBlurRunRows;
        hipExtLaunchKernelGGL(radthr_strong_blur_kernel(s->ctx->settings.pixel_bytes, blur), dim3(strips * runs, n_frames), dim3(64), 0, s->st, nullptr, stop, 0, a);
        return;
    }
    const dim3 grid(a.s_strips * (uint32_t)a.n_tiles, n_frames);
    if (s->ctx->settings.pixel_bytes == 2) hipExtLaunchKernelGGL(k_radthr_strong<uint16_t>, grid, dim3(64), 0, s->st, nullptr, stop, 0, a);
    else hipExtLaunchKernelGGL(k_radthr_strong<uint32_t>, grid, dim3(64), 0, s->st, nullptr, stop, 0, a);
}

// The records of the radial-profile threshold, handed out as the profile is and under the same flag (radial_pending: once per batch; a re-run
// inside ffs_wait computed the same records into the same buffer).  A batch of another algorithm hands out that it has none.
void radthr_publish(ffs_stream* s) {
    if (!s->radial_pending) return;
    s->radthr_out = nullptr;
    if (s->batch.radthr_bins) {
        s->radthr_out = s->h_radthr[s->radthr_turn];
        s->radthr_turn ^= 1;
    }
    s->radthr_out_bins = s->batch.radthr_bins;
    s->radthr_out_frames = s->n_frames;
}

extern "C" int ffs_stream_radial_thresholds(ffs_stream* s, uint32_t frame_in_batch, const ffs_radial_shell** out, uint32_t* n_bins) {
    if (!s || !out || !n_bins || !stream_handle_ok(s)) return FFS_ERR_INVALID;
    ffs_ctx* c = s->ctx;
    if (!s->radthr_out || s->radthr_out_bins == 0)
        return refuse(c->err, FFS_ERR_INVALID,
                      "ffs_stream_radial_thresholds: the last batch ffs_wait returned on this stream did not run the radial_profile algorithm (FFS_ALGO_RADIAL_PROFILE)");
    if (frame_in_batch >= s->radthr_out_frames)
        return refuse(c->err, FFS_ERR_INVALID,
                      "ffs_stream_radial_thresholds: frame_in_batch " + std::to_string(frame_in_batch) + " is out of range: the batch had " + std::to_string(s->radthr_out_frames) + " frames");
    *out = s->radthr_out + (size_t)frame_in_batch * s->radthr_out_bins;   // (the layout k_radthr_cut writes: [frame][bins of the batch])
    *n_bins = s->radthr_out_bins;
    return FFS_OK;
}

// ---- the per-pixel statistics (kernels_pixstats.hpp) -----------------------------------------------------------
int pixstats_ensure(ffs_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->stats_st) HIP_TRY(c, hipStreamCreateWithFlags(&c->stats_st, hipStreamNonBlocking));
    if (!c->d_stats && hipMalloc(reinterpret_cast<void**>(&c->d_stats), pixstats_layout(c).bytes()) != hipSuccess) {
        (void)hipGetLastError();
        c->d_stats = nullptr;
        return refuse(c->err, FFS_ERR_NOMEM, "pixel statistics: hipMalloc(accumulators, " + std::to_string(pixstats_layout(c).bytes() >> 20) + " MB) failed");
    }
    return FFS_OK;
}

extern "C" int ffs_ctx_set_pixel_stats(ffs_ctx* c, int mode) {
    if (!c) return FFS_ERR_INVALID;
    if (mode != FFS_PIXEL_STATS_OFF && mode != FFS_PIXEL_STATS_START && mode != FFS_PIXEL_STATS_RESUME)
        return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_set_pixel_stats: mode must be FFS_PIXEL_STATS_OFF (0), _START (1) or _RESUME (2), got " + std::to_string(mode));
    if (mode == FFS_PIXEL_STATS_OFF) {   // (at any time: a batch in flight carries its own "on")
        c->settings.pixel_stats = false;
        return FFS_OK;
    }
    if (mode == FFS_PIXEL_STATS_RESUME && c->stats_started) {
        c->settings.pixel_stats = true;
        return FFS_OK;
    }
    FFS_TRY(refuse_in_flight(c, "ffs_ctx_set_pixel_stats", ": a start zeroes the accumulators"));
    if (const int rc = pixstats_ensure(c); rc != FFS_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_stats, 0, pixstats_layout(c).bytes(), c->stats_st));
    HIP_TRY(c, hipStreamSynchronize(c->stats_st));
    std::lock_guard<std::mutex> lock(c->stats_mu);
    c->stats_frames = 0;
    c->stats_started = true;
    c->settings.pixel_stats = true;
    return FFS_OK;
}

int pixstats_launch(ffs_ctx* c, const void* d_img, size_t pitch, size_t fstride, uint32_t n_frames, long long max_valid, hipStream_t st, hipEvent_t start,
                    hipEvent_t stop) {
    const PixStatsLayout P = pixstats_layout(c);
    if (!c->d_stats || n_frames == 0) return refuse(c->err, FFS_ERR_INVALID, "pixel statistics: the context has no accumulators");
    PixStatsArgs a{};
    a.frame_stride = fstride;
    a.pitch = (uint32_t)pitch;
    a.groups = P.groups;
    a.n_lanes = P.n_lanes;
    a.limit = counting_limit(max_valid);
    a.count = reinterpret_cast<uint4*>(c->d_stats);
    a.max = reinterpret_cast<uint4*>(c->d_stats + P.plane32);
    a.sum = reinterpret_cast<uint4*>(c->d_stats + 2 * P.plane32);
    a.sum_sq = reinterpret_cast<uint4*>(c->d_stats + 2 * P.plane32 + P.plane64);
    const dim3 grid((P.n_lanes + kPixStatsThreads - 1) / kPixStatsThreads);
    // (one launch holds at most kPixStatsMaxFrames frames -- the 16-bit kernel's 32-bit sums; a longer batch is several, one behind the other)
    for (uint32_t f0 = 0; f0 < n_frames; f0 += kPixStatsMaxFrames) {
        a.image = static_cast<const uint8_t*>(d_img) + (size_t)f0 * fstride;
        a.n_frames = std::min(n_frames - f0, kPixStatsMaxFrames);
        const bool first = f0 == 0, last = n_frames - f0 <= kPixStatsMaxFrames;
        if (c->settings.pixel_bytes == 2) hipExtLaunchKernelGGL(k_pixel_stats<uint16_t>, grid, dim3(kPixStatsThreads), 0, st, first ? start : nullptr, last ? stop : nullptr, 0, a);
        else hipExtLaunchKernelGGL(k_pixel_stats<uint32_t>, grid, dim3(kPixStatsThreads), 0, st, first ? start : nullptr, last ? stop : nullptr, 0, a);
    }
    HIP_TRY(c, hipGetLastError());
    return FFS_OK;
}

// The batch's frames into the context's statistics, once: launched by the batch's first enqueue (stats_todo: the re-runs of ffs_wait find it
// off).  The accumulators belong to the context and every launch reads, adds and writes them whole, so two launches must never overlap,
// whichever ffs_streams and threads they come from.  Where: tuning "stats_stream".
//   0: the context's own HIP stream, in which launches follow one another.  It waits for the event behind which the frames are in place --
//      ev[1], recorded behind the upload or the decode; resident frames (ffs_submit_device) are in place as they come -- so the kernel may run
//      beside the batch's threshold stage, and the dense stream gets no packet of ours.
//   1: the batch's dense stream behind the threshold stage's kernels.  Only where that is ONE stream for the whole context: not under
//      "sched" 0 (a HIP stream per ffs_stream) and not under "dense_overlap" 1 (the stage's kernel may be in the partner stream); 0 is taken there.
// Either way ev_stats is recorded behind the launch and the batch's sparse stream waits for it ahead of the batch's last event
// (join_pixel_stats): the frames stay valid until ffs_wait returns, and every waited batch is in what ffs_ctx_get_pixel_stats copies.
// stats_mu makes wait, launch, record and the frame count one step.
int launch_pixel_stats(ffs_stream* s, uint32_t n) {
    if (!s->stats_todo) return FFS_OK;
    s->stats_todo = false;
    if (!s->batch.pixel_stats) return FFS_OK;
    ffs_ctx* c = s->ctx;
    if (!s->ev_stats) HIP_TRY(c, hipEventCreateWithFlags(&s->ev_stats, hipEventDisableTiming));
    const bool dense = c->tune.stats_stream == 1 && s->st2 != s->st && c->tune.dense_overlap == 0;
    std::lock_guard<std::mutex> lock(c->stats_mu);
    hipStream_t st = dense ? s->st : c->stats_st;
    if (!dense && !s->dev_input) HIP_TRY(c, hipStreamWaitEvent(st, s->ev[1], 0));
    FFS_TRY(pixstats_launch(c, s->cur_img, s->cur_pitch, s->cur_fstride, n, s->batch.params.max_valid, st, nullptr, nullptr));
    HIP_TRY(c, hipEventRecord(s->ev_stats, st));
    c->stats_frames += n;
    s->stats_join = true;
    return FFS_OK;
}
int join_pixel_stats(ffs_stream* s) {
    if (!s->stats_join) return FFS_OK;
    s->stats_join = false;
    HIP_TRY(s->ctx, hipStreamWaitEvent(s->st2, s->ev_stats, 0));
    return FFS_OK;
}

// Everything is checked before anything is copied.  No batch is in flight, so every launch lies ahead of an event some ffs_wait has seen
// -- the streams are synchronised all the same, for a batch whose wait failed -- and the planes are copied one at a time and un-interleaved.
static int ffs_ctx_get_pixel_stats_impl(ffs_ctx* c, ffs_pixel_stats* out) {
    if (!c->stats_started) return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_get_pixel_stats: no statistics yet (ffs_ctx_set_pixel_stats(ctx, FFS_PIXEL_STATS_START) first)");
    FFS_TRY(refuse_in_flight(c, "ffs_ctx_get_pixel_stats", ""));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stats_st));
    if (c->dense_st) HIP_TRY(c, hipStreamSynchronize(c->dense_st));
    const PixStatsLayout P = pixstats_layout(c);
    const size_t W = (size_t)c->L.W, H = (size_t)c->L.H;
    std::vector<uint64_t> plane;
    auto fetch = [&](size_t offset, size_t bytes, uint32_t entry_bytes, void* dst) -> int {
        if (!dst) return FFS_OK;
        plane.resize(bytes / 8);
        HIP_TRY(c, hipMemcpy(plane.data(), c->d_stats + offset, bytes, hipMemcpyDeviceToHost));
        for (size_t y = 0; y < H; ++y)
            for (size_t x = 0; x < W; ++x) {
                const size_t at = P.entry((uint32_t)(y * P.groups + x / P.px), (uint32_t)(x % P.px), entry_bytes);
                if (entry_bytes == 4) static_cast<uint32_t*>(dst)[y * W + x] = reinterpret_cast<const uint32_t*>(plane.data())[at];
                else static_cast<uint64_t*>(dst)[y * W + x] = plane[at];
            }
        return FFS_OK;
    };
    if (const int rc = fetch(0, P.plane32, 4, out->count); rc != FFS_OK) return rc;
    if (const int rc = fetch(P.plane32, P.plane32, 4, out->max); rc != FFS_OK) return rc;
    if (const int rc = fetch(2 * P.plane32, P.plane64, 8, out->sum); rc != FFS_OK) return rc;
    if (const int rc = fetch(2 * P.plane32 + P.plane64, P.plane64, 8, out->sum_sq); rc != FFS_OK) return rc;
    std::lock_guard<std::mutex> lock(c->stats_mu);
    out->n_frames = c->stats_frames;
    return FFS_OK;
}
extern "C" int ffs_ctx_get_pixel_stats(ffs_ctx* c, ffs_pixel_stats* out) {
    if (!c) return FFS_ERR_INVALID;
    if (!out) return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_get_pixel_stats: out is NULL");
    return guarded(c, [&] { return ffs_ctx_get_pixel_stats_impl(c, out); });
}
