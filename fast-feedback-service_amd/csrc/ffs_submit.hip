// ffs_submit.hip -- everything that puts a batch on the device: the threshold stage's arguments (their launch geometry comes from
// launch_geometry.hpp), the launches of the threshold stage and of the sparse stage (compaction -> connected components -> records),
// ffs_submit and ffs_submit_device (encoded input: ffs_encoded.hip).  All kernels of the hot path are included here and nowhere else (see
// ffs_internal.hpp).
//
// Reference: the per-frame section of spotfinder/spotfinder.cc:751-1008 (H2D, kernel launch wrapper
// spotfinder/spotfinder.cu:148-189, D2H of the mask, host connected components).
#include "ffs_internal.hpp"
#include "kernels_threshold.hpp"
#include "kernels_extended.hpp"
#include "kernels_stream.hpp"
#include "kernels_ccl.hpp"
#include "kernels_chain.hpp"
#include "kernels_band.hpp"
#include "kernels_window.hpp"

bool chain_prepare_device() {   // more than 64 KB of dynamic LDS has to be asked for, per device
    const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_frame_chain<uint16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, kChainDynBytes);
    const hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_frame_chain<uint32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, kChainDynBytes);
    const hipError_t e3 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_frame_chain<uint16_t, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kChainDynBytes);
    const hipError_t e4 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_frame_chain<uint16_t, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kChainDynBytes);
    const hipError_t e5 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_frame_chain<uint32_t, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kChainDynBytes);
    (void)hipGetLastError();
    return e1 == hipSuccess && e2 == hipSuccess && e3 == hipSuccess && e4 == hipSuccess && e5 == hipSuccess;
}

// ---- the threshold stage's arguments: buffers and pitches, the predicate's constants, the launch geometry ------------------
ThresholdRoute batch_route(const ffs_stream* s, const Rerun& how) {
    const ParamSnapshot& b = s->batch;
    return threshold_route(b.params.algorithm, s->ctx->settings.pixel_bytes, win_default(b.params), b.max_valid_scope, b.params.max_valid, b.gain, how.threshold_path,
                           s->ctx->tune, b.gain_map);
}
static void set_buffers(ThresholdArgs& a, const ffs_stream* s, const void* img, size_t pitch, size_t fstride, const ThresholdRoute& route) {
    const ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    const ffs_params& p = s->batch.params;
    a.image = img;
    a.frame_stride = fstride;
    a.pitch = (uint32_t)pitch;
    a.maskbits = c->d_maskbits;
    a.bits = s->d_bits;
    a.strong_bytes = s->d_sbytes;
    a.tile_counts = s->d_tile_counts;
    a.W = L.W;
    a.H = L.H;
    a.pitch_px = L.pitch_px;
    a.mpitch = L.mpitch;
    a.bpitch = L.bpitch;
    a.plane_frame_stride = L.plane_frame_stride;
    a.bytes_frame_stride = L.bytes_frame_stride;
    a.n_tiles = c->n_tiles;
    // bright windows (sum p >= 65536; 32-bit pixels >= 2^24): onto the list k_bright_fix works off, or into the plane as candidates
    a.bright_to_plane = route.bright_to_plane;
    a.overflow = s->d_overflow;
    a.bright_n = s->d_tile_counts + tile_counts_bytes(s) / 4 - 1;
    a.bright_list = s->d_bright;
    a.bright_cap = std::min<uint32_t>(kBrightCap, (uint32_t)c->tune.bright_cap);
    a.occ = s->d_occ;
    a.occ_frame_words = occ_frame_words(L);
    a.occ_spr = L.mpitch / 16;
    // The byte mask (the reference kernel's result_strong, 1 byte per pixel) is an OUTPUT only when it was asked for
    // (want_strong_mask: --writeout, parity tests): the hot path's own strong mask is the bit plane, and the 0.58 GB of
    // zeros per 32 Eiger frames cost the streaming kernel 15 %.  (The exact kernel of path 1 sets its 1s: zero-filled then too.)
    a.dense_mask = (p.want_strong_mask || c->tune.dense_mask || a.bright_to_plane) ? 1 : 0;
#ifdef FFS_EXPERIMENTS
    a.dbg = c->tune.exp.k1_debug;
    if (a.dbg & 16) a.dense_mask = 1;
    if (a.dbg & 8) a.dense_mask = 0;
#endif
    a.dbg_prio = c->tune.stream_prio;
    a.ginfo = c->d_ginfo;
    a.mmap = c->d_mmap;
    a.gpitch = ginfo_pitch(L, c->settings.pixel_bytes);
    a.gpf = groups_per_row(L, c->settings.pixel_bytes);
    a.dplane = s->d_dplane;
    a.eplane = s->d_eplane;
    a.eplane_clean = s->ext_e_clean ? 1 : 0;
    a.ext_variant = route.ext_variant;
}
static void set_predicate(ThresholdArgs& a, const ffs_params& p, bool trusted, double gain, const ffs_ctx* map_of) {
    a.nb_limit = counting_limit(trusted ? p.max_valid : -1);   // (exclusive; trusted: the window scope with a max_valid)
    a.kS = (float)(p.nsig_s * p.nsig_s * (1.0 - 1.0 / 65536.0));
    a.kB = (float)(p.nsig_b * (1.0 - 1.0 / 1048576.0));
    a.min_count = p.min_count;
    a.nsig_b = p.nsig_b;
    a.nsig_s = p.nsig_s;
    a.nsig_b2 = p.nsig_b * p.nsig_b;
    a.nsig_s2 = p.nsig_s * p.nsig_s;
    a.threshold = p.threshold;
    a.max_valid = p.max_valid;
    {
        const double b2 = p.nsig_b * p.nsig_b, s2 = p.nsig_s * p.nsig_s;
        a.int_pred = (b2 == std::floor(b2) && s2 == std::floor(s2) && b2 <= 1024.0 && s2 <= 1024.0 && p.threshold < 2147483648.0
                      && std::sqrt(b2) == p.nsig_b && std::sqrt(s2) == p.nsig_s) ? 1 : 0;   // (integer nsig: the squares are exact)
        a.ib2 = a.int_pred ? (uint32_t)b2 : 0u;
        a.is2 = a.int_pred ? (uint32_t)s2 : 0u;
        a.thr_floor = a.int_pred ? (uint32_t)std::floor(p.threshold) : 0u;
    }
    a.kx = win_half(p.kernel_half_x);
    a.ky = win_half(p.kernel_half_y);
    // the general-window kernel's float32 screens
    // (only where the float32 arithmetic of the screens can neither overflow nor lose its margin: DESIGN.md section 3.3b)
    a.w_kS = (std::isfinite(p.nsig_s) && p.nsig_s <= 1024.0) ? (float)(p.nsig_s * p.nsig_s * (1.0 - 1.0 / 65536.0)) : 0.0f;
    a.w_kB = (std::isfinite(p.nsig_b) && p.nsig_b <= 1024.0) ? (float)(p.nsig_b * p.nsig_b * (1.0 - 1.0 / 65536.0)) : 0.0f;
    a.ext_flavour = p.extended_flavour;
    // The detector gain and what the float32 screens of the gain kernels take: the signal screen is win_signal's
    // own with the gain inside its constant; the dispersion screen takes the gain and nsig_b as floats.  Outside the range the proofs
    // cover (the float32 products must stay normal numbers) a screen is off and float64 decides.
    a.gain = gain;
    a.g_gain = 0.0f;
    a.g_nb = 0.0f;
    if (gain > 0.0) {
        const bool in_range = gain >= 0x1p-60 && gain <= 0x1p60;
        if (!in_range) a.w_kS = 0.0f;
        else if (a.w_kS != 0.0f) a.w_kS = (float)(gain * (p.nsig_s * p.nsig_s) * (1.0 - 1.0 / 65536.0));
        // (a constant near the bottom of float32's normal range rounds by more than the margin: nsig_s has no lower bound of its own)
        if (a.w_kS < 0x1p-100f) a.w_kS = 0.0f;
        if (in_range && std::isfinite(p.nsig_b) && p.nsig_b <= 1024.0 && (p.nsig_b == 0.0 || p.nsig_b >= 0x1p-60)) {
            a.g_gain = (float)gain;
            a.g_nb = (float)p.nsig_b;
        }
    }
    // The gain map: the kernels multiply w_kS -- still nsig_s^2 (1 - 2^-16) here, nsig_s <= 1024 or 0 -- by the
    // pixel's own gain, so the smallest product any pixel forms, with the map's minimum, must be a normal float32 with its 24 bits (the
    // largest is below 2^80); and the dispersion screen takes the pixel's gain, always in range, so only nsig_b can switch its
    // square-root term off (g_nb = 0: cf = g x (m - 1), never above c).
    a.gain_map = nullptr;
    a.gm_pitch = 0;
    if (map_of) {
        a.gain_map = map_of->d_gain_map;
        a.gm_pitch = (uint32_t)map_of->L.pitch_px * 4u;
        if (map_of->gain_map_min * a.w_kS < 0x1p-100f) a.w_kS = 0.0f;
        if (std::isfinite(p.nsig_b) && p.nsig_b <= 1024.0 && p.nsig_b >= 0x1p-60) a.g_nb = (float)p.nsig_b;
    }
}
// (launch_geometry.hpp computes them; the super rows of the streaming launch, g.n_groups, are its grid's y and no argument)
static void set_geometry(ThresholdArgs& a, uint32_t n_frames, const StreamGeometry& g, const WindowGeometry& w, const ExtGeometry& e, const EmptyRuns& empty) {
    a.empty_runs = empty;   // (what the streaming waves trim off their bands' ends: the geometry itself does not depend on the mask)
    a.n_frames = (int)n_frames;
    a.group_frames = g.group_frames;
    a.n_strips = g.n_strips;
    a.n_bands = g.n_bands;
    a.band_rows = g.band_rows;
    a.band_rows2 = g.band_rows2;
    a.band_split = g.band_split;
    a.w_strips = w.w_strips;
    a.w_band_rows = w.w_band_rows;
    a.w_bands = w.w_bands;
    a.ext_strips = e.ext_strips;
    a.ext_band_rows = e.ext_band_rows;
    a.ext_bands = e.ext_bands;
}
StreamGeometry batch_stream_geometry(const ffs_stream* s, size_t fstride, uint32_t n_frames) {
    return stream_geometry(s->ctx->L, s->ctx->settings.pixel_bytes, fstride, n_frames, s->ctx->tune);
}
ThresholdArgs make_threshold_args(ffs_stream* s, const void* img, size_t pitch, size_t fstride, uint32_t n_frames, const StreamGeometry& g,
                                  const ThresholdRoute& route) {
    ThresholdArgs a{};
    set_buffers(a, s, img, pitch, fstride, route);
    set_predicate(a, s->batch.params, route.window_scope, s->batch.gain, s->batch.gain_map ? s->ctx : nullptr);
    set_geometry(a, n_frames, g, window_geometry(s->ctx->L, n_frames, a.ky), ext_geometry(s->ctx->L, n_frames), s->ctx->empty_runs);
    return a;
}

// ---- the threshold stage's launches -----------------------------------------------------------------------------
static dim3 stream_grid(const ThresholdArgs& a, const StreamGeometry& g) {
    return dim3(8u * stream_chunk(a), (unsigned)g.n_groups);   // (the units in eight equal chunks, one per XCD: launch_geometry.hpp, stream_unit_of)
}

// The instantiation of the streaming kernels a launch takes.  Rows of loads a wave keeps in flight: tuning "rows_ahead", within what
// exists for the pixel size (16-bit: 2, 3 or 4; 32-bit: 2 or 3, so 4 means 3); the kernels that zero-fill the byte mask (dense_mask) and
// the extended algorithm's first pass (16-bit pixels only) exist with two rows.
using StreamKernel = void (*)(ThresholdArgs);
static StreamKernel stream_kernel(const ffs_ctx* c, bool dense_mask, bool extended) {
    const int rows = std::clamp(c->tune.rows_ahead, 2, c->settings.pixel_bytes == 4 ? 3 : 4);
    if (c->settings.pixel_bytes == 4) return dense_mask ? k_stream_u32<2, true> : rows == 3 ? k_stream_u32<3, false> : k_stream_u32<2, false>;
    if (extended) return dense_mask ? k_stream_u16<2, true, true> : k_stream_u16<2, true, false>;
    if (dense_mask) return k_stream_u16<2, false, true>;
    return rows == 4 ? k_stream_u16<4, false, false> : rows == 3 ? k_stream_u16<3, false, false> : k_stream_u16<2, false, false>;
}
// The whole standard threshold in one kernel: final strong plane + per-tile counts (atomics into zeroed counters).
// Start and stop events ride on the dispatch itself (its completion signal): no marker packets around it.
static void launch_stream(ffs_stream* s, const ThresholdArgs& a, const StreamGeometry& g, hipEvent_t start, hipEvent_t stop, hipStream_t st = nullptr) {
    hipExtLaunchKernelGGL(stream_kernel(s->ctx, a.dense_mask != 0, false), stream_grid(a, g), dim3(64), 0, st ? st : s->st, start, stop, 0, a);
}
// The instantiation of a kernel family a launch takes: (pixel_bytes, variant) as compile-time tags, handed to `launch`, which names the
// kernel with them.  (`of` folds the variant as threshold_route.hpp's rule says, so no instantiation exists twice.)
template <typename PixelT, Predicate V>
struct KernelTag {
    using pixel = PixelT;
    static constexpr Predicate of(KernelFamily f) { return instantiated_as(f, sizeof(PixelT), V); }
};
template <Predicate V, typename Launch>
static void with_pixel_tag(int pixel_bytes, Launch& launch) {
    if (pixel_bytes == 4) launch(KernelTag<uint32_t, V>{});
    else launch(KernelTag<uint16_t, V>{});
}
template <typename Launch>
static void with_kernel_tag(int pixel_bytes, Predicate v, Launch&& launch) {
    if (v == Predicate::kGainMap) with_pixel_tag<Predicate::kGainMap>(pixel_bytes, launch);
    else if (v == Predicate::kGain) with_pixel_tag<Predicate::kGain>(pixel_bytes, launch);
    else if (v == Predicate::kWindowScope) with_pixel_tag<Predicate::kWindowScope>(pixel_bytes, launch);
    else with_pixel_tag<Predicate::kPhotonCount>(pixel_bytes, launch);
}

// The general-window kernel (kernels_window.hpp), where the route says so (ThresholdStage::kWindow).  The standard algorithm on the plane
// paths only (no wave logs: those belong to k_stream_u16); the cross-check path (threshold_path 2) keeps its gather.
template <typename PixelT, Predicate V>
static void launch_window_t(const ThresholdArgs& a, dim3 grid, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    const size_t lds = win_ring_bytes((int)sizeof(PixelT), a.ky);
    switch (a.kx) {
        case 1: hipExtLaunchKernelGGL((k_window<PixelT, 1, V>), grid, dim3(64), lds, st, start, stop, 0, a); break;
        case 2: hipExtLaunchKernelGGL((k_window<PixelT, 2, V>), grid, dim3(64), lds, st, start, stop, 0, a); break;
        case 3: hipExtLaunchKernelGGL((k_window<PixelT, 3, V>), grid, dim3(64), lds, st, start, stop, 0, a); break;
        case 4: hipExtLaunchKernelGGL((k_window<PixelT, 4, V>), grid, dim3(64), lds, st, start, stop, 0, a); break;
        case 5: hipExtLaunchKernelGGL((k_window<PixelT, 5, V>), grid, dim3(64), lds, st, start, stop, 0, a); break;
        case 6: hipExtLaunchKernelGGL((k_window<PixelT, 6, V>), grid, dim3(64), lds, st, start, stop, 0, a); break;
        default: hipExtLaunchKernelGGL((k_window<PixelT, 7, V>), grid, dim3(64), lds, st, start, stop, 0, a); break;
    }
}
static void launch_window(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, uint32_t n_frames, hipEvent_t start, hipEvent_t stop) {
    const dim3 grid((unsigned)(a.w_strips * a.w_bands), n_frames);
    with_kernel_tag(s->ctx->settings.pixel_bytes, route.variant, [&](auto tag) {
        using T = decltype(tag);
        launch_window_t<typename T::pixel, T::of(KernelFamily::kWindow)>(a, grid, s->st, start, stop);
    });
}
static void launch_bright_fix(ffs_stream* s, const ThresholdArgs& a, hipStream_t st) {
    if (s->ctx->settings.pixel_bytes == 4) hipLaunchKernelGGL(k_bright_fix<uint32_t>, dim3(32), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_bright_fix<uint16_t>, dim3(32), dim3(256), 0, st, a);
}
// path 1: every pixel marked in the plane (decided strong pixels and bright-window candidates alike) takes the gathered
// predicate; rewrites the plane, the per-tile counts and sets the byte mask's 1s
static void launch_exact(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, uint32_t n_frames, hipStream_t st) {
    const dim3 grid((unsigned)a.n_tiles, n_frames);
    // (a variant other than photon-count: the cross-check path, the only one that gets here with it)
    with_kernel_tag(s->ctx->settings.pixel_bytes, route.variant, [&](auto tag) {
        using T = decltype(tag);
        if (route.window_3x3) hipLaunchKernelGGL((k_exact<typename T::pixel, T::of(KernelFamily::kExact)>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_exact_w<typename T::pixel, T::of(KernelFamily::kExact)>), grid, dim3(256), 0, st, a);   // (the runtime-window gather: exact_strong_w)
    });
}

// Extended dispersion: first pass -> erosion -> final threshold (kernels_extended.hpp).  Leaves the strong plane in
// a.bits, the byte mask and the per-tile counts as the exact stage does.  First pass, 16-bit pixels: the streaming kernel
// in its extended mode decides it exactly in its drain (ext_variant 2, default); k_ext_first is the plain one-pixel-
// per-lane kernel that computes the same plane directly (32-bit pixels, tuning "ext_first_pass" = 0, and the fall-back
// when the bright-window list of a batch overflowed): ThresholdRoute::ext_streams_first.
static void launch_ext_first(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, const StreamGeometry& g, uint32_t n_frames, hipEvent_t start, hipEvent_t stop, bool fix_here = true,
                             bool plane_clean = false, bool counts_clean = false) {
    if (route.ext_streams_first()) {
        // the kernel writes the non-zero bytes of the first-pass plane; the bright-list count sits behind the tile counts
        // (both are usually clean already: the plane was cleared behind the previous batch's sparse launch, which also zeroed the counts)
        if (!plane_clean) (void)hipMemsetAsync(a.dplane, 0, (size_t)n_frames * a.plane_frame_stride, s->st);
        if (!counts_clean) (void)hipMemsetAsync(a.tile_counts, 0, tile_counts_bytes(s), s->st);
        hipExtLaunchKernelGGL(stream_kernel(s->ctx, a.dense_mask != 0, true), stream_grid(a, g), dim3(64), 0, s->st, start, stop, 0, a);
        if (fix_here) hipLaunchKernelGGL((k_bright_fix<uint16_t, true>), dim3(32), dim3(256), 0, s->st, a);
        return;
    }
    dim3 g1((unsigned)(a.ext_strips * a.ext_bands), n_frames);
    with_kernel_tag(s->ctx->settings.pixel_bytes, route.variant, [&](auto tag) {
        using T = decltype(tag);
        hipExtLaunchKernelGGL((k_ext_first<typename T::pixel, T::of(KernelFamily::kExtFirst)>), g1, dim3(64), 0, s->st, start, stop, 0, a);
    });
}
static void launch_ext_rest(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, uint32_t n_frames, hipStream_t st) {
    // The byte mask: the streaming kernel zero-filled it if somebody wants it (k_ext_final sets 1s in it either way; without a
    // taker they land in a buffer nobody reads); after k_ext_first it is always produced, so zero it here.
    if (!route.ext_streams_first()) (void)hipMemsetAsync(a.strong_bytes, 0, (size_t)n_frames * a.bytes_frame_stride, st);
    dim3 g3((unsigned)a.n_tiles, n_frames);
    if (route.ext_fused) {   // erosion inside the final pass's tiles: one launch, the plane crosses memory once (16-bit pixels, no gain)
        hipLaunchKernelGGL(route.variant == Predicate::kWindowScope ? k_ext_erode_final<Predicate::kWindowScope> : k_ext_erode_final<Predicate::kPhotonCount>, g3,
                           dim3(256), (size_t)(kTileRows + 10) * a.mpitch, st, a);
        return;
    }
    const int erode = s->ctx->tune.ext_erode;
    if (erode != 0) {
        const unsigned strips = (a.mpitch / 4 + 61) / 62, rows = erode == 1 ? 32 : 16;
        const dim3 ge(strips * 8u * (((unsigned)((a.H + rows - 1) / rows) + 7u) / 8u), n_frames);
        if (erode == 1 && a.eplane_clean) hipLaunchKernelGGL((k_ext_erode_strips<32, true>), ge, dim3(64), 0, st, a);
        else if (erode == 1) hipLaunchKernelGGL((k_ext_erode_strips<32, false>), ge, dim3(64), 0, st, a);
        else if (a.eplane_clean) hipLaunchKernelGGL((k_ext_erode_strips<16, true>), ge, dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_ext_erode_strips<16, false>), ge, dim3(64), 0, st, a);
    } else {
        const unsigned erode_lanes = (a.mpitch / 4) * (unsigned)((a.H + kErodeRows - 1) / kErodeRows);
        hipLaunchKernelGGL(k_ext_erode, dim3((erode_lanes + 255) / 256, n_frames), dim3(256), 0, st, a);
    }
    with_kernel_tag(s->ctx->settings.pixel_bytes, route.variant, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_ext_final<typename T::pixel, T::of(KernelFamily::kExtFinal)>), g3, dim3(256), 0, st, a);
    });
}

int ensure_extended_buffers(ffs_stream* s) {
    if (s->d_dplane) return FFS_OK;
    ffs_ctx* c = s->ctx;
    const size_t bytes = (size_t)s->max_batch * c->L.plane_frame_stride;
    s->dplane2_clean = false;
    if (dmalloc(&s->d_ext_pair[0], 2 * bytes) != hipSuccess || dmalloc(&s->d_ext_pair[1], 2 * bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->err = "hipMalloc(extended dispersion planes) failed";
        return FFS_ERR_NOMEM;
    }
    s->d_dplane = s->d_ext_pair[0];
    s->d_eplane = s->d_ext_pair[0] + bytes;
    s->d_dplane2 = s->d_ext_pair[1];
    s->d_eplane2 = s->d_ext_pair[1] + bytes;
    return FFS_OK;
}

// Wave logs (tuning "strong_log"): the 16-bit standard path on a context with sparse streams, a geometry kernels_chain.hpp's merge holds
// (at most twelve strips per frame) -- can this batch take them?
static bool wave_logs_possible(const ffs_stream* s, const ThresholdArgs& a, const Rerun& how) {
    const ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    return c->tune.strong_log != 0 && !a.bright_to_plane && !s->log_off && !how.plane && s->st2 != s->st && c->chain_ok
           && s->batch.params.algorithm != FFS_ALGO_DISPERSION_EXTENDED && c->n_tiles <= kChainMaxTiles && L.H <= kChainMaxRows
           && strips_per_frame(L, c->settings.pixel_bytes) <= 16u && a.band_rows <= 1024 && L.W <= 65535;
}
// The stream's logs hold `slots` waves: allocated on first use; false: no memory for them.
static bool ensure_wave_logs(ffs_stream* s, size_t slots) {
    if (slots <= s->wlog_waves) return true;
    if (s->d_wlog) {
        (void)hipFree(s->d_wlog);
        (void)hipFree(s->d_wlog_n);
        (void)hipFree(s->d_wpix);
        s->d_wlog = nullptr;
        s->d_wlog_n = nullptr;
        s->d_wpix = nullptr;
    }
    s->wlog_waves = 0;
    if (hipMalloc(reinterpret_cast<void**>(&s->d_wlog), slots * kWlogCap * sizeof(uint2)) != hipSuccess
        || hipMalloc(reinterpret_cast<void**>(&s->d_wpix), slots * kWlogCap * sizeof(uint4)) != hipSuccess
        || hipMalloc(reinterpret_cast<void**>(&s->d_wlog_n), slots * 4) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    s->wlog_waves = slots;
    return true;
}
// Wave logs for this launch: allocates them on first use and puts them into `a`; false: the plane.
bool wave_logs_for(ffs_stream* s, ThresholdArgs& a, const StreamGeometry& g, const Rerun& how) {
    if (!wave_logs_possible(s, a, how)) return false;
    size_t slots = stream_log_slots(g);
    // Sized ONCE, for the largest launch any batch of this stream can make (1 .. max_batch frames), so that a batch of another
    // size never re-allocates: hipFree synchronises the whole device, i.e. every other worker's batches in flight.  (A stream is
    // idle here -- submit refuses a busy one, and a re-run inside ffs_wait comes after the batch's last event -- so nothing of
    // its own has to be waited for if it does happen: a tuning change between batches.)
    if (slots > s->wlog_waves) slots = std::max(slots, max_stream_log_slots(s->ctx->L, s->ctx->settings.pixel_bytes, a.frame_stride, s->max_batch, s->ctx->tune));
    if (!ensure_wave_logs(s, slots)) return false;
    a.wlog = s->d_wlog;
    a.wlog_n = s->d_wlog_n;
    a.wpix = s->d_wpix;
    return true;
}

// The threshold stage where all of it runs in s->st (ffs_internal.hpp): the dense kernel ...
void launch_dense_kernel(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, const StreamGeometry& g, uint32_t n_frames, hipEvent_t start,
                         hipEvent_t stop, bool plane_clean, bool counts_clean) {
    if (route.ext()) launch_ext_first(s, route, a, g, n_frames, start, stop, true, plane_clean, counts_clean);
    else if (route.stage == ThresholdStage::kRadial) launch_radthr_hist(s, a, n_frames, start, stop);
    else if (route.stage == ThresholdStage::kWindow) launch_window(s, route, a, n_frames, start, stop);
    else launch_stream(s, a, g, start, stop);
}
// ... and what follows it
void launch_dense_rest(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, uint32_t n_frames) {
    if (route.ext()) launch_ext_rest(s, route, a, n_frames, s->st);
    else if (route.stage == ThresholdStage::kRadial) launch_radthr_rest(s, a, n_frames, nullptr);
    else if (route.stage == ThresholdStage::kWindow) return;   // (it decides every pixel itself)
    else if (route.bright_to_plane) launch_exact(s, route, a, n_frames, s->st);
    else if (!a.wlog) launch_bright_fix(s, a, s->st);   // (with wave logs the sparse launch decides the bright windows)
}

int check_layout(ffs_stream* s, size_t pitch, size_t fstride, uint32_t n_frames) {
    ffs_ctx* c = s->ctx;
    if (n_frames == 0 || n_frames > s->max_batch) {
        c->err = "n_frames must be in 1..max_batch";
        return FFS_ERR_INVALID;
    }
    if (pitch % 16 || pitch < (size_t)c->L.pitch_px * c->settings.pixel_bytes || pitch >= (1ull << 32)
        || fstride < pitch * c->L.H || (pitch * c->L.H) >= (1ull << 32)) {
        c->err = "device layout: pitch must be a multiple of 16 bytes and >= round_up(width,128)*pixel_bytes; "
                 "frame_stride >= pitch*height";
        return FFS_ERR_INVALID;
    }
    return FFS_OK;
}

#ifdef FFS_EXPERIMENTS
// (experiment) occupies slots for a given time without touching memory
__global__ void k_dummy_spin(uint32_t ticks, uint32_t* sink) {
    extern __shared__ uint32_t s_dummy[];
    const uint64_t t0 = wall_clock64();
    uint32_t it = 0;
    while (wall_clock64() - t0 < ticks && it < (1u << 20)) { __builtin_amdgcn_s_sleep(20); ++it; }
    if (it == 0xFFFFFFFFu) { s_dummy[threadIdx.x] = it; *sink = s_dummy[0]; }
}
#endif

// The sparse stage in small workgroups (kernels_band.hpp, tuning "sparse_bands"): can this launch geometry take it, and are the
// buffers between its two kernels there (allocated once, for the most bands any batch of this stream can have).
// The three buffers hold `slots` (frame, band) pairs; false: no memory for them.
static bool ensure_band_buffers(ffs_stream* s, uint32_t slots) {
    if (slots <= s->band_slots) return true;
    if (s->d_band_hdr) {
        (void)hipFree(s->d_band_hdr); (void)hipFree(s->d_band_acc); (void)hipFree(s->d_band_seam);
        s->d_band_hdr = nullptr; s->d_band_acc = nullptr; s->d_band_seam = nullptr;
    }
    s->band_slots = 0;
    if (hipMalloc(reinterpret_cast<void**>(&s->d_band_hdr), (size_t)slots * sizeof(uint4)) != hipSuccess
        || hipMalloc(reinterpret_cast<void**>(&s->d_band_acc), (size_t)slots * kBandCompStride * sizeof(ChainAcc)) != hipSuccess
        || hipMalloc(reinterpret_cast<void**>(&s->d_band_seam), (size_t)slots * 2 * kBandSeamCap * 4) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    s->band_slots = slots;
    return true;
}
static bool band_stage_for(ffs_stream* s, const StreamGeometry& g, size_t fstride, uint32_t n_frames) {
    const ffs_ctx* c = s->ctx;
    if (!band_plan_holds(g, c->L, c->settings.pixel_bytes)) return false;
    uint32_t slots = band_slots(g, n_frames);
    // (sized once: hipFree synchronises the device -- see wave_logs_for)
    if (slots > s->band_slots) slots = std::max(slots, max_band_slots(c->L, c->settings.pixel_bytes, fstride, s->max_batch, c->tune));
    return ensure_band_buffers(s, slots);
}

// ---- one batch ------------------------------------------------------------------------------------------------------
// enqueue_batch() reads top to bottom: plan_batch() takes every decision of the batch, once, into a BatchPlan; reset_for_batch()
// clears what earlier batches left behind; launch_threshold_stage() enqueues the dense kernels and makes the batch's sparse stream
// wait for them; launch_sparse_stage() enqueues compaction -> connected components -> records behind that, and the batch's last
// event.  The three steps that launch branch on the plan and decide nothing again.

struct BatchPlan {
    uint32_t n = 0;                   // frames of the batch
    bool wait_upload = false;         // the frames are in place behind ev[1] (upload / decode stream): waited for in the dense stream this batch's first kernel takes
    bool counts_were_clean = false;   // the per-tile counts were zero before this batch's resets (the extended first pass then leaves out its own fill)
    // The extended algorithm (first pass -> erosion -> final pass).  Every other batch is "streamed": the plane the sparse stage
    // reads was produced by a streaming kernel into a zeroed plane (and is zeroed again by the compaction); path 0 also keeps the
    // occupancy bitmap in step with it
    bool ext = false;
    bool ext_sparse_erode = false;    // ... whose signal-region plane is cleared behind the previous batch together with the first-pass plane (ext_sparse_erode())
    bool radial = false;              // the radial-profile threshold (kernels_radthr.hpp) decides every pixel itself, like the general-window kernel: no list, no fix-up, no logs
    bool window = false;              // the general-window kernel (kernels_window.hpp) decides every pixel itself: no bright-window list, no fix-up, no wave logs
    bool list_path = false;           // a streaming kernel that hands its bright windows to k_bright_fix on a list (threshold path 0)
    bool aside = false;               // the context has sparse streams: the dense stream holds streaming kernels only
    bool will_chain = false;          // the whole sparse stage in one launch (k_frame_chain, or k_band_cc + k_frame_merge: `banded`); false: the four grid-wide kernels
    bool runs_ok = false;             // ... and its run-based instantiation can take frames beyond the LDS forest of pixels
    bool dense_batch = false;         // the stream's previous batch held a frame beyond that forest
    bool use_log = false;             // the streaming kernel writes wave logs (ta_launch has them) and the one launch merges them: no plane, no counters, no bright list
    bool runs_launch = false;         // the one launch is k_frame_chain's run-based instantiation
    bool need_lists = false;          // somebody reads the strong-pixel lists of this batch
    bool banded = false;              // the one launch is k_band_cc + k_frame_merge, `band` says how the streaming launch's bands are split for it
    bool chain_first = false;         // the one launch does the bright-window fix-up and the next streaming kernel waits for its start
    bool want_dense_bytes = false;    // the byte mask of this batch is produced
    ThresholdRoute route{};           // which threshold stage and which form of the predicate (threshold_route.hpp)
    StreamGeometry geo{};             // the streaming launch's geometry: super rows, strips, bands (launch_geometry.hpp)
    ThresholdArgs ta{};               // the threshold stage's arguments ...
    ThresholdArgs ta_launch{};        // ... and with the wave logs, for the streaming kernel and the one launch that reads them (== ta without logs)
    BandSplit band;
    uint32_t path_bits = 0;           // FFS_PATH_*: what ffs_stream_last_path reports for this batch
};

// Reads the stream, its context and tuning, the batch's settings (s->batch) and the previous batch's counts; `how`: what a
// re-run overrides.  Changes nothing of the stream but what is allocated on first use (wave logs, the band stage's buffers).
static BatchPlan plan_batch(ffs_stream* s, const void* d_img, size_t pitch, size_t fstride, uint32_t n, const Rerun& how) {
    ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    const ffs_params& p = s->batch.params;
    BatchPlan P;
    P.n = n;
    P.wait_upload = s->st_up != s->st && !s->dev_input;
    P.counts_were_clean = !s->counts_dirty;
    P.route = batch_route(s, how);
    P.ext = P.route.ext();
    P.ext_sparse_erode = ext_sparse_erode(c->tune);
    P.geo = batch_stream_geometry(s, fstride, n);
    P.ta = make_threshold_args(s, d_img, pitch, fstride, n, P.geo, P.route);
    P.window = P.route.stage == ThresholdStage::kWindow;
    P.radial = P.route.stage == ThresholdStage::kRadial;
    P.list_path = P.route.stage == ThresholdStage::kStreamList;
    // (the byte mask: zero-filled by the streaming kernels only when asked for; the exact stages always produce it)
    P.want_dense_bytes = (P.window || P.radial) ? (p.want_strong_mask || c->tune.dense_mask)
                                  : (P.list_path || (P.ext && P.route.ext_streams_first())) ? P.ta.dense_mask != 0 : true;
    // The whole sparse stage in one launch, one workgroup per frame (kernels_chain.hpp) ...
    const bool can_chain = c->tune.sparse_stage >= 2 && L.H <= 65535 && c->chain_ok && s->direct_recs && s->h_counts_dev
                           && c->n_tiles <= kChainMaxTiles && L.H <= kChainMaxRows;
    // ... as long as the frames' strong pixels fit its LDS forest.  A frame beyond that runs the same stages on global arrays
    // inside its one workgroup (2.8 ms for 32 frames of 61 k strong pixels, the extended algorithm on the bench frames),
    // where the four grid-wide kernels spread the work over the machine: the path of this batch follows what the stream's
    // previous batch held (data that is dense stays dense; a single dense frame costs one slow batch).
    // Denser frames of 16-bit pixels stay in the one launch while their RUNS fit LDS (kernels_chain.hpp, the RUNS instantiation:
    // 61 k strong pixels are 12 k runs on the bench frames of the extended algorithm); a frame with more runs than that raises
    // kOvfRuns, ffs_wait() runs the batch again through the grid-wide kernels and the stream stays with them for dense batches.
    P.runs_ok = c->settings.pixel_bytes == 2 && L.W <= kChainRunMaxW && c->tune.chain_runs != 0 && !s->runs_overflowed;
    if (can_chain && c->tune.sparse_stage == 2 && s->n_frames > 0) {
        uint32_t prev_max = 0;
        for (uint32_t f = 0; f < s->n_frames; ++f) prev_max = std::max(prev_max, s->h_counts[counts_strong_at(s->max_batch) + f]);
        P.dense_batch = prev_max > (uint32_t)kChainLdsEntries;
    }
    P.will_chain = can_chain && (!P.dense_batch || P.runs_ok) && !how.grid;
    // Wave logs instead of the plane (tuning "strong_log"): the standard 16-bit path, sparse stage in the one launch, frames
    // that fit its LDS forest.  The streaming kernel then leaves plane, counters, occupancy bitmap and bright list alone.
    P.ta_launch = P.ta;
    P.use_log = P.list_path && P.will_chain && !P.dense_batch && wave_logs_for(s, P.ta_launch, P.geo, how);
#ifdef FFS_EXPERIMENTS
    if (c->tune.exp.chain_skip) P.will_chain = false;   // (use_log stays what it was with the one launch)
#endif
    // (the launch that merges wave logs and the run-based launch of dense frames can do without the lists)
    P.runs_launch = P.will_chain && !P.use_log && P.runs_ok && (P.dense_batch || c->tune.chain_runs == 2);
    P.aside = !P.ext && s->st2 != s->st;
    const int depth = c->inflight.load() + (s->busy ? 0 : 1);
    // The sparse stage in small workgroups (kernels_band.hpp): wave logs, nobody reads the pixel lists or the byte mask, a geometry
    // its LDS plan holds, and the stream's recent batches did not overflow that plan.
    P.need_lists = p.want_strong_list || c->tune.device_lists == 1 || (c->tune.device_lists == 2 && g_live_stacks.load() > 0);
    // By pipeline depth (tuning "sparse_bands" = 1): its two launches each become ready behind a streaming kernel that is already
    // being dispatched, so a batch's results are two steps away -- hidden with four batches in flight (101 k against 95.6 k frames/s),
    // not with two or three (79 k / 89 k against 88 k / 95 k for the one-workgroup launch with its head start); alone in flight the
    // band waves win again (58 k against 53 k: nothing to wait behind).  profiles/r05n_bands_by_pipeline_depth.log
    // A context with four or more streams is a pipeline that FILLS through depths two and three (the start of a run, of a timed
    // region): there the band launches win at every depth (+1.2 % on the driver-style line, profiles/r05zo_tune_ab.log).
    const bool depth_ok = c->tune.sparse_bands >= 2 || depth >= 4 || depth <= 1 || c->n_streams_made >= 4;
    P.banded = P.use_log && c->tune.sparse_bands != 0 && depth_ok && !P.need_lists && !P.ta.dense_mask && !how.no_bands && s->band_backoff == 0
               && band_stage_for(s, P.geo, fstride, n);
    if (P.banded) P.band = band_split(P.geo);
    // chain_first: the one launch, one workgroup per frame, of a list-path batch on a context with sparse streams ...
    // ... which then also does the bright-window fix-up, and whose workgroups (a whole CU each) should get their CUs
    // BEFORE the next batch's streaming kernel floods the dispatcher: that kernel waits for this launch to have STARTED.
    // (Without it a batch's sparse launch sits out the whole next streaming kernel: 0.35 ms more latency per batch.)
    // Only while few batches are in flight: with a deep pipeline the latency is hidden anyway, the wait costs the dense
    // stream ~15 us per batch and the fix-up inside the one-workgroup-per-frame launch ~25 us of its CUs (4 batches in
    // flight: 0.369-0.377 against 0.353 ms per step; 2 in flight: 0.385 against 0.523).
    // (band waves fit wherever a streaming wave has left: they need no head start)
    P.chain_first = P.list_path && P.aside && P.will_chain && !P.banded && c->tune.chain_first > 0 && depth <= c->tune.chain_first;
    P.path_bits = (P.use_log ? FFS_PATH_WAVE_LOGS : 0u) | (P.will_chain && !P.banded ? FFS_PATH_FRAME_CHAIN : 0u) | (P.banded ? FFS_PATH_BANDS : 0u)
                  | (P.runs_launch ? FFS_PATH_RUNS : 0u) | (!P.will_chain ? FFS_PATH_GRID_KERNELS : 0u) | (P.ext ? FFS_PATH_EXTENDED : 0u)
                  | (P.window ? FFS_PATH_WINDOW : 0u) | (P.radial ? FFS_PATH_RADIAL_THRESHOLD : 0u)
                  | (P.radial && s->batch.radial_blur ? FFS_PATH_RADIAL_BLUR : 0u);
    return P;
}

// Extended algorithm: this batch's planes are the ones cleared behind the previous batch (d_dplane2 / d_eplane2 keep that batch's).
// plane_clean: the first-pass plane is zero already.
static int take_extended_planes(ffs_stream* s, bool& plane_clean) {
    plane_clean = false;
    s->ext_e_clean = false;
    if (s->batch.params.algorithm != FFS_ALGO_DISPERSION_EXTENDED) return FFS_OK;
    FFS_TRY(ensure_extended_buffers(s));
    std::swap(s->d_dplane, s->d_dplane2);
    std::swap(s->d_eplane, s->d_eplane2);
    plane_clean = s->dplane2_clean;
    s->ext_e_clean = s->dplane2_clean && s->eplane2_clean && ext_sparse_erode(s->ctx->tune);
    s->dplane2_clean = false;
    s->eplane2_clean = false;
    return FFS_OK;
}

// What an earlier batch left behind and this one needs zero, filled in the stream's own dense stream.  dense_resets: there were
// such fills, and this batch's kernel has to follow them there.
static int reset_for_batch(ffs_stream* s, const BatchPlan& plan, bool& dense_resets) {
    ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    dense_resets = false;
    // (the extended algorithm waits for its frames ahead of all its fills; every other path where its first kernel goes: launch_threshold_stage)
    if (plan.wait_upload && plan.ext) HIP_TRY(c, hipStreamWaitEvent(s->st, s->ev[1], 0));
    if (!plan.ext && s->bits_dirty) {  // (another algorithm or a failed batch left bits behind)
        HIP_TRY(c, hipMemsetAsync(s->d_bits, 0, (size_t)s->max_batch * L.plane_frame_stride, s->st));
        dense_resets = true;
    }
    if (!plan.ext && s->counts_dirty) {
        HIP_TRY(c, hipMemsetAsync(s->d_tile_counts, 0, tile_counts_bytes(s), s->st));
        dense_resets = true;
    }
    if (s->occ_dirty) {
        HIP_TRY(c, hipMemsetAsync(s->d_occ, 0, (size_t)s->max_batch * occ_frame_words(L) * 4, s->st));
        s->occ_dirty = false;
        dense_resets = true;
    }
    s->counts_dirty = true;
    s->bits_dirty = true;  // until every launch of this batch is enqueued (a failure in between leaves bits behind)
    return FFS_OK;
}

// ---- ... its threshold stage ----------------------------------------------------------------------------------------
// What the arms of launch_threshold_stage share.  The frames are in place: waited for in the stream the batch's first kernel takes ...
static int wait_for_upload(ffs_stream* s, const BatchPlan& plan, hipStream_t st) {
    if (plan.wait_upload) HIP_TRY(s->ctx, hipStreamWaitEvent(st, s->ev[1], 0));
    return FFS_OK;
}
// ... and the stage's output is: ev[2], recorded behind the stage's kernels in s->st unless it rode on a dispatch, and waited for by
// the batch's sparse stream
static int sparse_stream_follows(ffs_stream* s, bool ev2_on_dispatch) {
    if (!ev2_on_dispatch) HIP_TRY(s->ctx, hipEventRecord(s->ev[2], s->st));
    if (s->st2 != s->st) HIP_TRY(s->ctx, hipStreamWaitEvent(s->st2, s->ev[2], 0));
    return FFS_OK;
}

// Wave-log path with a deep pipeline: the context's two dense HIP streams take the streaming kernels alternately (ffs_internal.hpp,
// "dense_overlap"): this launch waits for the value the PREVIOUS launch's last workgroup wrote as it started, not for that
// kernel's end, and writes its own.  Everything that must precede the kernel (the upload's event) goes into the same stream.
// launched = false: not on this device (the caller launches as without the tuning).
static int launch_stream_overlapped(ffs_stream* s, const BatchPlan& plan, hipEvent_t ev_start, bool& launched) {
    ffs_ctx* c = s->ctx;
    launched = false;
    std::lock_guard<std::mutex> dense_lock(c->dense_mu);   // (several threads submit to one context: a launch's number, stream and wait are one step)
    if (!c->dense_st2) {   // the partner stream and the hand-over word: made on first use (nothing of this exists in a context that never asks)
        int lo = 0, hi = 0, can = 0;
        bool ok = hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, c->device) == hipSuccess && can
                  && hipExtMallocWithFlags(reinterpret_cast<void**>(&c->d_handoff), 8, hipMallocSignalMemory) == hipSuccess;
        ok = ok && hipMemsetAsync(c->d_handoff, 0, 8, c->up_st) == hipSuccess && hipStreamSynchronize(c->up_st) == hipSuccess;
        ok = ok && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess
             && hipStreamCreateWithPriority(&c->dense_st2, hipStreamNonBlocking, (lo + hi) / 2) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (c->d_handoff) (void)hipFree(c->d_handoff);
            c->d_handoff = nullptr;
            c->dense_st2 = nullptr;
            c->tune.dense_overlap = 0;   // (not on this device)
            return FFS_OK;
        }
    }
    const uint32_t seq = ++c->handoff_seq;
    const int which = (int)(seq & 1u);
    hipStream_t dst = which ? c->dense_st2 : c->dense_st;
    FFS_TRY(wait_for_upload(s, plan, dst));
    if (c->handoff_last >= 0 && c->handoff_last != which)
        HIP_TRY(c, hipStreamWaitValue32(dst, c->d_handoff, seq - 1, hipStreamWaitValueGte, 0xFFFFFFFFu));
    ThresholdArgs a = plan.ta_launch;
    a.handoff = c->d_handoff;
    a.handoff_seq = seq;
    launch_stream(s, a, plan.geo, ev_start, s->ev[2], dst);
    c->handoff_last = which;
    launched = true;
    return FFS_OK;
}

static int launch_threshold_stage(ffs_stream* s, const BatchPlan& plan, bool dense_resets, bool ext_plane_clean) {
    ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    const ThresholdArgs& ta = plan.ta;
    const uint32_t n = plan.n;
    if (plan.chain_first) {
        std::lock_guard<std::mutex> lock(c->stream_mu);   // (the newest start event cannot be re-recorded between the two lines)
        const int slot = c->chain_ev_newest.load();
        if (slot >= 0) HIP_TRY(c, hipStreamWaitEvent(s->st, c->chain_ev[slot], 0));
    }
    hipEvent_t ev_start = nullptr;
    if (s->ev1_pending) { ev_start = s->ev[1]; s->ev1_pending = false; }
    if (plan.ext && s->st2 != s->st && c->tune.ext_rest_aside) {
        // The dense stream carries the first pass alone; erosion and the final pass -- a latency-bound gather over the signal
        // region that keeps the vector units half busy -- go to the batch's sparse stream, ahead of its sparse launch, and run
        // BESIDE the next batch's first pass (an issue-bound stream of the whole frame) instead of between two of them.
        const bool streams = plan.route.ext_streams_first();   // (the first pass's stop event rides on its dispatch; the bright-window fix-up goes aside too)
        launch_ext_first(s, plan.route, ta, plan.geo, n, ev_start, streams ? s->ev[2] : nullptr, false, ext_plane_clean, plan.counts_were_clean);
        FFS_TRY(sparse_stream_follows(s, streams));
        if (streams) hipLaunchKernelGGL((k_bright_fix<uint16_t, true>), dim3(32), dim3(256), 0, s->st2, ta);
        launch_ext_rest(s, plan.route, ta, n, s->st2);
    } else if (plan.window) {
        // The plane, the per-tile counts, the byte mask when it is asked for and the occupancy bitmap when the one-launch sparse stage
        // reads it: what that stage reads after k_exact
        ThresholdArgs tw = ta;
        tw.dense_mask = plan.want_dense_bytes ? 1 : 0;
        tw.occ = (c->tune.occupancy_bitmap && plan.will_chain) ? s->d_occ : nullptr;
        FFS_TRY(wait_for_upload(s, plan, s->st));
        launch_window(s, plan.route, tw, n, ev_start, s->ev[2]);
        FFS_TRY(sparse_stream_follows(s, true));
    } else if (plan.radial) {
        // The same outputs from the radial-profile threshold's three launches: the histogram (behind the fill that zeroes its tables), the
        // cutoffs, the strong pixels
        ThresholdArgs tr = ta;
        tr.dense_mask = plan.want_dense_bytes ? 1 : 0;
        tr.occ = (c->tune.occupancy_bitmap && plan.will_chain) ? s->d_occ : nullptr;
        FFS_TRY(radthr_ensure_buffers(s));
        FFS_TRY(wait_for_upload(s, plan, s->st));
        launch_radthr_hist(s, tr, n, ev_start, nullptr);
        launch_radthr_rest(s, tr, n, s->ev[2]);
        FFS_TRY(sparse_stream_follows(s, true));
    } else if (plan.list_path && plan.aside) {
        // the bright-window fix-up goes to the sparse stream (or into the sparse launch itself: chain_first; with wave logs the
        // sparse launch decides those pixels as it reads the logs)
        bool launched = false;
        if (plan.use_log && !plan.chain_first && !dense_resets && c->tune.dense_overlap != 0 && s->st == c->dense_st)
            FFS_TRY(launch_stream_overlapped(s, plan, ev_start, launched));
        if (!launched) {
            FFS_TRY(wait_for_upload(s, plan, s->st));
            launch_stream(s, plan.ta_launch, plan.geo, ev_start, s->ev[2]);
        }
        FFS_TRY(sparse_stream_follows(s, true));
        if (!plan.chain_first && !plan.use_log) launch_bright_fix(s, ta, s->st2);
    } else if (plan.route.stage == ThresholdStage::kCrossCheck) {
        // the cross-check path of `spotfinder --validate` (tuning "threshold_path" = 2): no streaming kernel, no screen, no LDS
        // queue -- the plane starts as the valid-pixel mask, so k_exact gathers the window of EVERY valid pixel from memory and
        // applies the oracle's predicate to 64-bit sums (exact_strong).  Shares nothing with the hot path but that predicate.
        FFS_TRY(wait_for_upload(s, plan, s->st));
        if (ev_start) HIP_TRY(c, hipEventRecord(ev_start, s->st));
        HIP_TRY(c, hipMemsetAsync(s->d_sbytes, 0, (size_t)n * L.bytes_frame_stride, s->st));
        for (uint32_t f = 0; f < n; ++f)
            HIP_TRY(c, hipMemcpyAsync(s->d_bits + (size_t)f * L.plane_frame_stride, c->d_maskbits, L.plane_frame_stride, hipMemcpyDeviceToDevice, s->st));
        launch_exact(s, plan.route, ta, n, s->st);
        FFS_TRY(sparse_stream_follows(s, false));
    } else {
        // the whole stage in the dense stream: the streaming kernel + k_bright_fix (path 0 on a context without sparse streams) or
        // + k_exact (path 1); the extended algorithm's first pass + erosion + final pass
        if (!plan.ext) FFS_TRY(wait_for_upload(s, plan, s->st));   // (extended: waited for already, reset_for_batch)
        launch_dense_kernel(s, plan.route, ta, plan.geo, n, ev_start, nullptr, ext_plane_clean, plan.counts_were_clean);
        launch_dense_rest(s, plan.route, ta, n);
        FFS_TRY(sparse_stream_follows(s, false));
    }
    HIP_TRY(c, hipGetLastError());
    return FFS_OK;
}

// ---- ... and its sparse stage ---------------------------------------------------------------------------------------
static CclArgs make_ccl_args(const ffs_stream* s, const BatchPlan& plan) {
    const ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    CclArgs ca{};
    ca.image = plan.ta.image;
    ca.frame_stride = plan.ta.frame_stride;
    ca.pitch = plan.ta.pitch;
    ca.bits = s->d_bits;
    ca.clear_bits = plan.ext ? 0 : 1;
    ca.tile_counts = s->d_tile_counts;
    ca.num_strong = s->d_num_strong;
    ca.row_off = s->d_row_off;
    ca.list_k = s->d_list_k;
    ca.list_i = s->d_list_i;
    ca.parent = s->d_parent;
    ca.n_comp = s->d_n_comp;
    ca.overflow = s->d_overflow;
    ca.W = L.W;
    ca.H = L.H;
    ca.pitch_px = L.pitch_px;
    ca.mpitch = L.mpitch;
    ca.plane_frame_stride = L.plane_frame_stride;
    ca.n_tiles = c->n_tiles;
    ca.cap = s->cap;
    ca.max_comp = s->max_comp;
    ca.pixel_bytes = c->settings.pixel_bytes;
    ca.strong_bytes = s->d_sbytes;
    ca.bpitch = L.bpitch;
    ca.bytes_frame_stride = L.bytes_frame_stride;
    ca.acc2 = s->d_acc2;
    ca.summary = s->d_summary;
    ca.dense_bytes = plan.want_dense_bytes ? 1 : 0;
    ca.need_lists = plan.need_lists ? 1 : 0;
    ca.occ = s->d_occ;
    ca.occ_frame_words = occ_frame_words(L);
    ca.occ_spr = L.mpitch / 16;
    // only the streaming kernels and their fix-up keep the bitmap (path 1: a superset of the final plane, which is fine)
    ca.use_occ = (c->tune.occupancy_bitmap && plan.ta.bright_to_plane != 2) ? 1 : 0;   // (kept by the streaming kernels, their fix-up and the extended algorithm's final pass)
    return ca;
}
static SegArgs make_seg_args(const ffs_stream* s, const BatchPlan& plan) {
    const ffs_ctx* c = s->ctx;
    const Layout& L = c->L;
    SegArgs sa{};
    sa.list_k = s->d_list_k;
    sa.list_i = s->d_list_i;
    sa.parent = s->d_parent;
    sa.seg_n = s->d_num_strong;
    sa.seg_stride = s->cap;
    sa.n_comp = s->d_n_comp;
    sa.max_comp = s->max_comp;
    sa.overflow = s->d_overflow;
    sa.W = (uint32_t)L.W;
    sa.H = (uint32_t)L.H;
    sa.row_off = s->d_row_off;
    sa.n_slices = 1;
    sa.min_spot_size = s->batch.params.min_spot_size;
    sa.max_sep = s->batch.params.max_peak_centroid_separation;
    sa.summary = s->d_summary;
    sa.acc2 = s->d_acc2;
    sa.zero_counts = s->d_tile_counts;
    sa.zero_per_seg = (uint32_t)c->n_tiles;
    sa.zero_word = s->d_tile_counts + tile_counts_bytes(s) / 4 - 1;
    return sa;
}

// every launch of the batch is enqueued: what it leaves of plane and counts, and the batch is in flight
static int finish_enqueue(ffs_stream* s, uint32_t n, bool bits_dirty, bool counts_dirty) {
    s->bits_dirty = bits_dirty;
    s->counts_dirty = counts_dirty;
    mark_busy(s);
    s->n_frames = n;
    s->radial_pending = true;   // (the batch is in flight: its wait hands out its profile, or that it has none)
    return FFS_OK;
}

using ChainKernel = void (*)(ChainArgs);
static ChainKernel frame_chain_kernel(const BatchPlan& plan, int pixel_bytes) {
    if (plan.use_log) return pixel_bytes == 2 ? k_frame_chain<uint16_t, false, true> : k_frame_chain<uint32_t, false, true>;
    if (plan.runs_launch) return k_frame_chain<uint16_t, true>;   // (runs_ok: 16-bit pixels)
    return pixel_bytes == 2 ? k_frame_chain<uint16_t> : k_frame_chain<uint32_t>;
}

// The one launch (plan.will_chain): k_frame_chain, a workgroup per frame, or -- banded -- k_band_cc + k_frame_merge.  Counters and
// records go straight to the host: one event behind it.
static int launch_one_launch_stage(ffs_stream* s, const BatchPlan& plan, const CclArgs& ca, const SegArgs& sa) {
    ffs_ctx* c = s->ctx;
    const uint32_t n = plan.n;
    ChainArgs A{};
    A.c = ca;
    A.s = sa;
    A.s.recs = s->h_recs_dev;
    A.h_counts = s->h_counts_dev;
    A.max_batch = (uint32_t)s->max_batch;
    A.rec_stride = s->max_comp;
#ifdef FFS_EXPERIMENTS
    A.stop_after = c->tune.exp.chain_stop;
    if (std::getenv("FFS_EXP_CHAIN_TS")) {
        if (!s->h_phase_ts && hipHostMalloc(reinterpret_cast<void**>(&s->h_phase_ts), (size_t)s->max_batch * 64, hipHostMallocDefault) == hipSuccess) {
            std::memset(s->h_phase_ts, 0, (size_t)s->max_batch * 64);
            (void)hipHostGetDevicePointer(reinterpret_cast<void**>(&s->h_phase_ts_dev), s->h_phase_ts, 0);
        }
        A.phase_ts = s->h_phase_ts_dev;
    }
#endif
    A.t = plan.ta_launch;
    A.fix_bright = (plan.chain_first && !plan.use_log) ? 1 : 0;
    A.fix_done = s->d_tile_counts + tile_counts_bytes(s) / 4 - 2;
    A.runs_ok = plan.runs_ok ? (c->tune.chain_runs == 2 ? 2 : 1) : 0;
    {
        // the launch's start event belongs to the context (ffs_internal.hpp); published under the lock the waiting side takes
        std::lock_guard<std::mutex> lock(c->stream_mu);
        const int slot = (int)(c->chain_ev_next.fetch_add(1) % ffs_ctx::kChainEvents);
        if (plan.banded) {
            BandArgs BA{};
            BA.A = A;
            BA.hdr = s->d_band_hdr;
            BA.acc = reinterpret_cast<ChainAcc*>(s->d_band_acc);
            BA.seam = s->d_band_seam;
            BA.sub = plan.band.sub;
            BA.sub_rows = plan.band.sub_rows;
            const dim3 gb((unsigned)(plan.ta_launch.n_bands * BA.sub), n);
            if (c->settings.pixel_bytes == 2) hipExtLaunchKernelGGL(k_band_cc<uint16_t>, gb, dim3(64), 0, s->st2, c->chain_ev[slot], nullptr, 0, BA);
            else hipExtLaunchKernelGGL(k_band_cc<uint32_t>, gb, dim3(64), 0, s->st2, c->chain_ev[slot], nullptr, 0, BA);
            hipLaunchKernelGGL(k_frame_merge, dim3(n), dim3(kMergeThreads), 0, s->st2, BA);
        } else {
            hipExtLaunchKernelGGL(frame_chain_kernel(plan, c->settings.pixel_bytes), dim3(n), dim3(kChainThreads), kChainDynBytes, s->st2, c->chain_ev[slot], nullptr, 0, A);
        }
        if (plan.aside) c->chain_ev_newest.store(slot);
    }
    HIP_TRY(c, hipGetLastError());
    if (plan.ext && plan.route.ext_streams_first() && s->st2 != s->st) {
        // the plane the previous batch used (nobody reads it any more) is cleared here, beside the dense kernels, for the next batch
        // (with the strip erosion the signal-region plane behind it too: one fill, the two are one allocation)
        HIP_TRY(c, hipMemsetAsync(s->d_dplane2, 0, (size_t)s->max_batch * c->L.plane_frame_stride * (plan.ext_sparse_erode ? 2u : 1u), s->st2));
        s->dplane2_clean = true;
        s->eplane2_clean = plan.ext_sparse_erode;
    }
    FFS_TRY(launch_radial_stage(s, n));
    FFS_TRY(join_pixel_stats(s));
    HIP_TRY(c, hipEventRecord(s->ev[4], s->st2));
    s->ev3_is_ev4 = true;
    s->spec_recs_copied = (uint64_t)s->max_batch * s->max_comp;
    return finish_enqueue(s, n, plan.ext, false);
}

// the same stages as four grid-wide kernels (frames taller than k_frame_chain's LDS plan, records not written to the
// host directly, tuning "sparse_stage" = 1)
static int launch_grid_stage(ffs_stream* s, const BatchPlan& plan, const CclArgs& ca, SegArgs sa) {
    ffs_ctx* c = s->ctx;
    const uint32_t n = plan.n;
    bool skip_sparse = false;
#ifdef FFS_EXPERIMENTS
    if (c->tune.exp.chain_skip) {
        skip_sparse = true;
        if (c->tune.exp.dummy_us > 0)
            hipLaunchKernelGGL(k_dummy_spin, dim3(c->tune.exp.dummy_wg), dim3(c->tune.exp.dummy_threads),
                               (size_t)c->tune.exp.dummy_lds, s->st2, (uint32_t)c->tune.exp.dummy_us * 100u, s->d_tile_counts);
    }
#endif
    if (!skip_sparse) {
        sa.recs = s->direct_recs ? (void*)s->h_recs_dev : (void*)s->d_recs;
        sa.chunk_roots = s->d_chunk_roots;
        sa.chunks_max = s->cap / kRootChunk + 1;
        const dim3 gseg((unsigned)c->tune.ccl_grid, n), b256(256);
        if (c->settings.pixel_bytes == 2) hipLaunchKernelGGL(k_emit_list_w<uint16_t>, dim3(c->n_tiles, n), dim3(64), 0, s->st2, ca);
        else hipLaunchKernelGGL(k_emit_list_w<uint32_t>, dim3(c->n_tiles, n), dim3(64), 0, s->st2, ca);
        hipLaunchKernelGGL(k_union<false>, gseg, b256, 0, s->st2, sa);
        hipLaunchKernelGGL(k_reduce_roots, gseg, b256, 0, s->st2, sa);
        hipLaunchKernelGGL(k_finalize_roots, gseg, b256, 0, s->st2, sa);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(s->ev[3], s->st2));
    s->ev3_is_ev4 = false;

    // small counts first; ffs_wait() sizes the record copy from them
    const size_t B = s->max_batch;
    HIP_TRY(c, hipMemcpyAsync(s->h_counts, s->d_num_strong, counts_device_words(B) * 4, hipMemcpyDeviceToHost, s->st2));
    if (s->direct_recs) {
        s->spec_recs_copied = (uint64_t)B * s->max_comp;  // everything is on the host already
    } else {
        s->spec_recs_copied = std::min<uint64_t>((uint64_t)s->spec_recs_per_frame * n, (uint64_t)B * s->max_comp);
        HIP_TRY(c, hipMemcpyAsync(s->h_recs, s->d_recs, s->spec_recs_copied * sizeof(WireRec2), hipMemcpyDeviceToHost, s->st2));
    }
    FFS_TRY(launch_radial_stage(s, n));
    FFS_TRY(join_pixel_stats(s));
    HIP_TRY(c, hipEventRecord(s->ev[4], s->st2));
    // the compaction of a streamed batch leaves the plane all zero again; k_union cleared the counts of the frames of this batch (all
    // the streaming kernel touched)
    return finish_enqueue(s, n, plan.ext || skip_sparse, skip_sparse);
}

static int launch_sparse_stage(ffs_stream* s, const BatchPlan& plan) {
    const CclArgs ca = make_ccl_args(s, plan);
    const SegArgs sa = make_seg_args(s, plan);
    // what the batch leaves on the device, for ffs_wait and the accessors
    s->bits_cleared = ca.clear_bits != 0;
    s->lists_valid = !(plan.use_log || plan.runs_launch) || plan.need_lists;
    s->dense_valid = plan.want_dense_bytes;
    s->occ_dirty = !(ca.use_occ && plan.will_chain);      // nobody consumes (and clears) the bits this batch sets
    s->chain_mode = plan.will_chain;
    s->path_bits = plan.path_bits | (s->batch.radial_bins ? FFS_PATH_RADIAL : 0u) | (s->batch.pixel_stats ? FFS_PATH_PIXEL_STATS : 0u);
    return plan.will_chain ? launch_one_launch_stage(s, plan, ca, sa) : launch_grid_stage(s, plan, ca, sa);
}

int enqueue_batch(ffs_stream* s, const void* d_img, size_t pitch, size_t fstride, uint32_t n, const ParamSnapshot* snapshot, const Rerun& how) {
    s->batch = snapshot ? *snapshot : snapshot_of(s->ctx->settings);
    s->cur_img = d_img;
    s->cur_pitch = pitch;
    s->cur_fstride = fstride;
    (void)hipGetLastError();  // drop any stale error state: the checks below are for OUR launches
    bool ext_plane_clean = false;
    FFS_TRY(take_extended_planes(s, ext_plane_clean));
    const BatchPlan plan = plan_batch(s, d_img, pitch, fstride, n, how);
    // (the one thing planning changes in what the stream remembers: a batch that could take bands brings the stream one step back to
    // them after a band overflowed their plan -- ffs_wait.hip, decide_recovery, sets the 32)
    if (plan.use_log && s->band_backoff > 0 && !how.no_bands) --s->band_backoff;
    bool dense_resets = false;
    FFS_TRY(reset_for_batch(s, plan, dense_resets));
    FFS_TRY(launch_threshold_stage(s, plan, dense_resets, ext_plane_clean));
    FFS_TRY(launch_radial_dense(s, n));
    FFS_TRY(launch_pixel_stats(s, n));
    return launch_sparse_stage(s, plan);
}

extern "C" int ffs_submit_device(ffs_stream* s, const void* device_pixels, size_t pitch, size_t fstride,
                                 uint32_t n_frames, int64_t first_frame_id) {
    if (!s || !device_pixels || !stream_handle_ok(s)) return FFS_ERR_INVALID;
    ffs_ctx* c = s->ctx;
    if (s->busy) {
        c->err = "stream already has a batch in flight: call ffs_wait() first";
        return FFS_ERR_INVALID;
    }
    int rc = check_layout(s, pitch, fstride, n_frames);
    if (rc != FFS_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // (no marker here: every packet in the dense stream is ~5 us between two streaming kernels; enqueue_batch attaches
    // the start event to its first kernel where it can, or records it)
    s->dev_input = true;
    s->ev1_pending = true;
    s->first_id = first_frame_id;
    s->reruns = 0;
    s->radial_todo = true;
    s->stats_todo = true;
    rc = enqueue_batch(s, device_pixels, pitch, fstride, n_frames);
    if (rc == FFS_OK) ahead_register(s);
    return rc;
}

extern "C" int ffs_submit(ffs_stream* s, const void* host_pixels, uint32_t n_frames, int64_t first_frame_id) {
    if (!s || !host_pixels || !stream_handle_ok(s)) return FFS_ERR_INVALID;
    ffs_ctx* c = s->ctx;
    if (s->busy) {
        c->err = "stream already has a batch in flight: call ffs_wait() first";
        return FFS_ERR_INVALID;
    }
    if (n_frames == 0 || n_frames > s->max_batch) {
        c->err = "n_frames must be in 1..max_batch";
        return FFS_ERR_INVALID;
    }
    const Layout& L = c->L;
    HIP_TRY(c, hipSetDevice(c->device));
    s->radial_todo = true;
    s->stats_todo = true;
    s->dev_input = false;
    HIP_TRY(c, hipEventRecord(s->ev[0], s->st_up));
    // one 2D copy: the default device layout keeps frames contiguous (frame_stride = H * pitch)
    const size_t row = (size_t)L.W * c->settings.pixel_bytes;
    HIP_TRY(c, hipMemcpy2DAsync(s->d_img, L.pitch, host_pixels, row, row, (size_t)L.H * n_frames,
                                hipMemcpyHostToDevice, s->st_up));
    HIP_TRY(c, hipEventRecord(s->ev[1], s->st_up));
    s->first_id = first_frame_id;
    s->reruns = 0;
    const int rc = enqueue_batch(s, s->d_img, L.pitch, L.frame_stride, n_frames);
    if (rc == FFS_OK) ahead_register(s);
    return rc;
}
