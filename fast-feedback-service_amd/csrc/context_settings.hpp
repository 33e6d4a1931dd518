// context_settings.hpp -- what a context is set to, which of its settings combine, and what a batch takes of them at submit.  No HIP header:
// the setters of ffs_context.hip and ffs_products.hip ask the rules here before they touch anything, and a plain C++ test program
// (tests/context_settings_check.cc) holds every text and every rule against literals and against each other.  DESIGN.md section 3.3g has
// the pair rules as a table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <string>

#include "ffs_hip.h"
#include "radial_threshold_model.hpp"

namespace ffsamd {

// The settings of a context: what the ffs_ctx_set_* calls store, what the rules below read and what snapshot_of copies.  The device
// buffers behind gain_map, radial_bins and jungfrau_calibration are resources of ffs_ctx; here is only whether they are in force.
struct ContextSettings {
    ffs_params params{};                          // ffs_ctx_set_params (ffs_ctx_create: default_params())
    int max_valid_scope = FFS_MAX_VALID_CENTRE;   // ffs_ctx_set_max_valid_scope: kept across ffs_ctx_set_params, as everything below is
    double gain = 0.0;                            // ffs_ctx_set_gain (0 = off)
    bool gain_map = false;                        // ffs_ctx_set_gain_map: a map is in force
    uint32_t radial_bins = 0;                     // ffs_ctx_set_radial_bins: the bins of the map in force (0 = none)
    double n_iqr = 6.0;                           // ffs_ctx_set_radial_threshold
    int radial_blur = FFS_RADIAL_BLUR_NONE;       // ffs_ctx_set_radial_blur
    bool pixel_stats = false;                     // ffs_ctx_set_pixel_stats: batches submitted from now on are folded in
    bool jungfrau_calibration = false;            // ffs_ctx_set_jungfrau_calibration: a calibration is in force
    int pixel_bytes = 2;                          // ffs_ctx_create: 2 or 4, never changes
};

// What a batch is computed with: the context's settings as they were at submit (re-runs inside ffs_wait keep them).  A new per-batch
// setting is a new field here and a new line in snapshot_of.  gain_map: the context had a gain map at submit -- the route's input; the map
// itself is a property of the context like the mask, and cannot change while a batch is in flight (ffs_ctx_set_gain_map).
struct ParamSnapshot {
    ffs_params params{};
    int max_valid_scope = FFS_MAX_VALID_CENTRE;
    double gain = 0.0;
    bool gain_map = false;
    uint32_t radial_bins = 0;   // bins of the context's radial bin map at submit (0: no map): the batch computes a profile over that many bins
    bool pixel_stats = false;   // ffs_ctx_set_pixel_stats was on at submit: the batch's frames are folded into the context's per-pixel statistics, once
    // The radial-profile threshold (FFS_ALGO_RADIAL_PROFILE): the shells of the map at submit when the parameters say that
    // algorithm, else 0 -- its own field, because a one-frame re-run drops radial_bins (the profile is computed once) and still thresholds by
    // shell -- and n_iqr (ffs_ctx_set_radial_threshold).  The map itself is the context's, like the gain map.
    uint32_t radthr_bins = 0;
    double n_iqr = 6.0;
    int radial_blur = 0;        // ffs_ctx_set_radial_blur at submit (FFS_RADIAL_BLUR_*); plays a part only where radthr_bins does
};
inline ParamSnapshot snapshot_of(const ContextSettings& s) {
    ParamSnapshot b;
    b.params = s.params;
    b.max_valid_scope = s.max_valid_scope;
    b.gain = s.gain;
    b.gain_map = s.gain_map;
    b.radial_bins = s.radial_bins;
    b.pixel_stats = s.pixel_stats;
    b.radthr_bins = s.params.algorithm == FFS_ALGO_RADIAL_PROFILE ? s.radial_bins : 0u;
    b.n_iqr = s.n_iqr;
    b.radial_blur = s.radial_blur;
    return b;
}

// ---- parameters -----------------------------------------------------------------------------------------------------------------------
inline ffs_params default_params() {   // ffs_default_params
    ffs_params p;
    std::memset(&p, 0, sizeof(p));
    p.min_count = 2;  // baseline/spotfinder/standalone.cc:17
    p.nsig_b = 6.0;   // :19
    p.nsig_s = 3.0;   // :20
    p.threshold = 0.0;
    p.max_valid = -1;
    p.min_spot_size = 3;     // spotfinder/spotfinder.cc:321
    p.min_spot_size_3d = 3;  // :327
    p.max_peak_centroid_separation = 2.0f;  // :335
    p.want_reflections = 1;
    p.want_strong_list = 0;
    p.want_strong_mask = 0;
    p.algorithm = FFS_ALGO_DISPERSION;
    p.extended_flavour = 0;
    p.kernel_half_x = 3;     // standalone.cc:16 (kernel_size_ = 3,3)
    p.kernel_half_y = 3;
    return p;
}
// window half-sizes of a parameter set (ffs_params.kernel_half_x / _y: 0 means 3)
constexpr int kWinMaxHalf = 7;
inline int win_half(int v) { return v ? v : 3; }
inline bool win_default(const ffs_params& p) { return win_half(p.kernel_half_x) == 3 && win_half(p.kernel_half_y) == 3; }

constexpr uint32_t kRadialBinsMax = 1024;   // bins of a radial bin map (kernels_radial.hpp's kRadialMaxBins: ffs_products.hip holds the two equal)

// ---- the pair rules -------------------------------------------------------------------------------------------------------------------
// Two settings that do not combine: whichever of their two setters is called second is refused, with its own text.  Each rule is one line:
// the condition on the settings AS THE CALL WOULD LEAVE THEM, and the text for either caller (with_bins: the bins of the map follow the
// text).  A setter's refusal is the first rule, in this order, that names it and holds -- the order in which ffs_ctx_set_params checks.
// Every rule needs its caller's setting "on", so the off values (gain 0, map NULL, scope centre, flavour 0) are never refused by one.
enum class Setter : int { kParams, kGain, kGainMap, kMaxValidScope, kRadialBins };
struct PairRule {
    bool (*holds)(const ContextSettings&);
    Setter first, second;
    const char *first_text, *second_text;
    bool with_bins;
};
inline bool radial_profile(const ContextSettings& s) { return s.params.algorithm == FFS_ALGO_RADIAL_PROFILE; }
inline bool flavour_1(const ContextSettings& s) { return s.params.extended_flavour == 1; }
inline const PairRule kPairRules[6] = {
    {[](const ContextSettings& s) { return radial_profile(s) && s.radial_bins == 0; }, Setter::kParams, Setter::kRadialBins,
     "ffs_ctx_set_params: the radial_profile algorithm needs a radial bin map (ffs_ctx_set_radial_bins) and the context has none",
     "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which needs the map: set another algorithm first", false},
    {[](const ContextSettings& s) { return radial_profile(s) && s.radial_bins > kRadThrMaxBins; }, Setter::kParams, Setter::kRadialBins,
     "ffs_ctx_set_params: the radial_profile algorithm takes a radial bin map of at most 128 bins and the context's has ",
     "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which takes at most 128 bins, got ", true},
    {[](const ContextSettings& s) { return flavour_1(s) && s.max_valid_scope == FFS_MAX_VALID_WINDOW; }, Setter::kParams, Setter::kMaxValidScope,
     "ffs_ctx_set_params: extended_flavour 1 cannot be combined with the window scope of max_valid (ffs_ctx_set_max_valid_scope): "
     "the device-flavour erosion skips masked neighbours by the static mask",
     "ffs_ctx_set_max_valid_scope: the window scope cannot be combined with extended_flavour 1: the device-flavour erosion "
     "skips masked neighbours by the static mask", false},
    {[](const ContextSettings& s) { return flavour_1(s) && s.gain > 0.0; }, Setter::kParams, Setter::kGain,
     "ffs_ctx_set_params: extended_flavour 1 cannot be combined with a detector gain (ffs_ctx_set_gain): "
     "the reference's device kernels, which that flavour copies, have no gain",
     "ffs_ctx_set_gain: a detector gain cannot be combined with extended_flavour 1: the reference's device kernels, "
     "which that flavour copies, have no gain", false},
    {[](const ContextSettings& s) { return s.gain > 0.0 && s.gain_map; }, Setter::kGain, Setter::kGainMap,
     "ffs_ctx_set_gain: a gain map is set (ffs_ctx_set_gain_map): drop it with ffs_ctx_set_gain_map(ctx, NULL) first",
     "ffs_ctx_set_gain_map: a scalar gain is set (ffs_ctx_set_gain): switch it off with ffs_ctx_set_gain(ctx, 0) first", false},
    {[](const ContextSettings& s) { return flavour_1(s) && s.gain_map; }, Setter::kParams, Setter::kGainMap,
     "ffs_ctx_set_params: extended_flavour 1 cannot be combined with a gain map (ffs_ctx_set_gain_map): "
     "the reference's device kernels, which that flavour copies, have no gain",
     "ffs_ctx_set_gain_map: a gain map cannot be combined with extended_flavour 1: the reference's device kernels, "
     "which that flavour copies, have no gain", false},
};
static_assert(kRadThrMaxBins == 128, "the texts of the second pair rule say 128");
// the refusal of `caller`, whose call would leave the settings as `after`; empty: no pair rule stands against it
inline std::string pair_refusal(Setter caller, const ContextSettings& after) {
    for (const PairRule& r : kPairRules)
        if ((caller == r.first || caller == r.second) && r.holds(after))
            return std::string(caller == r.first ? r.first_text : r.second_text) + (r.with_bins ? std::to_string(after.radial_bins) : std::string());
    return {};
}

// ---- the setters' rules: the refusal's text for the value asked for, or empty for accepted ----------------------------------------------
// Each checks the value's own range first, then the pair rules on the settings with the value in place; nothing is stored here.
inline std::string set_params(const ContextSettings& s, const ffs_params& p) {
    if (p.kernel_half_x < 0 || p.kernel_half_x > kWinMaxHalf || p.kernel_half_y < 0 || p.kernel_half_y > kWinMaxHalf)
        return "ffs_ctx_set_params: kernel_half_x / kernel_half_y must be in 1..7 (0 = 3)";
    const int win_px = (2 * win_half(p.kernel_half_x) + 1) * (2 * win_half(p.kernel_half_y) + 1);
    if (p.min_count < 2 || p.min_count > win_px || p.nsig_b < 0 || p.nsig_s < 0 || p.threshold < 0)   // the asserts of standalone.cc:52-63
        return "ffs_ctx_set_params: need 2 <= min_count <= (2*kernel_half_x+1)*(2*kernel_half_y+1) (49 for the 7x7 window), "
               "nsig_b >= 0, nsig_s >= 0, threshold >= 0";
    if (p.algorithm == FFS_ALGO_DISPERSION_EXTENDED && !win_default(p))
        return "ffs_ctx_set_params: the extended dispersion algorithm needs the 7x7 window (kernel_half_x = kernel_half_y = 3): "
               "its erosion and final pass derive from it";
    if ((p.algorithm != FFS_ALGO_DISPERSION && p.algorithm != FFS_ALGO_DISPERSION_EXTENDED && p.algorithm != FFS_ALGO_RADIAL_PROFILE)
        || (p.extended_flavour != 0 && p.extended_flavour != 1))
        return "ffs_ctx_set_params: unknown algorithm / extended_flavour";
    ContextSettings after = s;
    after.params = p;
    return pair_refusal(Setter::kParams, after);
}
inline std::string set_gain(const ContextSettings& s, double gain) {
    if (!std::isfinite(gain) || gain < 0.0) return "ffs_ctx_set_gain: the gain must be finite and >= 0 (0 = off: pixel values are photon counts)";
    ContextSettings after = s;
    after.gain = gain;
    return pair_refusal(Setter::kGain, after);
}
inline std::string set_gain_map(const ContextSettings& s, bool on) {   // (the entries' ranges: the setter, over the map)
    ContextSettings after = s;
    after.gain_map = on;
    return pair_refusal(Setter::kGainMap, after);
}
inline std::string set_max_valid_scope(const ContextSettings& s, int scope) {
    if (scope != FFS_MAX_VALID_CENTRE && scope != FFS_MAX_VALID_WINDOW)
        return "ffs_ctx_set_max_valid_scope: scope must be FFS_MAX_VALID_CENTRE (0) or FFS_MAX_VALID_WINDOW (1)";
    ContextSettings after = s;
    after.max_valid_scope = scope;
    return pair_refusal(Setter::kMaxValidScope, after);
}
// on: a map of n_bins bins; off (ffs_ctx_set_radial_bins(ctx, NULL, ..)): no map, n_bins plays no part
inline std::string set_radial_bins(const ContextSettings& s, bool on, uint32_t n_bins) {
    if (on && (n_bins < 1 || n_bins > kRadialBinsMax))
        return "ffs_ctx_set_radial_bins: n_bins must be in 1.." + std::to_string(kRadialBinsMax) + ", got " + std::to_string(n_bins);
    ContextSettings after = s;
    after.radial_bins = on ? n_bins : 0u;
    return pair_refusal(Setter::kRadialBins, after);
}
inline std::string set_radial_threshold(const ContextSettings&, double n_iqr) {
    if (!std::isfinite(n_iqr) || n_iqr < 0.0 || n_iqr > kRadThrMaxNIqr)
        return "ffs_ctx_set_radial_threshold: n_iqr must be finite and in 0 .. 2^20 (the cutoff median + n_iqr * iqr is a uint32)";
    return {};
}
inline std::string set_radial_blur(const ContextSettings&, int blur) {
    if (blur != FFS_RADIAL_BLUR_NONE && blur != FFS_RADIAL_BLUR_NARROW && blur != FFS_RADIAL_BLUR_WIDE)
        return "ffs_ctx_set_radial_blur: blur must be FFS_RADIAL_BLUR_NONE (0), _NARROW (1) or _WIDE (2), got " + std::to_string(blur);
    return {};
}
inline std::string set_jungfrau_calibration(const ContextSettings& s, bool on) {   // (the planes' ranges: jungfrau_model.hpp, over the planes)
    if (on && s.pixel_bytes != 4)
        return "ffs_ctx_set_jungfrau_calibration: raw Jungfrau words convert to 32-bit photon counts: the context must have pixel_bytes 4";
    return {};
}

// "entry 87 (x = 7, y = 5) is 0.000000": how the gain map, the bin map and the calibration name the entry they refuse (row length W)
template <typename V>
inline std::string entry_text(size_t i, size_t W, V value) {
    return "entry " + std::to_string(i) + " (x = " + std::to_string(i % W) + ", y = " + std::to_string(i / W) + ") is " + std::to_string(value);
}

}  // namespace ffsamd
