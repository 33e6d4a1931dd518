// threshold_route.hpp -- which threshold stage and which form of the predicate a batch takes, decided once per batch from its settings,
// the tuning and what a re-run overrides; and which instantiation of a kernel family serves a predicate for a pixel size.  No HIP header:
// host code, the kernels (through ffs_device.h) and a plain C++ test program (tests/threshold_route_check.cc) compile the same text.
// DESIGN.md section 3.3e has the rules as a table.
#pragma once
#include <stddef.h>

#include "ffs_hip.h"
#include "tuning.hpp"

namespace ffsamd {

// ---- the predicate's variants and the kernels' instantiations --------------------------------------------------------
enum class Predicate : int {
    kPhotonCount = 0,   // the oracle's predicate: variance = mean; max_valid tests the centre pixel alone
    kWindowScope = 1,   // ... and a pixel p >= ThresholdArgs.nb_limit leaves every window (ffs_ctx_set_max_valid_scope)
    kGain = 2,          // variance = gain * mean (ffs_ctx_set_gain, section 3.3d); carries the neighbour limit too (2^24 under the centre scope)
    kGainMap = 3,       // kGain with the gain of the CENTRE pixel read from a float32 map (ffs_ctx_set_gain_map, section 3.3f); the limit as kGain
};
// The kernels templated on it: k_exact and k_exact_w, k_ext_final, k_ext_erode_final, k_window, k_ext_first
enum class KernelFamily : int { kExact, kExtFinal, kExtFused, kWindow, kExtFirst };

// The one rule.  k_window and k_ext_first compare 32-bit pixels with the neighbour limit in EVERY instantiation (the oracle's 2^24 is that
// argument), so for them the window scope is the photon-count instantiation; everywhere else an instantiation carries the compare iff
// its variant is not photon-count.  (The two compile-time questions a kernel asks of its variant: compares_limit, gain_form.)
constexpr bool limit_is_argument(KernelFamily f, size_t pixel_bytes) {
    return pixel_bytes == 4 && (f == KernelFamily::kWindow || f == KernelFamily::kExtFirst);
}
constexpr Predicate instantiated_as(KernelFamily f, size_t pixel_bytes, Predicate v) {
    return limit_is_argument(f, pixel_bytes) && v == Predicate::kWindowScope ? Predicate::kPhotonCount : v;
}
constexpr bool compares_limit(KernelFamily f, size_t pixel_bytes, Predicate v) {
    return v != Predicate::kPhotonCount && !limit_is_argument(f, pixel_bytes);
}
constexpr bool gain_form(Predicate v) { return v == Predicate::kGain || v == Predicate::kGainMap; }
constexpr bool gain_from_map(Predicate v) { return v == Predicate::kGainMap; }   // g is ThresholdArgs.gain_map at the centre, not ThresholdArgs.gain

// ---- a batch's route through the threshold stage -------------------------------------------------------------------
enum class ThresholdStage : int {
    kCrossCheck,    // dispersion, threshold path 2: the plane starts as the valid-pixel mask, k_exact (3,3) or k_exact_w gathers every pixel
    kWindow,        // dispersion: the general-window kernel decides every pixel
    kStreamList,    // dispersion, path 0: a streaming kernel, its bright windows on the list k_bright_fix works off
    kStreamExact,   // dispersion, path 1: a streaming kernel, its bright windows marked in the plane k_exact filters
    kExtended,      // first pass -> erosion -> final pass
    kRadial,        // the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE): histogram -> cutoffs -> strong pixels (kernels_radthr.hpp)
};
struct ThresholdRoute {
    ThresholdStage stage = ThresholdStage::kStreamList;
    Predicate variant = Predicate::kPhotonCount;
    bool window_scope = false;   // the window scope of max_valid is on: what nb_limit follows, in a gain batch too
    bool window_3x3 = true;
    int bright_to_plane = 0, ext_variant = 0;   // the arguments of these names (ThresholdArgs)
    bool ext_fused = false;      // extended: erosion and final pass are one launch
    bool ext() const { return stage == ThresholdStage::kExtended; }
    bool ext_streams_first() const { return ext_variant >= 2; }   // extended: the streaming kernel is the first pass; else k_ext_first
    // threshold path 2 at a window other than 3,3 has no dense kernel ahead of its gather (nothing for ffs_bench_threshold to time)
    bool has_dense_kernel() const { return stage != ThresholdStage::kCrossCheck || window_3x3; }
};

// rerun_threshold_path: Rerun::threshold_path (< 0: none); the tuning's threshold_path, window_kernel, ext_first_pass and ext_fused are read
// gain_map: a per-pixel gain map is set (exclusive with gain > 0: ffs_ctx_set_gain_map)
inline ThresholdRoute threshold_route(int algorithm, int pixel_bytes, bool window_3x3, int scope, long long max_valid, double gain,
                                      int rerun_threshold_path, const Tuning& t, bool gain_map = false) {
    ThresholdRoute r;
    r.window_scope = scope == FFS_MAX_VALID_WINDOW && max_valid >= 0;   // (without a max_valid the scope changes nothing)
    r.variant = gain_map ? Predicate::kGainMap : gain > 0.0 ? Predicate::kGain : r.window_scope ? Predicate::kWindowScope : Predicate::kPhotonCount;
    r.window_3x3 = window_3x3;
    const bool photon = r.variant == Predicate::kPhotonCount;
    // bright windows: onto the list, or -- tuning "threshold_path" = 1, and whenever that list overflowed -- into the plane as candidates
    r.bright_to_plane = rerun_threshold_path >= 0 ? rerun_threshold_path : t.threshold_path;
    // (the streaming kernels' screens rest on the mask tables, which know nothing of a frame's pixels, and are proven for the photon-count
    // predicate: every other variant takes k_window / k_ext_first -- DESIGN.md sections 3.3c, 3.3d)
    r.ext_variant = (pixel_bytes == 2 && rerun_threshold_path < 0 && photon) ? t.ext_first_pass : 0;
    if (algorithm == FFS_ALGO_RADIAL_PROFILE) {
        // whatever the tuning's threshold_path and window_kernel say: the stage has one form, no bright windows and no first pass
        r.stage = ThresholdStage::kRadial;
        r.bright_to_plane = 0;
        r.ext_variant = 0;
    } else if (algorithm == FFS_ALGO_DISPERSION_EXTENDED) {
        r.stage = ThresholdStage::kExtended;
        r.ext_fused = pixel_bytes == 2 && t.ext_fused != 0 && !gain_form(r.variant);   // (a gain batch has no fused kernel)
    } else if (r.bright_to_plane == 2) {
        r.stage = ThresholdStage::kCrossCheck;
    } else if (!window_3x3 || t.window_kernel == 1 || !photon) {
        r.stage = ThresholdStage::kWindow;
    } else {
        r.stage = r.bright_to_plane ? ThresholdStage::kStreamExact : ThresholdStage::kStreamList;
    }
    return r;
}

}  // namespace ffsamd
