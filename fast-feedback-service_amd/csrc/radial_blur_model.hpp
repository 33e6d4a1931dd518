// radial_blur_model.hpp -- the blur of the radial-profile threshold (ffs_ctx_set_radial_blur) as plain integer
// arithmetic: the weights, the tap rule and v = floor(S / Wn).  No HIP header: the kernels (kernels_radthr.hpp, k_radthr_hist_blur and
// k_radthr_strong_blur) and a plain C++ test program (tests/radial_blur_check.cc) compile the same text.  The reference has no counterpart;
// the narrow kernel is DIALS's, the wide one the binomial of variance 1 in place of DIALS's table of rounded Gaussian values.
//
// The weights are separable, w(dx, dy) = w1(dx) * w1(dy) with w1 = (1, 2, 1) (radius 1, full weight 16) or (1, 4, 6, 4, 1) (radius 2, full
// weight 256).  A pixel is a TAP when it lies inside the image, the valid-pixel mask has its bit and p < limit (launch_geometry.hpp,
// counting_limit: max_valid under both scopes, and p < 2^24 for 32-bit pixels).  S = sum of w * p and Wn = sum of w over the kernel's taps;
// S <= 256 * (2^24 - 1) < 2^32.  Where every tap is present Wn is the full weight, a power of two, and the division is a shift; the
// kernels keep the general division under a branch, and radblur_value is that branch: the check program holds it to `/`.
#pragma once
#include <stdint.h>

#include "spot_background_model.hpp"

namespace ffsamd {

// FFS_RADIAL_BLUR_* of ffs_hip.h; the value is also the kernel's radius
constexpr int kRadBlurNone = 0, kRadBlurNarrow = 1, kRadBlurWide = 2;

// w1(d), d = -R .. R
FFS_SPOTBG_HD constexpr uint32_t radblur_w1(int R, int d) {
    const int a = d < 0 ? -d : d;
    return R == 1 ? (a == 0 ? 2u : 1u) : (a == 0 ? 6u : a == 1 ? 4u : 1u);
}
FFS_SPOTBG_HD constexpr int radblur_shift(int R) { return R == 1 ? 4 : 8; }
FFS_SPOTBG_HD constexpr uint32_t radblur_full(int R) { return 1u << radblur_shift(R); }

FFS_SPOTBG_HD inline bool radblur_tap(uint32_t mask_bit, uint32_t p, uint32_t limit) { return mask_bit != 0u && p < limit; }

// v = floor(S / Wn), Wn >= 1: the shift where no tap is missing, the division elsewhere
FFS_SPOTBG_HD inline uint32_t radblur_value(int R, uint32_t S, uint32_t Wn) { return Wn == radblur_full(R) ? S >> radblur_shift(R) : S / Wn; }

// The weight of one row of the kernel whose present taps are the set bits of `bits` (bit i: the tap at dx = i - R)
FFS_SPOTBG_HD inline uint32_t radblur_row_weight(int R, uint32_t bits) {
    uint32_t w = 0u;
    for (int i = 0; i <= 2 * R; ++i) w += ((bits >> i) & 1u) * radblur_w1(R, i - R);
    return w;
}

// The definition over a whole frame, pixel by pixel and tap by tap (the CPU check program's side): v of every tap pixel, 0 elsewhere.
// px: H rows of W pixels; taps: one byte a pixel, non-zero where the mask has the pixel (the value rule is applied here).
inline void radblur_frame(int R, const uint32_t* px, const uint8_t* mask, int W, int H, uint32_t limit, uint32_t* v_out) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint32_t v = 0u;
            if (radblur_tap(mask[(size_t)y * W + x], px[(size_t)y * W + x], limit)) {
                uint64_t S = 0;
                uint32_t Wn = 0u;
                for (int dy = -R; dy <= R; ++dy)
                    for (int dx = -R; dx <= R; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                        const uint32_t p = px[(size_t)yy * W + xx];
                        if (!radblur_tap(mask[(size_t)yy * W + xx], p, limit)) continue;
                        const uint32_t w = radblur_w1(R, dx) * radblur_w1(R, dy);
                        S += (uint64_t)w * p;
                        Wn += w;
                    }
                v = radblur_value(R, (uint32_t)S, Wn);   // (S < 2^32 whenever limit <= 2^24)
            }
            v_out[(size_t)y * W + x] = v;
        }
}

}  // namespace ffsamd
