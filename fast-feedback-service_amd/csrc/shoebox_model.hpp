// shoebox_model.hpp -- the rule of summation integration in Kabsch space (ffs_ctx_shoebox_begin / ffs_stream_shoebox_fold /
// ffs_ctx_get_shoebox_sums): which pixels of a predicted reflection's shoebox are foreground on which image, what a
// pixel adds to its reflection, and how the accumulated integers become an intensity and a variance.  No HIP header: the kernel
// (kernels_shoebox.hpp), the library's host side, tools/ffs_hosttool.cc and a plain C++ test program (tests/shoebox_check.cc) compile the
// same text, all with -ffp-contract=off.
//
// It restates the reference's integrator (integrator/kabsch.cu: pixel to Kabsch coordinates, the ellipsoid test, the per-pixel
// accumulation; integrator/integrator.cc: the final sums) for a FLAT PANEL WITHOUT PARALLAX CORRECTION.  A panel with parallax correction is
// out of scope: its corner positions would have to be corrected in mm before the step to the laboratory frame.  The reference's scalar_t may
// be float; nothing here is, and no parity with its binaries is claimed: THIS TEXT IS THE CONTRACT.  Every operation is an IEEE float64
// + - * / sqrt, each rounded on its own, in the order written.
//
//   dot(a, b)   = (a0*b0 + a1*b1) + a2*b2
//   cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
//   normalized(v) = v_i / sqrt(dot(v, v))
//   Corner (cx, cy), integers that may lie outside the image:
//       x = (double)cx * px[0], y = (double)cy * px[1], L_i = (D[3i]*x + D[3i+1]*y) + D[3i+2], n = sqrt((L0*L0 + L1*L1) + L2*L2),
//       s_i = (L_i / n) / wavelength
//   Per reflection: e1 = normalized(cross(s1, s0)), e2 = normalized(cross(s1, e1)), len = sqrt(dot(s1, s1)), zeta = dot(rot_axis, e1)
//   Per corner:     d = s - s1, eps1 = dot(e1, d) / len, eps2 = dot(e2, d) / len, xy = (eps1*eps1 + eps2*eps2) * ib
//   Image n (0-based position in the scan): phi_low = (osc_start + (double)n * osc_width) * (M_PI / 180.0), phi_high the same with n + 1,
//       centre = phi_c >= phi_low && phi_c <= phi_high
//   ib = 1.0 / (delta_b * delta_b), im = 1.0 / (delta_m * delta_m)
//   kShoeboxEllipsoid: a corner is foreground when xy + (e3*e3) * im <= 1.0 holds for e3 = zeta * (phi_low - phi_c), for
//       e3 = zeta * (phi_high - phi_c), or -- when centre holds -- for e3 = 0.
//   kShoeboxDials:     xy <= 1.0 (the image plays no part).
//   A pixel (px, py) is foreground when any of its four corners {px, px+1} x {py, py+1} is.
// A corner's xy does not depend on the image, and an image's three e3 terms do not depend on the corner: the kernel computes each once.
//
// What a pixel does to its reflection.  A pixel COUNTS when it lies in the image, its mask bit is set and p < limit (counting_limit of
// launch_geometry.hpp: max_valid inclusive when set, and p < 2^24).
//   foreground and counting:      fg_sum += p, fg_count += 1, m_x += p * (2 px + 1), m_y += p * (2 py + 1), m_z += p * (2 n + 1)
//   foreground and not counting:  flags |= kShoeboxFgInvalid
//   background and counting:      hist[p] += 1 for p < 256, else n_overflow += 1
//   background and not counting:  nothing
// Everything accumulated is an integer: the result does not depend on batch size, stream, order or tuning.
#pragma once
#include <math.h>
#include <stdint.h>

#include "spot_background_glm_model.hpp"
#include "spot_background_model.hpp"

namespace ffsamd {

constexpr int kShoeboxEllipsoid = 0, kShoeboxDials = 1;   // FFS_SHOEBOX_ELLIPSOID, FFS_SHOEBOX_DIALS
constexpr uint32_t kShoeboxFgInvalid = 1u;                // FFS_SHOEBOX_FG_INVALID
constexpr int kShoeboxBgTukey = 0, kShoeboxBgGlm = 1;     // background_model of ffs_ctx_get_shoebox_sums
constexpr double kShoeboxDegToRad = M_PI / 180.0;

struct ShoeboxGeometry {   // = ffs_scan_geometry
    double d_matrix[9], pixel_size_mm[2], wavelength, s0[3], rot_axis[3], osc_start_deg, osc_width_deg;
};
struct ShoeboxEntry {      // = ffs_shoebox, 56 bytes
    double s1[3], phi;
    int32_t x_min, x_max, y_min, y_max, z_min, z_max;   // half-open
};
// The integers a reflection accumulates, without its histogram: the device's record, 48 bytes
struct ShoeboxAcc {
    uint64_t fg_sum, m_x, m_y, m_z;
    uint32_t fg_count, n_overflow, flags, reserved;
};
struct ShoeboxSum {        // = ffs_shoebox_sum, 80 bytes
    uint64_t fg_sum, m_x, m_y, m_z;
    uint32_t fg_count, n_background, n_overflow, flags, bg_status, reserved;
    double bg_mean, intensity, variance;
};

FFS_SPOTBG_HD inline double shoebox_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
FFS_SPOTBG_HD inline void shoebox_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
FFS_SPOTBG_HD inline void shoebox_normalize(double* v) {
    const double n = sqrt(shoebox_dot(v, v));
    v[0] = v[0] / n, v[1] = v[1] / n, v[2] = v[2] / n;
}

// What is computed once per reflection
struct ShoeboxFrame {
    double e1[3], e2[3], s1[3], len, zeta, phi_c;
};
FFS_SPOTBG_HD inline ShoeboxFrame shoebox_frame(const ShoeboxGeometry& g, const double* s1, double phi) {
    ShoeboxFrame f;
    f.s1[0] = s1[0], f.s1[1] = s1[1], f.s1[2] = s1[2];
    shoebox_cross(s1, g.s0, f.e1);
    shoebox_normalize(f.e1);
    shoebox_cross(s1, f.e1, f.e2);
    shoebox_normalize(f.e2);
    f.len = sqrt(shoebox_dot(s1, s1));
    f.zeta = shoebox_dot(g.rot_axis, f.e1);
    f.phi_c = phi;
    return f;
}

FFS_SPOTBG_HD inline void shoebox_corner_s(const ShoeboxGeometry& g, int32_t cx, int32_t cy, double* s) {
    const double x = (double)cx * g.pixel_size_mm[0], y = (double)cy * g.pixel_size_mm[1];
    const double* D = g.d_matrix;
    const double l0 = (D[0] * x + D[1] * y) + D[2], l1 = (D[3] * x + D[4] * y) + D[5], l2 = (D[6] * x + D[7] * y) + D[8];
    const double n = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
    s[0] = (l0 / n) / g.wavelength, s[1] = (l1 / n) / g.wavelength, s[2] = (l2 / n) / g.wavelength;
}
// xy of a corner: (eps1*eps1 + eps2*eps2) * ib
FFS_SPOTBG_HD inline double shoebox_corner_xy(const ShoeboxGeometry& g, const ShoeboxFrame& f, int32_t cx, int32_t cy, double ib) {
    double s[3];
    shoebox_corner_s(g, cx, cy, s);
    const double d[3] = {s[0] - f.s1[0], s[1] - f.s1[1], s[2] - f.s1[2]};
    const double eps1 = shoebox_dot(f.e1, d) / f.len, eps2 = shoebox_dot(f.e2, d) / f.len;
    return (eps1 * eps1 + eps2 * eps2) * ib;
}

FFS_SPOTBG_HD inline double shoebox_inverse_square(double delta) { return 1.0 / (delta * delta); }

// What is computed once per (reflection, image): the (e3*e3) * im terms of the image's two edges and whether phi_c lies in it
struct ShoeboxImage {
    double z_low, z_high, z_centre;
    bool centre;
};
FFS_SPOTBG_HD inline ShoeboxImage shoebox_image(const ShoeboxGeometry& g, const ShoeboxFrame& f, int64_t n, double im) {
    const double phi_low = (g.osc_start_deg + (double)n * g.osc_width_deg) * kShoeboxDegToRad;
    const double phi_high = (g.osc_start_deg + (double)(n + 1) * g.osc_width_deg) * kShoeboxDegToRad;
    const double e_low = f.zeta * (phi_low - f.phi_c), e_high = f.zeta * (phi_high - f.phi_c);
    ShoeboxImage i;
    i.z_low = (e_low * e_low) * im;
    i.z_high = (e_high * e_high) * im;
    i.z_centre = (0.0 * 0.0) * im;
    i.centre = f.phi_c >= phi_low && f.phi_c <= phi_high;
    return i;
}
// The foreground decision of a corner on an image (z_centre is the e3 = 0 term as written, (0*0) * im: 0 for every finite im)
FFS_SPOTBG_HD inline bool shoebox_corner_foreground(int algorithm, double xy, const ShoeboxImage& i) {
    if (algorithm == kShoeboxDials) return xy <= 1.0;
    return xy + i.z_low <= 1.0 || xy + i.z_high <= 1.0 || (i.centre && xy + i.z_centre <= 1.0);
}

// ---- the end of the sweep: accumulators and histogram to a record (integrator.cc's final loop) ---------------------------------------
// The background is the box's histogram under one of the two existing models, unchanged, with its status codes; b = mean when the status is
// 0, else 0; B = b * fg_count, I = fg_sum - B, var = |I| + |B| * (1 + fg_count / n_bg) (the ratio is 0 without background pixels), and
// I = 0, var = -1 for a reflection without foreground.
inline ShoeboxSum shoebox_sum(const ShoeboxAcc& a, const uint32_t* hist, int background_model) {
    ShoeboxSum o{};
    o.fg_sum = a.fg_sum, o.m_x = a.m_x, o.m_y = a.m_y, o.m_z = a.m_z;
    o.fg_count = a.fg_count, o.n_overflow = a.n_overflow, o.flags = a.flags;
    if (background_model == kShoeboxBgGlm) {
        const SpotBgGlmResult r = spotbg_glm_from_histogram(hist, a.n_overflow);
        o.n_background = r.n_pixels, o.bg_status = r.status, o.bg_mean = r.status == kSpotBgOk ? r.mean : 0.0;
    } else {
        const SpotBgResult r = spotbg_from_histogram(hist, a.n_overflow);
        o.n_background = r.n_pixels, o.bg_status = r.status;
        o.bg_mean = (r.status == kSpotBgOk && r.n_inliers) ? (double)r.inlier_sum / (double)r.n_inliers : 0.0;
    }
    if (a.fg_count == 0) {
        o.intensity = 0.0, o.variance = -1.0;
        return o;
    }
    const double B = o.bg_mean * (double)a.fg_count;
    const double I = (double)a.fg_sum - B;
    const double ratio = o.n_background > 0 ? (double)a.fg_count / (double)o.n_background : 0.0;
    o.intensity = I;
    o.variance = fabs(I) + fabs(B) * (1.0 + ratio);
    return o;
}

// ---- the whole rule over one image on the CPU (tools/ffs_hosttool.cc, tests/shoebox_check.cc): pixel by pixel, corner by corner ------
// frame: H rows of pitch_px pixels; mask: W*H bytes (non-zero = valid) or null; limit: counting_limit; n: the image's position in the scan.
// fg_map (may be null): (x_max - x_min) * (y_max - y_min) bytes, the foreground decision of every pixel of the box on this image.
template <typename PixelT>
inline void shoebox_fold_image(const ShoeboxGeometry& g, const ShoeboxEntry& b, int algorithm, double delta_b, double delta_m, const PixelT* frame,
                               size_t pitch_px, int W, int H, const uint8_t* mask, uint32_t limit, int64_t n, ShoeboxAcc& acc, uint32_t* hist,
                               uint8_t* fg_map = nullptr) {
    if (n < b.z_min || n >= b.z_max) return;
    const double ib = shoebox_inverse_square(delta_b), im = shoebox_inverse_square(delta_m);
    const ShoeboxFrame f = shoebox_frame(g, b.s1, b.phi);
    const ShoeboxImage img = shoebox_image(g, f, n, im);
    auto corner = [&](int32_t cx, int32_t cy) { return shoebox_corner_foreground(algorithm, shoebox_corner_xy(g, f, cx, cy, ib), img); };
    for (int32_t py = b.y_min; py < b.y_max; ++py)
        for (int32_t px = b.x_min; px < b.x_max; ++px) {
            const bool fg = corner(px, py) || corner(px + 1, py) || corner(px, py + 1) || corner(px + 1, py + 1);
            if (fg_map) fg_map[(size_t)(py - b.y_min) * (size_t)(b.x_max - b.x_min) + (size_t)(px - b.x_min)] = fg;
            bool counts = px >= 0 && px < W && py >= 0 && py < H;
            uint64_t p = 0;
            if (counts) {
                p = frame[(size_t)py * pitch_px + (size_t)px];
                counts = (!mask || mask[(size_t)py * (size_t)W + (size_t)px]) && p < limit;
            }
            if (fg && counts) {
                acc.fg_sum += p, acc.fg_count += 1;
                acc.m_x += p * (uint64_t)(2 * px + 1), acc.m_y += p * (uint64_t)(2 * py + 1), acc.m_z += p * (uint64_t)(2 * n + 1);
            } else if (fg) {
                acc.flags |= kShoeboxFgInvalid;
            } else if (counts) {
                if (p < (uint64_t)kSpotBgBins) hist[p] += 1;
                else acc.n_overflow += 1;
            }
        }
}

}  // namespace ffsamd
