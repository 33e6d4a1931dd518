// predict_model.hpp -- the rule of scan prediction for a rotation sweep (ffs_ctx_predict): which Miller indices
// cross the Ewald sphere on which image, where the diffracted ray meets the panel, and the bounding box of the reflection's shoebox in
// Kabsch space.  No HIP header: the kernels (kernels_predict.hpp), the library's host side, tools/ffs_hosttool.cc and a plain C++ test
// program (tests/predict_check.cc) compile the same text, all with -ffp-contract=off.
//
// It restates the reference's per-image ray predictor (predictor/predict.cc:31-128, predict_ray_monochromatic_sv in
// predictor/ray_predictors.cc:115-201) and its Kabsch bounding boxes (compute_kabsch_bounding_boxes, integrator/extent.cc:14-198) for ONE
// FLAT PANEL, ONE s0 AND ONE CRYSTAL SETTING OVER THE SCAN.  No parity with the reference's binaries is claimed: THIS TEXT IS THE CONTRACT.
// Every operation is an IEEE float64 + - * / sqrt floor ceil, a comparison or an integer-to-double conversion, each rounded on its own, in
// the order written.  No trigonometric function is evaluated here: the rotation's cosine and sine are arguments.
//
//   dot(a, b) = (a0*b0 + a1*b1) + a2*b2,  cross and normalized as in shoebox_model.hpp
//   inverse(M): c00 = M4*M8 - M5*M7, c01 = M5*M6 - M3*M8, c02 = M3*M7 - M4*M6, det = (M0*c00 + M1*c01) + M2*c02,
//       inv = [c00, M2*M7 - M1*M8, M1*M5 - M2*M4;  c01, M0*M8 - M2*M6, M2*M3 - M0*M5;  c02, M1*M6 - M0*M7, M0*M4 - M1*M3] each / det
//   Scan point k = 0 .. n_images: phi_k = (osc_start + (double)k * osc_width) * (M_PI / 180.0); the HOST evaluates c = cos(phi_k),
//       s = sin(phi_k) with libm; u = normalized(rot_axis), t = 1.0 - c,
//       R = [c + t*(u0*u0), t*(u0*u1) - s*u2, t*(u0*u2) + s*u1;  t*(u0*u1) + s*u2, c + t*(u1*u1), t*(u1*u2) - s*u0;
//            t*(u0*u2) - s*u1, t*(u1*u2) + s*u0, c + t*(u2*u2)]   (Rodrigues),  A_k[i][j] = (R[i][0]*A[0][j] + R[i][1]*A[1][j]) + R[i][2]*A[2][j]
//   Candidates: the rows of inverse(A) are the real-space axes; h_max[i] = (int)floor(sqrt(dot(row_i, row_i)) / dmin) + 1;
//       candidate number q = ((h + h_max[0]) * (2 h_max[1] + 1) + (k + h_max[1])) * (2 h_max[2] + 1) + (l + h_max[2]): h slowest, l fastest.
//       (0, 0, 0) and the indices absent under the centring (integers: I h+k+l odd, F mixed parity, A k+l odd, B h+l odd, C h+k odd,
//       R obverse (-h+k+l) mod 3 != 0) predict nothing.
//   Per candidate and scan point: r_k[i] = (A_k[3i]*(double)h + A_k[3i+1]*(double)k) + A_k[3i+2]*(double)l, rr_k = dot(r_k, r_k),
//       t = s0 + r_k, outside_k = dot(t, t) >= dot(s0, s0).
//       DEPARTURE: the reference compares norm() - norm() with 0; here the squared norms are compared, which saves two square roots and
//       decides the same side except within a rounding of the sphere.
//       A candidate with rr_0 > res_leave = (1 / (dmin*dmin)) * 1.000001 is left at once: the rotation preserves |r| to a few units in
//       the last place, so the per-image resolution test below is true on every image of such a candidate.
//   Image n = 0 .. n_images - 1, r1 = r_n, r2 = r_{n+1} (ray_predictors.cc:126-143): a ray exists only when outside_n != outside_{n+1}
//       and not rr_n > 1.0 / (dmin*dmin).  Then (lines 149-189)
//       dr = r2 - r1, a = dot(dr, dr), b = dot(s0 + r1, dr), c = rr_n + 2.0 * dot(s0, r1), d = b*b - a*c; none when d < 0;
//       q = sqrt(d), roots (-b - q) / a then (-b + q) / a, alpha1 = the first of them with 0 <= root <= 1; none when neither;
//       b = -dot(s0 + r2, dr), c = rr_{n+1} + 2.0 * dot(s0, r2), the same again for alpha2;  alpha = alpha1 / (alpha1 + alpha2);
//       s1[i] = (r1[i] + alpha * dr[i]) + s0[i]   (with one s0 the reference's interpolated s0_at_intersection, lines 192-195, is s0 itself:
//       both unit vectors are equal and the wavenumber is |s0|; it is taken as s0 without the round trip through normalized());
//       angle = (osc_start + (double)n * osc_width) + alpha * osc_width  in degrees, phi = angle * (M_PI / 180.0);  entering = outside_n.
//   Impact (predict.cc:106-116, one panel): v[i] = (Dinv[3i]*s1[0] + Dinv[3i+1]*s1[1]) + Dinv[3i+2]*s1[2] with Dinv = inverse(D);
//       none unless v[2] > 0;  x_px = (v[0] / v[2]) / px[0], y_px = (v[1] / v[2]) / px[1];  kept when 0 <= x_px < W and 0 <= y_px < H;
//       z = (double)n + alpha.
//   Extent (extent.cc:47-192): e1 = normalized(cross(s1, s0)), e2 = normalized(cross(s1, e1)), len = sqrt(dot(s1, s1)); for the signs
//       (+,+), (+,-), (-,+), (-,-): p[i] = ((sa*delta_b) * e1[i]) * len + ((sb*delta_b) * e2[i]) * len, b = len*len - dot(p, p); the corner
//       is LOST when b < 0; d = -(dot(p, s1) / len) + sqrt(b), s'[i] = (d * s1[i]) / len + p[i], through Dinv as above without the panel
//       bound; a corner is also lost when not v[2] > 0 or when its pixel position is not finite (the reference skips a corner without an
//       intersection).  Over the surviving corners x_min = floor(min x), x_max = ceil(max x), likewise y, each clamped to +-2^30 before the
//       conversion to int32.  A lost corner sets kPredictCornerLost.
//       zeta = dot(rot_axis, e1).  When zeta > 1e-10 or zeta < -1e-10: phi+- = phi +- delta_m / zeta, z+- = ((phi+- * 180.0 / M_PI) -
//       osc_start) / osc_width (image_range_start = 1, so the reference's image_range_start - 1 is 0), z_min = floor(min) clamped to
//       [0, n_images - 1], z_max = ceil(max) clamped to [1, n_images] (lines 179-186; clamped as doubles, then converted).  Otherwise
//       kPredictZetaSmall and the whole scan.  DEPARTURE: the reference's degenerate branch sets z_min = image_range_start (1 here), which
//       would leave the scan's first image out; [0, n_images) is taken.
//       kPredictBoxRefused marks a record ffs_ctx_shoebox_begin would refuse: no corner survived (the box is then all zero), a side that
//       is empty or longer than 1024 pixels, or a box that does not meet the image padded by 1024 pixels.
#pragma once
#include <math.h>
#include <stdint.h>

#include "shoebox_model.hpp"

namespace ffsamd {

constexpr int kPredictCentrings = 7;   // FFS_CENTRING_P I F A B C R = 0 .. 6
constexpr uint32_t kPredictEntering = 1u, kPredictCornerLost = 2u, kPredictZetaSmall = 4u, kPredictBoxRefused = 8u;   // FFS_PREDICT_*
constexpr double kPredictZetaTolerance = 1e-10;
constexpr double kPredictLeaveMargin = 1.000001;
constexpr int32_t kPredictMaxSide = 1024, kPredictPad = 1024;   // = kShoeboxMaxSide, kShoeboxPad of shoebox_plan.hpp (predict_plan.hpp asserts it)
constexpr double kPredictIntClamp = 1073741824.0;               // 2^30

struct PredictCrystal {   // = ffs_crystal, 80 bytes
    double a_matrix[9];
    int32_t centring, reserved;
};
struct PredictRecord {    // = ffs_prediction, 96 bytes
    ShoeboxEntry box;
    double x_px, y_px, z;
    int32_t h, k, l;
    uint32_t flags;
};
// What the host computes once per call (predict_plan.hpp) and every candidate reads
struct PredictSetup {
    double s0[3], s0s0;
    double res_limit, res_leave;   // 1 / dmin^2 and that times kPredictLeaveMargin
    double d_inv[9], px[2], rot_axis[3];
    double osc_start, osc_width, delta_b, delta_m;
    int32_t h_max[3], centring;
    int32_t W, H;
    uint32_t n_images, n_candidates;
};
struct PredictRay {
    double s1[3], phi, alpha, x_px, y_px;
    bool entering;
};

// inverse by cofactors; false when the determinant is zero or the result not finite
FFS_SPOTBG_HD inline bool predict_inverse(const double* m, double* inv) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    inv[0] = c00 / det, inv[1] = (m[2] * m[7] - m[1] * m[8]) / det, inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    inv[3] = c01 / det, inv[4] = (m[0] * m[8] - m[2] * m[6]) / det, inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    inv[6] = c02 / det, inv[7] = (m[1] * m[6] - m[0] * m[7]) / det, inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    bool ok = det != 0.0;
    for (int i = 0; i < 9; ++i) ok = ok && inv[i] - inv[i] == 0.0;
    return ok;
}

// A_k = R A for the rotation by the angle whose cosine and sine are c and s, about the normalized axis u
FFS_SPOTBG_HD inline void predict_scan_setting(const double* u, const double* A, double c, double s, double* out) {
    const double t = 1.0 - c;
    const double R[9] = {c + t * (u[0] * u[0]), t * (u[0] * u[1]) - s * u[2], t * (u[0] * u[2]) + s * u[1],
                         t * (u[0] * u[1]) + s * u[2], c + t * (u[1] * u[1]), t * (u[1] * u[2]) - s * u[0],
                         t * (u[0] * u[2]) - s * u[1], t * (u[1] * u[2]) + s * u[0], c + t * (u[2] * u[2])};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (R[3 * i] * A[j] + R[3 * i + 1] * A[3 + j]) + R[3 * i + 2] * A[6 + j];
}
FFS_SPOTBG_HD inline double predict_scan_point_deg(double osc_start, double osc_width, uint32_t k) { return osc_start + (double)k * osc_width; }

FFS_SPOTBG_HD inline bool predict_absent(int centring, int32_t h, int32_t k, int32_t l) {
    switch (centring) {
        case 1: return ((h + k + l) & 1) != 0;
        case 2: return ((h ^ k) & 1) != 0 || ((k ^ l) & 1) != 0;
        case 3: return ((k + l) & 1) != 0;
        case 4: return ((h + l) & 1) != 0;
        case 5: return ((h + k) & 1) != 0;
        case 6: return (-h + k + l) % 3 != 0;
        default: return false;
    }
}
// candidate number -> index (the number is below the box's size)
FFS_SPOTBG_HD inline void predict_index_of(const int32_t* h_max, uint32_t q, int32_t& h, int32_t& k, int32_t& l) {
    const uint32_t nk = 2u * (uint32_t)h_max[1] + 1u, nl = 2u * (uint32_t)h_max[2] + 1u;
    const uint32_t hk = q / nl;
    l = (int32_t)(q - hk * nl) - h_max[2];
    const uint32_t hh = hk / nk;
    k = (int32_t)(hk - hh * nk) - h_max[1];
    h = (int32_t)hh - h_max[0];
}
FFS_SPOTBG_HD inline int64_t predict_number_of(const int32_t* h_max, int32_t h, int32_t k, int32_t l) {
    return ((int64_t)(h + h_max[0]) * (2 * (int64_t)h_max[1] + 1) + (k + h_max[1])) * (2 * (int64_t)h_max[2] + 1) + (l + h_max[2]);
}

FFS_SPOTBG_HD inline void predict_r(const double* A, double h, double k, double l, double* r) {
    r[0] = (A[0] * h + A[1] * k) + A[2] * l;
    r[1] = (A[3] * h + A[4] * k) + A[5] * l;
    r[2] = (A[6] * h + A[7] * k) + A[8] * l;
}
FFS_SPOTBG_HD inline bool predict_outside(const PredictSetup& u, const double* r) {
    const double t[3] = {u.s0[0] + r[0], u.s0[1] + r[1], u.s0[2] + r[2]};
    return shoebox_dot(t, t) >= u.s0s0;
}
FFS_SPOTBG_HD inline bool predict_root(double a, double b, double d, double& alpha) {
    const double q = sqrt(d);
    const double first = (-b - q) / a, second = (-b + q) / a;
    if (0.0 <= first && first <= 1.0) alpha = first;
    else if (0.0 <= second && second <= 1.0) alpha = second;
    else return false;
    return true;
}
// The ray of image n from the two ends of its step (the caller has found the sides different and rr1 inside the limit)
FFS_SPOTBG_HD inline bool predict_ray(const PredictSetup& u, const double* r1, const double* r2, double rr1, double rr2, uint32_t n, bool starts_outside, PredictRay& ray) {
    const double dr[3] = {r2[0] - r1[0], r2[1] - r1[1], r2[2] - r1[2]};
    const double t1[3] = {u.s0[0] + r1[0], u.s0[1] + r1[1], u.s0[2] + r1[2]};
    const double t2[3] = {u.s0[0] + r2[0], u.s0[1] + r2[1], u.s0[2] + r2[2]};
    const double a = shoebox_dot(dr, dr);
    double b = shoebox_dot(t1, dr);
    double c = rr1 + 2.0 * shoebox_dot(u.s0, r1);
    double d = b * b - a * c;
    if (d < 0.0) return false;
    double alpha1, alpha2;
    if (!predict_root(a, b, d, alpha1)) return false;
    b = -shoebox_dot(t2, dr);
    c = rr2 + 2.0 * shoebox_dot(u.s0, r2);
    d = b * b - a * c;
    if (d < 0.0) return false;
    if (!predict_root(a, b, d, alpha2)) return false;
    const double alpha = alpha1 / (alpha1 + alpha2);
    ray.s1[0] = (r1[0] + alpha * dr[0]) + u.s0[0];
    ray.s1[1] = (r1[1] + alpha * dr[1]) + u.s0[1];
    ray.s1[2] = (r1[2] + alpha * dr[2]) + u.s0[2];
    const double angle = predict_scan_point_deg(u.osc_start, u.osc_width, n) + alpha * u.osc_width;
    ray.phi = angle * kShoeboxDegToRad;
    ray.alpha = alpha;
    ray.entering = starts_outside;
    return true;
}
// s through inverse(D) to pixels; false without an intersection in front of the source
FFS_SPOTBG_HD inline bool predict_to_pixels(const PredictSetup& u, const double* s, double& x_px, double& y_px) {
    const double* M = u.d_inv;
    const double v0 = (M[0] * s[0] + M[1] * s[1]) + M[2] * s[2], v1 = (M[3] * s[0] + M[4] * s[1]) + M[5] * s[2], v2 = (M[6] * s[0] + M[7] * s[1]) + M[8] * s[2];
    if (!(v2 > 0.0)) return false;
    x_px = (v0 / v2) / u.px[0];
    y_px = (v1 / v2) / u.px[1];
    return true;
}
FFS_SPOTBG_HD inline bool predict_impact(const PredictSetup& u, PredictRay& ray) {
    if (!predict_to_pixels(u, ray.s1, ray.x_px, ray.y_px)) return false;
    return 0.0 <= ray.x_px && ray.x_px < (double)u.W && 0.0 <= ray.y_px && ray.y_px < (double)u.H;
}

// The walk of one candidate over the scan points: every A_k h is computed once and carried, with its side of the sphere, into the next
// step; sink(n, ray) is called for every kept ray, in the order of n.  A: (n_images + 1) * 9 doubles.
template <typename Sink>
FFS_SPOTBG_HD inline void predict_walk(const PredictSetup& u, const double* A, int32_t h, int32_t k, int32_t l, Sink&& sink) {
    if ((h == 0 && k == 0 && l == 0) || predict_absent(u.centring, h, k, l)) return;
    const double hd = (double)h, kd = (double)k, ld = (double)l;
    double r1[3], r2[3];
    predict_r(A, hd, kd, ld, r1);
    double rr1 = shoebox_dot(r1, r1);
    if (rr1 > u.res_leave) return;
    bool out1 = predict_outside(u, r1);
    for (uint32_t n = 0; n < u.n_images; ++n) {
        predict_r(A + 9u * (n + 1u), hd, kd, ld, r2);
        const double rr2 = shoebox_dot(r2, r2);
        const bool out2 = predict_outside(u, r2);
        if (out1 != out2 && !(rr1 > u.res_limit)) {
            PredictRay ray;
            if (predict_ray(u, r1, r2, rr1, rr2, n, out1, ray) && predict_impact(u, ray)) sink(n, ray);
        }
        r1[0] = r2[0], r1[1] = r2[1], r1[2] = r2[2];
        rr1 = rr2;
        out1 = out2;
    }
}

FFS_SPOTBG_HD inline int32_t predict_to_int(double v) {
    if (v < -kPredictIntClamp) v = -kPredictIntClamp;
    if (v > kPredictIntClamp) v = kPredictIntClamp;
    return (int32_t)v;
}
// Would ffs_ctx_shoebox_begin refuse the box (the integer part of shoebox_plan.hpp's rule)
FFS_SPOTBG_HD inline bool predict_box_refused(const ShoeboxEntry& b, int W, int H) {
    if (!(b.x_min < b.x_max) || !(b.y_min < b.y_max) || !(b.z_min < b.z_max)) return true;
    if ((int64_t)b.x_max - b.x_min > kPredictMaxSide || (int64_t)b.y_max - b.y_min > kPredictMaxSide) return true;
    return b.x_max <= -kPredictPad || b.x_min >= W + kPredictPad || b.y_max <= -kPredictPad || b.y_min >= H + kPredictPad;
}

// A kept ray to its record: the extent in Kabsch space
FFS_SPOTBG_HD inline PredictRecord predict_record(const PredictSetup& u, int32_t h, int32_t k, int32_t l, uint32_t n, const PredictRay& ray) {
    PredictRecord o;
    o.box.s1[0] = ray.s1[0], o.box.s1[1] = ray.s1[1], o.box.s1[2] = ray.s1[2];
    o.box.phi = ray.phi;
    o.x_px = ray.x_px, o.y_px = ray.y_px, o.z = (double)n + ray.alpha;
    o.h = h, o.k = k, o.l = l;
    uint32_t flags = ray.entering ? kPredictEntering : 0u;
    double e1[3], e2[3];
    shoebox_cross(ray.s1, u.s0, e1);
    shoebox_normalize(e1);
    shoebox_cross(ray.s1, e1, e2);
    shoebox_normalize(e2);
    const double len = sqrt(shoebox_dot(ray.s1, ray.s1));
    double x_lo = 0.0, x_hi = 0.0, y_lo = 0.0, y_hi = 0.0;
    int survived = 0;
    for (int ci = 0; ci < 4; ++ci) {
        const double sa = (ci & 2) ? -1.0 : 1.0, sb = (ci & 1) ? -1.0 : 1.0;
        const double fa = sa * u.delta_b, fb = sb * u.delta_b;
        const double p[3] = {(fa * e1[0]) * len + (fb * e2[0]) * len, (fa * e1[1]) * len + (fb * e2[1]) * len, (fa * e1[2]) * len + (fb * e2[2]) * len};
        const double b = len * len - shoebox_dot(p, p);
        bool lost = b < 0.0;
        double x = 0.0, y = 0.0;
        if (!lost) {
            const double d = -(shoebox_dot(p, ray.s1) / len) + sqrt(b);
            const double sp[3] = {(d * ray.s1[0]) / len + p[0], (d * ray.s1[1]) / len + p[1], (d * ray.s1[2]) / len + p[2]};
            lost = !predict_to_pixels(u, sp, x, y) || !(x - x == 0.0) || !(y - y == 0.0);
        }
        if (lost) {
            flags |= kPredictCornerLost;
            continue;
        }
        if (survived == 0) x_lo = x_hi = x, y_lo = y_hi = y;
        else {
            if (x < x_lo) x_lo = x;
            if (x > x_hi) x_hi = x;
            if (y < y_lo) y_lo = y;
            if (y > y_hi) y_hi = y;
        }
        ++survived;
    }
    o.box.x_min = predict_to_int(floor(x_lo)), o.box.x_max = predict_to_int(ceil(x_hi));
    o.box.y_min = predict_to_int(floor(y_lo)), o.box.y_max = predict_to_int(ceil(y_hi));
    const double zeta = shoebox_dot(u.rot_axis, e1);
    const double n_img = (double)u.n_images;
    if (zeta > kPredictZetaTolerance || zeta < -kPredictZetaTolerance) {
        const double phi_plus = ray.phi + u.delta_m / zeta, phi_minus = ray.phi - u.delta_m / zeta;
        const double z_plus = ((phi_plus * 180.0 / M_PI) - u.osc_start) / u.osc_width, z_minus = ((phi_minus * 180.0 / M_PI) - u.osc_start) / u.osc_width;
        double lo = floor(z_plus < z_minus ? z_plus : z_minus), hi = ceil(z_plus > z_minus ? z_plus : z_minus);
        if (lo < 0.0) lo = 0.0;
        if (lo > n_img - 1.0) lo = n_img - 1.0;
        if (hi < 1.0) hi = 1.0;
        if (hi > n_img) hi = n_img;
        o.box.z_min = (int32_t)lo, o.box.z_max = (int32_t)hi;
    } else {
        flags |= kPredictZetaSmall;
        o.box.z_min = 0, o.box.z_max = (int32_t)u.n_images;
    }
    if (survived == 0 || predict_box_refused(o.box, u.W, u.H)) flags |= kPredictBoxRefused;
    o.flags = flags;
    return o;
}

}  // namespace ffsamd
