// predict_plan_check.cc -- csrc/predict_plan.hpp as a plain C++ program (tests/test_predict_plan.py builds it under the address and
// undefined-behaviour sanitizers).  It holds:
//   every refusal of ffs_ctx_predict that the header decides -- its text, and that the caller's PredictSetup is untouched;
//   what a taken call computes: h_max, the candidate count, 1 / dmin^2, inverse(D);
//   h_max against brute force on 200 random settings: no index inside the resolution sphere lies outside the box;
//   the candidate numbering: round trip, h slowest and l fastest, (0,0,0) in the middle;
//   the centring absences against their definitions;
//   kPredictBoxRefused against shoebox_plan.hpp's own refusal on random boxes;
//   the scan-point settings: orthogonal to rounding, the first one A itself when osc_start is 0.
// Prints FAIL lines and ends with OK or FAILED.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

#include "predict_plan.hpp"

using namespace ffsamd;

static int failures = 0;
#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            ++failures;                         \
            std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);           \
            std::printf("\n");                  \
        }                                       \
    } while (0)

static ShoeboxGeometry geometry() {
    ShoeboxGeometry g{};
    const double D[9] = {1, 0, -70.65, 0, -1, 48.8, 0, 0, -100};
    std::memcpy(g.d_matrix, D, sizeof D);
    g.pixel_size_mm[0] = g.pixel_size_mm[1] = 0.5;
    g.wavelength = 1.0;
    g.s0[2] = -1.0;
    g.rot_axis[0] = 1.0;
    g.osc_start_deg = 0.0, g.osc_width_deg = 0.5;
    return g;
}
static PredictCrystal crystal(double a, double b, double c) {
    PredictCrystal x{};
    x.a_matrix[0] = 1.0 / a, x.a_matrix[4] = 1.0 / b, x.a_matrix[8] = 1.0 / c;
    return x;
}

static void refused(const char* what, const ShoeboxGeometry& g, const PredictCrystal& x, uint32_t n_images, double dmin, double db, double dm, const char* needle) {
    PredictSetup u, before;
    std::memset(&u, 0x5a, sizeof u);
    std::memcpy(&before, &u, sizeof u);
    const std::string why = predict_refusal(g, x, n_images, dmin, db, dm, 300, 200, u);
    CHECK(!why.empty() && why.find(needle) != std::string::npos, "%s: got \"%s\", wanted \"%s\"", what, why.c_str(), needle);
    CHECK(std::memcmp(&u, &before, sizeof u) == 0, "%s: the setup was touched", what);
}

static void refusals() {
    const ShoeboxGeometry g = geometry();
    const PredictCrystal x = crystal(41, 45, 51);
    const double inf = 1.0 / 0.0, nan = inf - inf;
    PredictSetup u{};
    CHECK(predict_refusal(g, x, 16, 2.0, 0.01, 0.004, 300, 200, u).empty(), "the good call is refused");
    CHECK(u.h_max[0] == 21 && u.h_max[1] == 23 && u.h_max[2] == 26 && u.n_candidates == 43u * 47u * 53u, "h_max %d %d %d", u.h_max[0], u.h_max[1], u.h_max[2]);
    CHECK(u.res_limit == 0.25 && u.res_leave == 0.25 * kPredictLeaveMargin && u.s0s0 == 1.0 && u.n_images == 16 && u.W == 300 && u.H == 200, "the constants");
    CHECK(u.d_inv[0] == 1.0 && u.d_inv[4] == -1.0 && u.d_inv[8] == -0.01 && u.d_inv[2] == -70.65 / 100.0 && u.d_inv[5] == -48.8 / 100.0, "inverse(D): %g %g %g %g %g", u.d_inv[0], u.d_inv[4],
          u.d_inv[8], u.d_inv[2], u.d_inv[5]);
    for (int i = 0; i < 20; ++i) {
        ShoeboxGeometry b = g;
        double v[20];
        std::memcpy(v, &b, sizeof v);
        v[i] = i % 2 ? nan : inf;
        std::memcpy(&b, v, sizeof v);
        refused("a geometry entry that is not finite", b, x, 16, 2.0, 0.01, 0.004, "geometry has an entry that is not finite");
    }
    for (int i = 0; i < 9; ++i) {
        PredictCrystal b = x;
        b.a_matrix[i] = i % 2 ? -inf : nan;
        refused("an a_matrix entry that is not finite", g, b, 16, 2.0, 0.01, 0.004, "a_matrix has an entry that is not finite");
    }
    for (double bad : {0.0, -1.0, inf, nan}) {
        refused("dmin", g, x, 16, bad, 0.01, 0.004, "dmin must be finite and positive");
        refused("delta_b", g, x, 16, 2.0, bad, 0.004, "delta_b must be finite and positive");
        refused("delta_m", g, x, 16, 2.0, 0.01, bad, "delta_m must be finite and positive");
    }
    ShoeboxGeometry b = g;
    b.wavelength = 0.0;
    refused("wavelength", b, x, 16, 2.0, 0.01, 0.004, "wavelength and pixel sizes must be positive");
    b = g, b.pixel_size_mm[1] = -0.5;
    refused("pixel size", b, x, 16, 2.0, 0.01, 0.004, "wavelength and pixel sizes must be positive");
    b = g, b.osc_width_deg = 0.0;
    refused("osc_width", b, x, 16, 2.0, 0.01, 0.004, "osc_width_deg must not be 0");
    b = g, b.osc_width_deg = -0.5;
    CHECK(predict_refusal(b, x, 16, 2.0, 0.01, 0.004, 300, 200, u).empty(), "a negative osc_width is a scan the other way round");
    refused("n_images 0", g, x, 0, 2.0, 0.01, 0.004, "n_images must be 1 .. 65535");
    refused("n_images 65536", g, x, 65536, 2.0, 0.01, 0.004, "n_images must be 1 .. 65535");
    CHECK(predict_refusal(g, x, 65535, 2.0, 0.01, 0.004, 300, 200, u).empty(), "65535 images are refused");
    for (int c : {-1, 7, 100}) {
        PredictCrystal y = x;
        y.centring = c;
        refused("centring", g, y, 16, 2.0, 0.01, 0.004, "unknown centring");
    }
    b = g, b.rot_axis[0] = 0.0;
    refused("rot_axis", b, x, 16, 2.0, 0.01, 0.004, "rot_axis and s0 must not be zero");
    b = g, b.s0[2] = 0.0;
    refused("s0", b, x, 16, 2.0, 0.01, 0.004, "rot_axis and s0 must not be zero");
    b = g, b.d_matrix[2] = b.d_matrix[5] = b.d_matrix[8] = 0.0;
    refused("a singular D", b, x, 16, 2.0, 0.01, 0.004, "d_matrix is singular");
    PredictCrystal y = x;
    y.a_matrix[8] = 0.0;
    refused("a singular A", g, y, 16, 2.0, 0.01, 0.004, "a_matrix is singular");
    y = x;
    for (int j = 0; j < 3; ++j) y.a_matrix[3 + j] = 2.0 * y.a_matrix[j];
    refused("an A with two parallel rows", g, y, 16, 2.0, 0.01, 0.004, "a_matrix is singular");
    refused("a box of 1291^3 indices", g, crystal(2578, 2578, 2578), 16, 4.0, 0.01, 0.004, "more than 2^31 - 1 indices");   // h_max 645: 1291^3 > 2^31 - 1
    CHECK(predict_refusal(g, crystal(2574, 2574, 2574), 16, 4.0, 0.01, 0.004, 300, 200, u).empty() && u.n_candidates == 1289u * 1289u * 1289u,
          "the largest cubic box: %u", u.n_candidates);
    refused("an axis beyond 2^31 dmin", g, crystal(1e12, 10, 10), 16, 2.0, 0.01, 0.004, "more than 2^31 - 1 indices");
    PredictCrystal s = x;
    CHECK(predict_settings_refusal(g, s, 16).empty() && !predict_settings_refusal(g, s, 0).empty() && !predict_settings_refusal(g, s, 65536).empty(), "settings: n_images");
    s.a_matrix[3] = nan;
    CHECK(!predict_settings_refusal(g, s, 16).empty(), "settings: a_matrix");
}

static void random_rotation(std::mt19937_64& rng, double* R) {
    std::normal_distribution<double> nd;
    double q[4], n = 0;
    for (double& v : q) v = nd(rng), n += v * v;
    n = std::sqrt(n);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    std::memcpy(R, M, sizeof M);
}

static void brute_force() {
    std::mt19937_64 rng(20240);
    std::uniform_real_distribution<double> len(3.0, 14.0), skew(-0.3, 0.3), res(1.5, 4.0);
    const ShoeboxGeometry g = geometry();
    long inside_total = 0;
    for (int trial = 0; trial < 200; ++trial) {
        // a triclinic cell: real-space axes as rows of a sheared diagonal, turned at random; A = inverse(real)
        double real0[9] = {len(rng), 0, 0, 0, len(rng), 0, 0, 0, len(rng)};
        real0[1] = skew(rng) * real0[0], real0[2] = skew(rng) * real0[0], real0[5] = skew(rng) * real0[4];
        double R[9], real[9];
        random_rotation(rng, R);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) real[3 * i + j] = (real0[3 * i] * R[j] + real0[3 * i + 1] * R[3 + j]) + real0[3 * i + 2] * R[6 + j];
        PredictCrystal x{};
        CHECK(predict_inverse(real, x.a_matrix), "trial %d: the cell is singular", trial);
        const double dmin = trial % 10 == 0 ? std::sqrt(shoebox_dot(real, real)) / 3.0 : res(rng);   // (every tenth: |a| / dmin an integer to rounding)
        PredictSetup u{};
        CHECK(predict_refusal(g, x, 4, dmin, 0.01, 0.004, 300, 200, u).empty(), "trial %d refused", trial);
        const int pad = 3;
        for (int h = -u.h_max[0] - pad; h <= u.h_max[0] + pad; ++h)
            for (int k = -u.h_max[1] - pad; k <= u.h_max[1] + pad; ++k)
                for (int l = -u.h_max[2] - pad; l <= u.h_max[2] + pad; ++l) {
                    double r[3];
                    predict_r(x.a_matrix, (double)h, (double)k, (double)l, r);
                    if (shoebox_dot(r, r) > u.res_limit) continue;
                    ++inside_total;
                    CHECK(std::abs(h) <= u.h_max[0] && std::abs(k) <= u.h_max[1] && std::abs(l) <= u.h_max[2], "trial %d: (%d %d %d) inside the sphere, outside the box %d %d %d",
                          trial, h, k, l, u.h_max[0], u.h_max[1], u.h_max[2]);
                    CHECK(!(shoebox_dot(r, r) > u.res_leave), "trial %d: inside the limit and beyond the margin", trial);
                }
    }
    CHECK(inside_total > 20000, "the trials hold %ld indices inside their spheres", inside_total);
}

static void numbering() {
    const int32_t hm[3] = {2, 3, 5};
    uint32_t q = 0;
    for (int h = -2; h <= 2; ++h)
        for (int k = -3; k <= 3; ++k)
            for (int l = -5; l <= 5; ++l, ++q) {
                int32_t a, b, c;
                predict_index_of(hm, q, a, b, c);
                CHECK(a == h && b == k && c == l, "candidate %u is (%d %d %d), not (%d %d %d)", q, a, b, c, h, k, l);
                CHECK(predict_number_of(hm, h, k, l) == (int64_t)q, "(%d %d %d) has number %lld, not %u", h, k, l, (long long)predict_number_of(hm, h, k, l), q);
            }
    CHECK(q == 5u * 7u * 11u, "the box has %u candidates", q);
    const int32_t big[3] = {644, 644, 644};   // 1289^3 = 2 141 700 569, the largest cubic box below 2^31
    int32_t a, b, c;
    predict_index_of(big, 1289u * 1289u * 1289u - 1u, a, b, c);
    CHECK(a == 644 && b == 644 && c == 644, "the last candidate of the largest box: %d %d %d", a, b, c);
    CHECK(predict_blocks(1) == 1 && predict_blocks(256) == 1 && predict_blocks(257) == 2 && predict_blocks(0x7FFFFFFFu) == 8388608u, "predict_blocks");
}

static void absences() {
    auto mod = [](int v, int m) { return ((v % m) + m) % m; };
    for (int h = -4; h <= 4; ++h)
        for (int k = -4; k <= 4; ++k)
            for (int l = -4; l <= 4; ++l) {
                const bool want[7] = {false, mod(h + k + l, 2) != 0, !(mod(h, 2) == mod(k, 2) && mod(k, 2) == mod(l, 2)), mod(k + l, 2) != 0, mod(h + l, 2) != 0,
                                      mod(h + k, 2) != 0, mod(-h + k + l, 3) != 0};
                for (int c = 0; c < 7; ++c) CHECK(predict_absent(c, h, k, l) == want[c], "centring %d, (%d %d %d)", c, h, k, l);
            }
}

static void box_refusal() {
    std::mt19937_64 rng(77);
    std::uniform_int_distribution<int> at(-2500, 2500), size(-5, 1100), z(-3, 20);
    const double s0[3] = {0, 0, -1};
    int refused_n = 0, taken_n = 0;
    for (int i = 0; i < 20000; ++i) {
        ShoeboxEntry b{};
        b.s1[0] = 0.1, b.s1[1] = 0.2, b.s1[2] = -0.97;
        b.x_min = at(rng), b.x_max = b.x_min + size(rng), b.y_min = at(rng) / 2, b.y_max = b.y_min + size(rng), b.z_min = z(rng), b.z_max = b.z_min + z(rng);
        const bool want = !shoebox_entry_refusal(b, s0, 300, 200).empty();
        CHECK(predict_box_refused(b, 300, 200) == want, "box %d: x %d %d y %d %d z %d %d", i, b.x_min, b.x_max, b.y_min, b.y_max, b.z_min, b.z_max);
        (want ? refused_n : taken_n)++;
    }
    CHECK(refused_n > 1000 && taken_n > 1000, "%d refused, %d taken", refused_n, taken_n);
}

static void settings() {
    ShoeboxGeometry g = geometry();
    g.rot_axis[0] = 3.0, g.rot_axis[1] = 0.1, g.rot_axis[2] = -0.2;   // (not normalized: the settings normalize it)
    const PredictCrystal x = crystal(40, 45, 50);
    std::vector<double> A(17 * 9);
    predict_scan_settings(g, x.a_matrix, 16, A.data());
    CHECK(std::memcmp(A.data(), x.a_matrix, 9 * sizeof(double)) == 0, "A_0 is A when osc_start is 0 (cos 0 = 1, sin 0 = 0)");
    for (int k = 0; k <= 16; ++k) {
        // A_k B^-1 = R must be orthogonal: columns of A_k scaled by the cell lengths
        const double* M = A.data() + 9 * k;
        const double cell[3] = {40, 45, 50};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double d = 0;
                for (int r = 0; r < 3; ++r) d += M[3 * r + i] * cell[i] * M[3 * r + j] * cell[j];
                CHECK(std::fabs(d - (i == j ? 1.0 : 0.0)) < 1e-14, "scan point %d: R^T R [%d][%d] = %.17g", k, i, j, d);
            }
    }
}

int main() {
    refusals();
    brute_force();
    numbering();
    absences();
    box_refusal();
    settings();
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
