// radial_bins_check.cc -- host/radial_bins.hpp on its own, in a plain program (tests/test_radial_params.py builds it once as it is
// and once under the address and undefined-behaviour sanitizers):
//   radial_bins_check                    the checks below; prints FAIL lines, then OK, exit code 0 iff none failed
//   radial_bins_check dump FILE W H N wavelength distance_m beam_x_px beam_y_px pixel_x_m pixel_y_m
//                                        the builder's map as W*H little-endian uint16 into FILE and its d edges on stdout; the six
//                                        numbers are parsed as float32 and widened, as the driver's geometry is
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "radial_bins.hpp"

using namespace ffshost;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL ");         \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            ++failures;                   \
        }                                 \
    } while (0)

static double radius(const RadialGeometry& g, uint32_t x, uint32_t y) {
    const double dx = (((double)x + 0.5) - g.beam_center_x) * g.pixel_size_x, dy = (((double)y + 0.5) - g.beam_center_y) * g.pixel_size_y;
    return std::sqrt(dx * dx + dy * dy);
}

static void check_detector(uint32_t W, uint32_t H, const RadialGeometry& g, const char* name) {
    for (uint32_t N : {1u, 2u, 7u, 8u, 100u, 1024u}) {
        const RadialBins b = radial_bins(g, W, H, N);
        CHECK(b.n_bins == N && b.bin_of_pixel.size() == (size_t)W * H, "%s N=%u: sizes", name, N);
        // every pixel in a shell < N; N = 1 puts everything in shell 0
        uint32_t top = 0;
        for (uint16_t v : b.bin_of_pixel) top = std::max<uint32_t>(top, v);
        CHECK(top < N, "%s N=%u: a pixel in shell %u", name, N, top);
        if (N == 1) CHECK(top == 0, "%s N=1: shell %u", name, top);
        // monotone in the radius from the beam centre: a pixel further out is never in a lower shell
        std::vector<double> far_of(N, -1.0), near_of(N, 1e300);
        size_t far_i = 0;
        double far_r = -1.0;
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                const size_t i = (size_t)y * W + x;
                const double r = radius(g, x, y);
                const uint16_t s = b.bin_of_pixel[i];
                far_of[s] = std::max(far_of[s], r);
                near_of[s] = std::min(near_of[s], r);
                if (r > far_r) { far_r = r; far_i = i; }
            }
        double seen = -1.0;
        for (uint32_t s = 0; s < N; ++s) {
            if (far_of[s] < 0) continue;
            CHECK(near_of[s] >= seen, "%s N=%u: shell %u starts at r = %.17g, inside a lower shell that reaches %.17g", name, N, s, near_of[s], seen);
            seen = far_of[s];
        }
        // the pixel furthest out -- a corner -- sits exactly on the last edge and belongs to shell N - 1
        const uint32_t fx = (uint32_t)(far_i % W), fy = (uint32_t)(far_i / W);
        CHECK((fx == 0 || fx == W - 1) && (fy == 0 || fy == H - 1), "%s N=%u: the furthest pixel (%u, %u) is no corner", name, N, fx, fy);
        CHECK(b.bin_of_pixel[far_i] == N - 1, "%s N=%u: the corner pixel is in shell %u", name, N, (unsigned)b.bin_of_pixel[far_i]);
        // the edges: infinity, then decreasing down to the corner's d
        CHECK(std::isinf(b.d_edge(0)), "%s N=%u: first edge", name, N);
        for (uint32_t k = 1; k < N; ++k) CHECK(b.d_edge(k) > b.d_edge(k + 1), "%s N=%u: edges %u, %u", name, N, k, k + 1);
        CHECK(std::fabs(1.0 / (b.d_edge(N) * b.d_edge(N)) - b.inv_d2_max) <= 1e-12 * b.inv_d2_max, "%s N=%u: last edge", name, N);
    }
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "dump") == 0) {
        if (argc != 12) {
            std::printf("usage: radial_bins_check dump FILE W H N wavelength distance_m beam_x_px beam_y_px pixel_x_m pixel_y_m\n");
            return 2;
        }
        const uint32_t W = (uint32_t)std::atoi(argv[3]), H = (uint32_t)std::atoi(argv[4]), N = (uint32_t)std::atoi(argv[5]);
        float v[6];
        for (int i = 0; i < 6; ++i) v[i] = std::strtof(argv[6 + i], nullptr);
        const RadialBins b = radial_bins(RadialGeometry{v[0], v[1], v[2], v[3], v[4], v[5]}, W, H, N);
        FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(b.bin_of_pixel.data(), 2, b.bin_of_pixel.size(), f) != b.bin_of_pixel.size()) return 2;
        std::fclose(f);
        for (uint32_t k = 0; k <= N; ++k) std::printf("%.17g\n", b.d_edge(k));
        return 0;
    }
    // the two detectors of the issue: beam centre inside, off the middle and off every pixel centre; and one with the beam off the detector
    check_detector(37, 29, RadialGeometry{0.976, 0.3, 17.3, 11.9, 75e-6, 75e-6}, "37x29");
    check_detector(64, 64, RadialGeometry{1.0, 0.15, 32.0, 32.0, 172e-6, 172e-6}, "64x64");
    check_detector(64, 64, RadialGeometry{0.5, 0.1, -40.25, 20.5, 172e-6, 100e-6}, "64x64 beam outside");
    // a single pixel on the beam centre: 1/d^2 is 0 everywhere, everything in shell 0
    const RadialBins one = radial_bins(RadialGeometry{1.0, 0.1, 0.5, 0.5, 1e-4, 1e-4}, 1, 1, 8);
    CHECK(one.bin_of_pixel.size() == 1 && one.bin_of_pixel[0] == 0, "1x1 on the beam");
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("OK\n");
    return failures ? 1 : 0;
}
