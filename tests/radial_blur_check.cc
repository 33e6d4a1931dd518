// radial_blur_check.cc -- what csrc/radial_blur_model.hpp computes, as a process of its own: the header the blurred kernels of
// kernels_radthr.hpp compile, built by tests/test_radial_blur_oracle.py once plain and once under the address and undefined-behaviour
// sanitizers.
//   radial_blur_check division        for both kernels: every reachable Wn (the sums of the kernel's weights over the subsets that hold the
//                                     centre) and, for each, S = k Wn - 1, k Wn, k Wn + 1 over random k, 0 and the largest S = Wn x (2^24 - 1):
//                                     radblur_value against `/` in 64 bits.  stdout: "W1 R w ...", "WN R wn ...", "CHECKED R n", then OK;
//                                     exit 1 with the first difference on stderr.
//   radial_blur_check frame R W H LIMIT   stdin: W x H pixel values, then W x H mask values (0 / 1).  stdout: v of every pixel, a row a line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "radial_blur_model.hpp"

using namespace ffsamd;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_random() {   // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}

static int division() {
    const uint64_t p_max = (1ull << 24) - 1;
    for (int R = 1; R <= 2; ++R) {
        const int n = 2 * R + 1;
        std::printf("W1 %d", R);
        for (int d = -R; d <= R; ++d) std::printf(" %u", radblur_w1(R, d));
        std::printf("\n");
        // the row weights are the subset sums of w1: the table the kernels' slow path reads bit by bit
        for (uint32_t bits = 0; bits < (1u << n); ++bits) {
            uint32_t w = 0;
            for (int i = 0; i < n; ++i)
                if ((bits >> i) & 1u) w += radblur_w1(R, i - R);
            if (radblur_row_weight(R, bits) != w) {
                std::fprintf(stderr, "row weight: R %d bits %u: %u, expected %u\n", R, bits, radblur_row_weight(R, bits), w);
                return 1;
            }
        }
        // reachable Wn: subset sums of the n x n weights, the centre always in
        const uint32_t full = radblur_full(R);
        std::vector<char> reach(full + 1, 0);
        reach[radblur_w1(R, 0) * radblur_w1(R, 0)] = 1;
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx) {
                if (dx == 0 && dy == 0) continue;
                const uint32_t w = radblur_w1(R, dx) * radblur_w1(R, dy);
                for (uint32_t s = full; s >= w; --s)
                    if (reach[s - w]) reach[s] = 1;
            }
        if (!reach[full]) {
            std::fprintf(stderr, "R %d: the full weight %u is not the sum of the weights\n", R, full);
            return 1;
        }
        std::printf("WN %d", R);
        unsigned long checked = 0;
        for (uint32_t wn = 1; wn <= full; ++wn) {
            if (!reach[wn]) continue;
            std::printf(" %u", wn);
            const uint64_t s_max = (uint64_t)wn * p_max;
            auto check = [&](uint64_t S) -> bool {
                if (S > s_max) return true;
                ++checked;
                const uint32_t got = radblur_value(R, (uint32_t)S, wn);
                if ((uint64_t)got == S / wn) return true;
                std::fprintf(stderr, "R %d Wn %u S %llu: %u, expected %llu\n", R, wn, (unsigned long long)S, got, (unsigned long long)(S / wn));
                return false;
            };
            if (!check(0) || !check(s_max) || !check(s_max - 1)) return 1;
            for (int i = 0; i < 4000; ++i) {
                const uint64_t k = 1 + next_random() % p_max;
                if (!check(k * wn - 1) || !check(k * wn) || !check(k * wn + 1)) return 1;
            }
        }
        std::printf("\nCHECKED %d %lu\n", R, checked);
    }
    std::printf("OK\n");
    return 0;
}

static int frame(int R, int W, int H, uint32_t limit) {
    if ((R != 1 && R != 2) || W < 1 || H < 1) return 2;
    const size_t n = (size_t)W * H;
    std::vector<uint32_t> px(n), v(n);
    std::vector<uint8_t> mask(n);
    for (size_t i = 0; i < 2 * n; ++i) {
        unsigned long x = 0;
        if (std::scanf("%lu", &x) != 1) {
            std::fprintf(stderr, "short input: %zu of %zu values\n", i, 2 * n);
            return 2;
        }
        if (i < n) px[i] = (uint32_t)x;
        else mask[i - n] = (uint8_t)(x != 0);
    }
    radblur_frame(R, px.data(), mask.data(), W, H, limit, v.data());
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) std::printf(x ? " %u" : "%u", v[(size_t)y * W + x]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "division")) return division();
    if (argc == 6 && !std::strcmp(argv[1], "frame"))
        return frame(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), (uint32_t)std::strtoul(argv[5], nullptr, 10));
    std::fprintf(stderr, "usage: radial_blur_check division | frame R W H LIMIT\n");
    return 2;
}
