// spot_background_glm_check.cc -- the robust Poisson GLM background (csrc/spot_background_glm_model.hpp, the text the kernel compiles) in a
// plain C++ program: reads histograms from stdin, 257 unsigned integers each (the counts of the bins 0 .. 255, then the count of the tail),
// and prints one line per histogram: n_pixels n_overflow median n_iter status beta mean, the two doubles as the 16 hex digits of their bit
// patterns (the format of `ffs_hosttool spotbgglm`).  tests/test_spot_background_glm_oracle.py builds it plain and under the address and
// undefined-behaviour sanitizers and compares its lines with tests/spot_background_glm_oracle.py and the golden file.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spot_background_glm_model.hpp"

static uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

int main() {
    using namespace ffsamd;
    std::vector<uint32_t> bins(kSpotBgBins);
    unsigned long long lines = 0;
    for (;;) {
        int got = 0;
        for (; got < kSpotBgBins; ++got)
            if (std::scanf("%" SCNu32, &bins[(size_t)got]) != 1) break;
        if (got == 0) break;
        uint32_t tail = 0;
        if (got != kSpotBgBins || std::scanf("%" SCNu32, &tail) != 1) {
            std::fprintf(stderr, "histogram %llu is short: 257 integers each\n", lines);
            return 2;
        }
        const SpotBgGlmResult r = spotbg_glm_from_histogram(bins.data(), tail);
        std::printf("%" PRIu32 " %" PRIu32 " %" PRId32 " %" PRIu32 " %" PRIu32 " %016" PRIx64 " %016" PRIx64 "\n", r.n_pixels, r.n_overflow, r.median, r.n_iter,
                    r.status, bits_of(r.beta), bits_of(r.mean));
        ++lines;
    }
    return 0;
}
