// spot_background_check.cc -- the decisions of the per-spot background (csrc/spot_background_model.hpp, the text the kernel compiles) in a
// plain C++ program: reads histograms from stdin, 257 unsigned integers each (the counts of the bins 0 .. 255, then the count of the tail),
// and prints one line per histogram: n_pixels n_overflow q1 median q3 n_inliers inlier_sum status.  tests/test_spot_background_oracle.py
// builds it plain and under the address and undefined-behaviour sanitizers and compares its lines with tests/spot_background_oracle.py.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "spot_background_model.hpp"

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
        const SpotBgResult r = spotbg_from_histogram(bins.data(), tail);
        std::printf("%" PRIu32 " %" PRIu32 " %" PRId32 " %" PRId32 " %" PRId32 " %" PRIu32 " %" PRIu64 " %" PRIu32 "\n", r.n_pixels, r.n_overflow, r.q1, r.median,
                    r.q3, r.n_inliers, r.inlier_sum, r.status);
        ++lines;
    }
    return 0;
}
