// radial_threshold_check.cc -- what csrc/radial_threshold_model.hpp decides, as a process of its own: the header the kernel compiles, built by
// tests/test_radial_threshold_oracle.py once plain and once under the address and undefined-behaviour sanitizers.
//   radial_threshold_check            stdin: the text form of float64 n_iqr ("%a"), then histograms of 257 counters each (the values 0 .. 255
//                                     and the tail), whitespace-separated.  stdout: one line a histogram,
//                                     "n_pixels n_overflow q1 median q3 cutoff status".  Exit 2 when the input ends inside a histogram.
//   radial_threshold_check cutoff     stdin: triples "median iqr n_iqr" (n_iqr as "%a"); stdout: one cutoff a line.
//   radial_threshold_check route      stdout: "R algorithm pixel_bytes path rerun window_kernel | stage bright_to_plane ext_variant" over the
//                                     tuning of csrc/threshold_route.hpp, then OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "radial_threshold_model.hpp"
#include "threshold_route.hpp"

using namespace ffsamd;

static int route_rows() {
    for (int algorithm = 0; algorithm <= 2; ++algorithm)
        for (int pixel_bytes : {2, 4})
            for (int path = 0; path <= 2; ++path)
                for (int rerun : {-1, 1})
                    for (int window_kernel = 0; window_kernel <= 1; ++window_kernel) {
                        Tuning t;
                        t.threshold_path = path;
                        t.window_kernel = window_kernel;
                        const ThresholdRoute r = threshold_route(algorithm, pixel_bytes, true, FFS_MAX_VALID_CENTRE, -1, 0.0, rerun, t);
                        std::printf("R %d %d %d %d %d | %d %d %d\n", algorithm, pixel_bytes, path, rerun, window_kernel, (int)r.stage, r.bright_to_plane,
                                    r.ext_variant);
                    }
    std::printf("K %d\n", (int)ThresholdStage::kRadial);
    std::printf("OK\n");
    return 0;
}

static int cutoffs() {
    long median = 0, iqr = 0;
    double n_iqr = 0.0;
    while (std::scanf("%ld %ld %la", &median, &iqr, &n_iqr) == 3) std::printf("%u\n", radthr_cutoff((int32_t)median, (int32_t)iqr, n_iqr));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "route")) return route_rows();
    if (argc > 1 && !std::strcmp(argv[1], "cutoff")) return cutoffs();
    double n_iqr = 0.0;
    if (std::scanf("%la", &n_iqr) != 1) {
        std::fprintf(stderr, "no n_iqr\n");
        return 2;
    }
    std::vector<uint32_t> h(kRadThrCounters);
    for (;;) {
        int got = 0;
        for (; got < kRadThrCounters; ++got) {
            unsigned long v = 0;
            if (std::scanf("%lu", &v) != 1) break;
            h[(size_t)got] = (uint32_t)v;
        }
        if (got == 0) break;
        if (got < kRadThrCounters) {
            std::fprintf(stderr, "short histogram: %d of %d counters\n", got, kRadThrCounters);
            return 2;
        }
        const RadThrShell r = radthr_from_histogram(h.data(), n_iqr);
        std::printf("%u %u %d %d %d %u %u\n", r.n_pixels, r.n_overflow, r.q1, r.median, r.q3, r.cutoff, r.status);
    }
    return 0;
}
