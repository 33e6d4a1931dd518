// threshold_route_check.cc -- a batch's route through the threshold stage (csrc/threshold_route.hpp) without a GPU: built and run by
// tests/test_threshold_route.py (g++ with the address and undefined-behaviour sanitizers, against that header alone).  Prints the route for
// the full product of its inputs ("R" lines: the inputs | the route) and the instantiation rule for every kernel family, pixel size and
// variant ("I" lines); the test restates the rules and compares.
#include <cstdio>
#include <initializer_list>

#include "threshold_route.hpp"

using namespace ffsamd;

int main() {
    for (int algorithm : {FFS_ALGO_DISPERSION, FFS_ALGO_DISPERSION_EXTENDED})
    for (int pixel_bytes : {2, 4})
    for (int window_3x3 : {1, 0})
    for (int scope : {FFS_MAX_VALID_CENTRE, FFS_MAX_VALID_WINDOW})
    for (long long max_valid : {-1ll, 1000ll})
    for (double gain : {0.0, 2.5})
    for (int path : {0, 1, 2})
    for (int rerun : {-1, 1})
    for (int window_kernel : {0, 1})
    for (int ext_first_pass : {0, 2})
    for (int ext_fused : {0, 1}) {
        Tuning t;
        t.threshold_path = path;
        t.window_kernel = window_kernel;
        t.ext_first_pass = ext_first_pass;
        t.ext_fused = ext_fused;
        const ThresholdRoute r = threshold_route(algorithm, pixel_bytes, window_3x3 != 0, scope, max_valid, gain, rerun, t);
        std::printf("R %d %d %d %d %lld %.1f %d %d %d %d %d | %d %d %d %d %d %d %d %d %d\n", algorithm, pixel_bytes, window_3x3, scope, max_valid, gain, path, rerun,
                    window_kernel, ext_first_pass, ext_fused, (int)r.stage, (int)r.variant, (int)r.window_scope, r.bright_to_plane, r.ext_variant,
                    (int)r.ext_streams_first(), (int)r.ext_fused, (int)r.ext(), (int)r.has_dense_kernel());
    }
    for (int family = (int)KernelFamily::kExact; family <= (int)KernelFamily::kExtFirst; ++family)
        for (size_t pixel_bytes : {2, 4})
            for (int v = 0; v < 3; ++v) {
                const KernelFamily f = (KernelFamily)family;
                const Predicate as = instantiated_as(f, pixel_bytes, (Predicate)v);
                std::printf("I %d %zu %d | %d %d %d\n", family, pixel_bytes, v, (int)as, (int)compares_limit(f, pixel_bytes, as), (int)gain_form(as));
            }
    std::printf("OK\n");
    return 0;
}
