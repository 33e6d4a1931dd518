// threshold_route_map_check.cc -- threshold_route_check.cc's product of inputs x {no map, a gain map} (csrc/threshold_route.hpp; the map is
// the route's trailing, defaulted input), without a GPU: built and run by tests/test_threshold_route_map.py (g++ with the address and
// undefined-behaviour sanitizers, against that header alone).  "R" lines: the inputs, the map last | the route; "I" lines: the instantiation rule
// for every kernel family and pixel size at variant 3 (kGainMap), with the answer to gain_from_map() last.
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
    for (int ext_fused : {0, 1})
    for (int map : {0, 1}) {
        Tuning t;
        t.threshold_path = path;
        t.window_kernel = window_kernel;
        t.ext_first_pass = ext_first_pass;
        t.ext_fused = ext_fused;
        const ThresholdRoute r = threshold_route(algorithm, pixel_bytes, window_3x3 != 0, scope, max_valid, gain, rerun, t, map != 0);
        std::printf("R %d %d %d %d %lld %.1f %d %d %d %d %d %d | %d %d %d %d %d %d %d %d %d\n", algorithm, pixel_bytes, window_3x3, scope, max_valid, gain, path, rerun,
                    window_kernel, ext_first_pass, ext_fused, map, (int)r.stage, (int)r.variant, (int)r.window_scope, r.bright_to_plane, r.ext_variant,
                    (int)r.ext_streams_first(), (int)r.ext_fused, (int)r.ext(), (int)r.has_dense_kernel());
    }
    static_assert((int)Predicate::kPhotonCount == 0 && (int)Predicate::kWindowScope == 1 && (int)Predicate::kGain == 2 && (int)Predicate::kGainMap == 3);
    static_assert(!gain_from_map(Predicate::kPhotonCount) && !gain_from_map(Predicate::kWindowScope) && !gain_from_map(Predicate::kGain));
    for (int family = (int)KernelFamily::kExact; family <= (int)KernelFamily::kExtFirst; ++family)
        for (size_t pixel_bytes : {2, 4}) {
            const KernelFamily f = (KernelFamily)family;
            const Predicate as = instantiated_as(f, pixel_bytes, Predicate::kGainMap);
            std::printf("I %d %zu 3 | %d %d %d %d\n", family, pixel_bytes, (int)as, (int)compares_limit(f, pixel_bytes, as), (int)gain_form(as), (int)gain_from_map(as));
        }
    std::printf("OK\n");
    return 0;
}
