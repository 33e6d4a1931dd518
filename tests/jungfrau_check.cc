// jungfrau_check.cc -- what csrc/jungfrau_model.hpp computes, as a process of its own: the header the kernel of kernels_jungfrau.hpp and the
// host converter compile, built by tests/test_jungfrau_oracle.py with g++ -ffp-contract=off, once plain and once under the address and
// undefined-behaviour sanitizers.  Floats cross as their bit patterns, so nothing is lost to text.
//   jungfrau_check frame N    stdin: N raw words, then 6 N float32 bit patterns (pedestal G0, G1, G2, factor G0, G1, G2, a plane after the
//                             other).  stdout: the N converted pixels, one a line (jf_convert_frame).
//   jungfrau_check entry      stdin: pairs "is_factor bits" to the end of input.  stdout: 1 or 0 per pair (jf_entry_ok).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jungfrau_model.hpp"

using namespace ffsamd;

static float float_of(uint32_t bits) {
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

static int frame(size_t n) {
    std::vector<uint16_t> raw(n);
    std::vector<float> planes(6 * n);
    std::vector<uint32_t> out(n);
    for (size_t i = 0; i < 7 * n; ++i) {
        unsigned long x = 0;
        if (std::scanf("%lu", &x) != 1) {
            std::fprintf(stderr, "short input: %zu of %zu values\n", i, 7 * n);
            return 2;
        }
        if (i < n) raw[i] = (uint16_t)x;
        else planes[i - n] = float_of((uint32_t)x);
    }
    const float* const ped[3] = {planes.data(), planes.data() + n, planes.data() + 2 * n};
    const float* const fac[3] = {planes.data() + 3 * n, planes.data() + 4 * n, planes.data() + 5 * n};
    jf_convert_frame(raw.data(), n, ped, fac, out.data());
    for (size_t i = 0; i < n; ++i) std::printf("%u\n", out[i]);
    return 0;
}

static int entry() {
    unsigned long is_factor = 0, bits = 0;
    while (std::scanf("%lu %lu", &is_factor, &bits) == 2) std::printf("%d\n", jf_entry_ok(is_factor != 0, float_of((uint32_t)bits)) ? 1 : 0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "frame")) return frame((size_t)std::strtoull(argv[2], nullptr, 10));
    if (argc == 2 && !std::strcmp(argv[1], "entry")) return entry();
    std::fprintf(stderr, "usage: jungfrau_check frame N | entry\n");
    return 2;
}
