// jungfrau_pedestal_check.cc -- what csrc/jungfrau_pedestal_model.hpp computes, as a process of its own: the header the kernel of
// kernels_jfped.hpp, the library's host function, the driver and ffs_hosttool compile, built by tests/test_jungfrau_pedestal_oracle.py with
// g++ -ffp-contract=off, once plain and once under the address and undefined-behaviour sanitizers.  Floats cross as their bit patterns.
//   jungfrau_pedestal_check fold F N     stdin: F frames of N raw words.  stdout: 9 N lines -- count G0 G1 G2, sum G0 G1 G2, sum_sq G0 G1 G2,
//                                        a plane after the other (jf_pedestal_fold_frame, F times into one accumulator set).
//   jungfrau_pedestal_check planes M R   M = min_frames, R = the bits of max_rms.  stdin: triples "count sum sum_sq" to the end of input.
//                                        stdout: "pedestal-bits rms-bits ok" per triple (jf_pedestal_entry).
//   jungfrau_pedestal_check args         stdin: pairs "min_frames max_rms-bits".  stdout: 1 or 0 per pair (jf_pedestal_args_ok).
//   jungfrau_pedestal_check fit          stdin: pairs "have n".  stdout: 1 or 0 per pair (jf_pedestal_frames_fit).
//   jungfrau_pedestal_check repedestal N stdin: 6 N old bits, 3 N pedestal bits, 3 N ok.  stdout: 6 N bits (jf_repedestal).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jungfrau_pedestal_model.hpp"

using namespace ffsamd;

static float float_of(uint32_t bits) {
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

static int fold(size_t frames, size_t n) {
    std::vector<uint16_t> raw(n);
    std::vector<uint32_t> count(3 * n, 0u);
    std::vector<uint64_t> sum(3 * n, 0ull), sum_sq(3 * n, 0ull);
    uint32_t* const c[3] = {count.data(), count.data() + n, count.data() + 2 * n};
    uint64_t* const s[3] = {sum.data(), sum.data() + n, sum.data() + 2 * n};
    uint64_t* const q[3] = {sum_sq.data(), sum_sq.data() + n, sum_sq.data() + 2 * n};
    for (size_t f = 0; f < frames; ++f) {
        for (size_t i = 0; i < n; ++i) {
            unsigned long x = 0;
            if (std::scanf("%lu", &x) != 1) {
                std::fprintf(stderr, "short input in frame %zu\n", f);
                return 2;
            }
            raw[i] = (uint16_t)x;
        }
        jf_pedestal_fold_frame(raw.data(), n, c, s, q);
    }
    for (size_t i = 0; i < 3 * n; ++i) std::printf("%u\n", count[i]);
    for (size_t i = 0; i < 3 * n; ++i) std::printf("%llu\n", (unsigned long long)sum[i]);
    for (size_t i = 0; i < 3 * n; ++i) std::printf("%llu\n", (unsigned long long)sum_sq[i]);
    return 0;
}

static int planes(uint32_t min_frames, float max_rms) {
    unsigned long long c = 0, s = 0, q = 0;
    while (std::scanf("%llu %llu %llu", &c, &s, &q) == 3) {
        const JfPedestalEntry e = jf_pedestal_entry((uint32_t)c, s, q, min_frames, max_rms);
        std::printf("%u %u %u\n", bits_of(e.pedestal), bits_of(e.rms), (unsigned)e.ok);
    }
    return 0;
}

static int args() {
    unsigned long long m = 0, bits = 0;
    while (std::scanf("%llu %llu", &m, &bits) == 2) std::printf("%d\n", jf_pedestal_args_ok((uint32_t)m, float_of((uint32_t)bits)) ? 1 : 0);
    return 0;
}

static int fit() {
    unsigned long long have = 0, n = 0;
    while (std::scanf("%llu %llu", &have, &n) == 2) std::printf("%d\n", jf_pedestal_frames_fit(have, n) ? 1 : 0);
    return 0;
}

static int repedestal(size_t n) {
    std::vector<float> old(6 * n), ped(3 * n), out(6 * n);
    std::vector<uint8_t> ok(3 * n);
    for (size_t i = 0; i < 12 * n; ++i) {
        unsigned long x = 0;
        if (std::scanf("%lu", &x) != 1) {
            std::fprintf(stderr, "short input: %zu of %zu values\n", i, 12 * n);
            return 2;
        }
        if (i < 6 * n) old[i] = float_of((uint32_t)x);
        else if (i < 9 * n) ped[i - 6 * n] = float_of((uint32_t)x);
        else ok[i - 9 * n] = (uint8_t)x;
    }
    const float* const p[3] = {ped.data(), ped.data() + n, ped.data() + 2 * n};
    const uint8_t* const k[3] = {ok.data(), ok.data() + n, ok.data() + 2 * n};
    jf_repedestal(old.data(), n, p, k, out.data());
    for (size_t i = 0; i < 6 * n; ++i) std::printf("%u\n", bits_of(out[i]));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "fold")) return fold((size_t)std::strtoull(argv[2], nullptr, 10), (size_t)std::strtoull(argv[3], nullptr, 10));
    if (argc == 4 && !std::strcmp(argv[1], "planes")) return planes((uint32_t)std::strtoull(argv[2], nullptr, 10), float_of((uint32_t)std::strtoull(argv[3], nullptr, 10)));
    if (argc == 2 && !std::strcmp(argv[1], "args")) return args();
    if (argc == 2 && !std::strcmp(argv[1], "fit")) return fit();
    if (argc == 3 && !std::strcmp(argv[1], "repedestal")) return repedestal((size_t)std::strtoull(argv[2], nullptr, 10));
    std::fprintf(stderr, "usage: jungfrau_pedestal_check fold F N | planes M R | args | fit | repedestal N\n");
    return 2;
}
