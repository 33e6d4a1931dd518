// jungfrau_model.hpp -- the gain-stage conversion of raw Jungfrau words (FFS_CODEC_JUNGFRAU_RAW) as plain C++: the
// stage of a word, the words that are invalid, the two float32 operations, the rounding and the clamp.  No HIP header: the kernel
// (kernels_jungfrau.hpp), the host converter (host/codecs.hpp) and a plain C++ test program (tests/jungfrau_check.cc) compile the same text.
// The reference has no counterpart -- its readers hand over photon counts -- and no parity with an external converter is claimed: the rule
// is the library's own.
//
// A raw word r (uint16) is two bits of gain code g = r >> 14 and 14 bits of ADC, adc = r & 0x3FFF.  The stage is s = 0, 1, 2 for
// g = 0, 1, 3 (G0, G1, G2); g == 2 does not occur in a working pixel.  Pixel k has pedestal[s][k] and factor[s][k], float32; the factor is
// photons per ADU, 1 / (gain_s x photon energy), negative for the inverted stages, and 0 is the caller's mark for "no calibration for this
// pixel in this stage".
//   invalid  g == 2, r == 0xFFFF, r == 0xC000 (G2 with ADC 0: the saturated word) or factor[s][k] == 0: the output is 0xFFFFFFFF.
//   else     d = (float)adc - pedestal and v = d * factor, each ONE float32 operation (built with -ffp-contract=off everywhere: (a - b) * c
//            cannot contract into a fused operation anyway), q = rintf(v), ties to even; the output is 0 for q <= 0, 16777215 for
//            q >= 16777215 and (uint32_t)q otherwise.
// A denormal d or v rounds to 0 with or without flushing, so the result does not depend on the denormal mode: a denormal pedestal changes
// (float)adc - pedestal only where adc == 0, and then |d| < 2^-126, |v| <= 2^16 |d| and q is a zero of either sign either way; a denormal v
// from a normal d is below 2^-126 and rounds to that zero too.  With the setter's ranges (ffs_ctx_set_jungfrau_calibration: entries finite,
// |pedestal| <= 65536, factor 0 or |factor| in [2^-30, 2^16]) |v| < 2^33: nothing overflows and no NaN arises.
//
// 0xFFFFFFFF needs nothing new downstream.  Every window, the radial profile, the pixel statistics, the blur and the spot backgrounds leave
// out 32-bit pixels >= 2^24 (launch_geometry.hpp, counting_limit), so an invalid pixel is masked for its frame; with max_valid <= 2^24 - 1,
// which the driver sets, such a centre is never strong either, and the fast kernel k_stream_u32 runs unchanged.  WITHOUT max_valid
// (max_valid < 0: no limit) the pixel still counts in no window, but as a centre it is compared like any other value and 0xFFFFFFFF
// stands above every threshold: it comes out as a strong pixel of intensity 0xFFFFFFFF.  Set max_valid.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FFS_JF_HD __host__ __device__
#else
#define FFS_JF_HD
#endif

namespace ffsamd {

constexpr uint32_t kJfInvalid = 0xFFFFFFFFu;    // the output of an invalid word
constexpr uint32_t kJfMaxPhotons = 16777215u;   // 2^24 - 1: what the 32-bit paths hold exactly, the clamp
// what ffs_ctx_set_jungfrau_calibration accepts (the check is jf_entry_ok)
constexpr float kJfMaxPedestal = 65536.0f, kJfMinFactor = 0x1p-30f, kJfMaxFactor = 65536.0f;

// the stage of a raw word: 0, 1, 2 for the gain codes 0, 1, 3 (and 2 for the code 2, whose words are invalid)
FFS_JF_HD inline uint32_t jf_stage(uint32_t r) { return (r >> 14) == 0u ? 0u : (r >> 14) == 1u ? 1u : 2u; }
// invalid by the word alone
FFS_JF_HD inline bool jf_word_invalid(uint32_t r) { return (r >> 14) == 2u || r == 0xFFFFu || r == 0xC000u; }

// one pixel from its word and the pedestal and factor of the word's stage
FFS_JF_HD inline uint32_t jf_convert(uint32_t r, float pedestal, float factor) {
    const float d = (float)(r & 0x3FFFu) - pedestal;
    const float v = d * factor;
    const float q = rintf(v);
    const uint32_t n = q <= 0.0f ? 0u : q >= 16777215.0f ? kJfMaxPhotons : (uint32_t)q;
    return (jf_word_invalid(r) || factor == 0.0f) ? kJfInvalid : n;
}

// ... and from the pixel's three pairs: the selects are branchless (a lane's eight pixels differ in stage)
FFS_JF_HD inline uint32_t jf_photons(uint32_t r, float p0, float p1, float p2, float f0, float f1, float f2) {
    const uint32_t g = r >> 14;
    const float p = g == 0u ? p0 : g == 1u ? p1 : p2;
    const float f = g == 0u ? f0 : g == 1u ? f1 : f2;
    return jf_convert(r, p, f);
}

// may `v` be entry of a pedestal plane (is_factor false) or of a factor plane?  (false for a NaN)
inline bool jf_entry_ok(bool is_factor, float v) {
    if (!is_factor) return v >= -kJfMaxPedestal && v <= kJfMaxPedestal;
    const float a = v < 0.0f ? -v : v;
    return v == 0.0f || (a >= kJfMinFactor && a <= kJfMaxFactor);
}

// a whole frame of n pixels on the host: six dense planes, raw little-endian words (the host converter's loop)
inline void jf_convert_frame(const uint16_t* raw, size_t n, const float* const pedestal[3], const float* const factor[3], uint32_t* out) {
    for (size_t k = 0; k < n; ++k) out[k] = jf_photons(raw[k], pedestal[0][k], pedestal[1][k], pedestal[2][k], factor[0][k], factor[1][k], factor[2][k]);
}

}  // namespace ffsamd
