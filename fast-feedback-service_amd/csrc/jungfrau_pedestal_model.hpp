// jungfrau_pedestal_model.hpp -- Jungfrau pedestals from dark frames (ffs_stream_jungfrau_pedestal_fold, ffs_jungfrau_pedestal_planes, DESIGN.md
// section 5e) as plain C++: which words of a dark frame count where, and how the accumulators become pedestal, noise and "usable" planes.
// No HIP header: the kernel (kernels_jfped.hpp), the library's host function, the driver's host fold (--cpu-decode), ffs_hosttool and a plain
// C++ test program (tests/jungfrau_pedestal_check.cc) compile the same text.  The stage of a word and the invalid words are
// jungfrau_model.hpp's (jf_stage, jf_word_invalid) and are not restated.  The reference has no counterpart.
//
// FOLD.  A frame is W * H little-endian 16-bit words.  A word r at flat pixel k with jf_word_invalid(r) (gain code 2, 0xFFFF, 0xC000) counts
// nowhere.  Otherwise, with s = jf_stage(r) and a = r & 0x3FFF: count[s][k] += 1, sum[s][k] += a, sum_sq[s][k] += a * a.  The word decides the
// stage: a run needs no label, one accumulator set takes G0, G1 and G2 frames in any order, and no calibration plays a part.  count is
// uint32, sum and sum_sq are uint64: with a < 2^14 they cannot wrap while fewer than 2^32 frames are folded (a^2 < 2^28, 2^28 * 2^32 = 2^60),
// and a fold that would take the frame count past 2^32 - 1 is refused (jf_pedestal_frames_fit).
//
// PLANES.  One stage of one pixel, c = count: c == 0 gives pedestal 0, rms 0, ok 0.  Otherwise, in float64, every operation rounded on its own
// (-ffp-contract=off wherever this is compiled): m = (double)sum / (double)c, q = (double)sum_sq / (double)c, v = q - m * m,
// pedestal = (float)m, rms = (float)sqrt(v > 0 ? v : 0), ok = c >= min_frames && (max_rms == 0 || rms <= max_rms).  The integer-to-double
// conversions round to nearest, ties to even (the C cast; sum_sq can exceed 2^53).  min_frames >= 1; max_rms is a finite float >= 0 and 0
// means no noise test.  This is the NumPy float64 / float32 rule, bit for bit (tests/jungfrau_pedestal_oracle.py).
//
// RE-PEDESTALLED CALIBRATION.  From a 6-plane calibration and the planes above: the pedestal planes are replaced; factor[s][k] is kept where
// ok[s][k] holds and 0 elsewhere -- 0 is the library's mark for "no calibration for this pixel in this stage" (jungfrau_model.hpp).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "jungfrau_model.hpp"

namespace ffsamd {

constexpr uint64_t kJfPedMaxFrames = 0xFFFFFFFFull;   // frames one accumulator set holds: count is 32 bits

// the ADC of a word, what is summed
FFS_JF_HD inline uint32_t jf_pedestal_adc(uint32_t r) { return r & 0x3FFFu; }

// may n more frames be folded behind `have`?
inline bool jf_pedestal_frames_fit(uint64_t have, uint64_t n) { return have <= kJfPedMaxFrames && n <= kJfPedMaxFrames - have; }

// one frame of n words into dense accumulator planes on the host (the loop --cpu-decode runs)
inline void jf_pedestal_fold_frame(const uint16_t* raw, size_t n, uint32_t* const count[3], uint64_t* const sum[3], uint64_t* const sum_sq[3]) {
    for (size_t k = 0; k < n; ++k) {
        const uint32_t r = raw[k];
        if (jf_word_invalid(r)) continue;
        const uint32_t s = jf_stage(r);
        const uint64_t a = jf_pedestal_adc(r);
        count[s][k] += 1u;
        sum[s][k] += a;
        sum_sq[s][k] += a * a;
    }
}

// what ffs_jungfrau_pedestal_planes accepts (false for a NaN)
inline bool jf_pedestal_args_ok(uint32_t min_frames, float max_rms) { return min_frames >= 1u && max_rms >= 0.0f && max_rms <= 3.4028234663852886e38f; }

struct JfPedestalEntry {
    float pedestal, rms;
    uint8_t ok;
};

// one stage of one pixel
inline JfPedestalEntry jf_pedestal_entry(uint32_t c, uint64_t sum, uint64_t sum_sq, uint32_t min_frames, float max_rms) {
    if (c == 0u) return JfPedestalEntry{0.0f, 0.0f, 0};
    const double n = (double)c;
    const double m = (double)sum / n;
    const double q = (double)sum_sq / n;
    const double mm = m * m;
    const double v = q - mm;
    const float rms = (float)sqrt(v > 0.0 ? v : 0.0);
    return JfPedestalEntry{(float)m, rms, (uint8_t)((c >= min_frames && (max_rms == 0.0f || rms <= max_rms)) ? 1 : 0)};
}

// a plane of n entries; any output may be null
inline void jf_pedestal_plane(const uint32_t* count, const uint64_t* sum, const uint64_t* sum_sq, size_t n, uint32_t min_frames, float max_rms, float* pedestal,
                              float* rms, uint8_t* ok) {
    for (size_t k = 0; k < n; ++k) {
        const JfPedestalEntry e = jf_pedestal_entry(count[k], sum[k], sum_sq[k], min_frames, max_rms);
        if (pedestal) pedestal[k] = e.pedestal;
        if (rms) rms[k] = e.rms;
        if (ok) ok[k] = e.ok;
    }
}

// the re-pedestalled calibration: old and out are six planes of n floats (pedestal G0 G1 G2, factor G0 G1 G2; out may be old)
inline void jf_repedestal(const float* old, size_t n, const float* const pedestal[3], const uint8_t* const ok[3], float* out) {
    for (int s = 0; s < 3; ++s)
        for (size_t k = 0; k < n; ++k) {
            out[(size_t)(3 + s) * n + k] = ok[s][k] ? old[(size_t)(3 + s) * n + k] : 0.0f;
            out[(size_t)s * n + k] = pedestal[s][k];
        }
}

}  // namespace ffsamd
