// ffs_device.h -- shared host/device definitions for libffs_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch_geometry.hpp"
#include "sweep_plan.hpp"
#include "threshold_route.hpp"

// Timing experiments (phases switched off, kernels stopped half way: results are wrong when used) exist only in builds
// with -DFFS_EXPERIMENTS (make experiments -> libffs_hip_exp.so, for tools/); the product library has none of them.
#ifdef FFS_EXPERIMENTS
#define FFS_DBG(args, bit) (((args).dbg & (bit)) != 0)
#define FFS_STOP_AFTER(A, phase) if ((A).stop_after == (phase)) return
// (experiments) device timestamps at the phase boundaries of the sparse launch, one set per frame: tools/chain_phase_times.sh
#define FFS_PHASE_TS(A, idx) do { if ((A).phase_ts && threadIdx.x == 0) (A).phase_ts[(size_t)blockIdx.x * 8 + (idx)] = wall_clock64(); } while (0)
#else
#define FFS_PHASE_TS(A, idx) do {} while (0)
#define FFS_DBG(args, bit) false
#define FFS_STOP_AFTER(A, phase) do {} while (0)
#endif

namespace ffsamd {

// The frame layout in HBM (Layout), the geometry constants of the kernels (kSOwned, kWinOwned, ...) and the unit map as plain integers
// (band_first_row, stream_unit_of, log_slot_of) are in launch_geometry.hpp, which has no HIP in it.
constexpr int kInfoExtraRows = 3;    // ginfo row y carries the mask bits of row y and the window counts of row y - 3

// Exact-stage tiles: one 256-thread workgroup per 8 rows.
constexpr int kWlogCap = 256;        // entries of a wave's log (a wave of the bench frames writes ~40)
constexpr int kTileRows = 8;
constexpr int kExactListCap = 2048;  // candidate entries staged in LDS per flush

struct ThresholdArgs {
    const void* image;         // device pixels
    uint64_t frame_stride;     // bytes
    uint32_t pitch;            // bytes
    // The neighbour limit, exclusive (ffs_ctx_set_max_valid_scope): a pixel p >= nb_limit is left out of the
    // count and the sums of every window.  Centre scope: 2^24, the oracle's rule for 32-bit pixels (standalone.cc:78,90), and no kernel
    // of 16-bit pixels reads it.  Window scope with max_valid >= 0: min(max_valid, 2^24 - 1) + 1 (16-bit pixels: at most 65536), read
    // by the general-window kernel, k_ext_first, and the gathered predicates' instantiations that carry the compare (threshold_route.hpp).  (It fills the four bytes
    // of padding between `pitch` and `maskbits`.)
    uint32_t nb_limit;
    const uint8_t* maskbits;   // valid-pixel bit plane [H][mpitch]
    uint8_t* bits;             // candidate / strong bit planes [n][H][mpitch]
    uint8_t* strong_bytes;     // byte masks [n][H][bpitch]
    uint32_t* tile_counts;     // [n][n_tiles] strong pixels per exact-stage tile
    int W, H, pitch_px;
    uint32_t mpitch, bpitch;
    uint64_t plane_frame_stride, bytes_frame_stride;
    int n_strips, band_rows, n_bands, n_tiles;
    // Bands of two heights (tuning "band_taper"): bands 0 .. band_split - 1 are band_rows tall, the rest band_rows2.  The block map
    // hands out bands in ascending order, so with band_rows2 < band_rows the LAST waves of a launch are the short ones and the
    // launch's tail (the slots of the machine that idle while the last round of waves finishes) shrinks.  band_split = n_bands: uniform.
    int band_rows2, band_split;
    // parameters
    float kS;                  // nsig_s^2 (1 - 2^-16): conservative signal pre-filter
    float kB;                  // nsig_b (1 - 2^-20): conservative dispersion pre-filter
    int min_count;
    double nsig_b, nsig_s, threshold;
    double nsig_b2, nsig_s2;   // squares (float64), for the square-root-free form of the predicate
    long long max_valid;       // < 0: no test
    // integer form of the predicate (kernels_stream.hpp: int_predicate): usable when nsig_b^2 and nsig_s^2 are integers
    int int_pred;              // 1: ib2 / is2 / thr_floor are valid
    uint32_t ib2, is2;         // nsig_b^2, nsig_s^2
    uint32_t thr_floor;        // floor(threshold): for an integer pixel p, p > threshold <=> p > floor(threshold)
    int bright_to_plane;       // streaming kernels: 0 = bright windows go onto bright_list (k_bright_fix decides them);
                               // 1 = they are marked in the plane as candidates and the exact kernel filters the plane;
                               // 2 (host side only) = the plane starts as the valid-pixel mask and the exact kernel decides every pixel
    // extended dispersion (kernels_extended.hpp)
    uint8_t* dplane;           // first-pass "not background" bit planes [n][H][mpitch]
    uint8_t* eplane;           // eroded signal-region bit planes [n][H][mpitch]
    int eplane_clean;          // the signal-region plane is all zero (cleared behind the previous batch): the erosion stores its non-zero words only
    int ext_strips, ext_band_rows, ext_bands;
    int ext_flavour;           // 0 = baseline.cpp rules, 1 = device-kernel rules
    int ext_variant;           // first pass, 16-bit pixels: 2 = streaming kernel (k_stream_u16<true>), 0 = k_ext_first (host side only: ThresholdRoute)
    // one-kernel threshold for 16-bit pixels (kernels_stream.hpp)
    const uint8_t* ginfo;      // [H + 3][gpitch] one dword per 8-pixel group: mask bits | min count << 8 | max count << 16
    const uint8_t* mmap;       // [H][pitch_px] 7x7 window count of every pixel
    uint32_t gpitch;           // bytes per ginfo row = pitch_px / 2
    int gpf;                   // lane groups per frame row = ceil(W / 8)
    int n_frames;              // frames of this launch
    int group_frames;          // frames laid side by side in one super row (group bytes < 2 GiB)
    uint32_t* bright_n;        // [1] pixels handed to k_bright_fix (window sum >= 65536)
    uint2* bright_list;        // [bright_cap] (frame << 16 | x, y)
    uint32_t bright_cap;
    uint32_t* overflow;        // status word: kOvfBrightList when the bright-window list overflowed
    // occupancy of the strong plane, one bit per 16-byte segment (128 pixels) of a plane row: set by whoever sets a plane
    // bit in a one-kernel batch, read and cleared by k_frame_chain, which then loads only the segments that hold something
    uint32_t* occ;             // [n][occ_frame_words]
    uint32_t occ_frame_words;  // words per frame = ceil(H * occ_spr / 32)
    uint32_t occ_spr;          // segments per plane row = mpitch / 16
    int dense_mask;            // the streaming kernels zero-fill the byte mask (somebody wants it); else they leave it alone
    // wave logs (tuning "strong_log", 16-bit standard path): instead of scattering plane bytes, counter and occupancy atomics
    // and bright-list entries over the stream's buffers, every wave appends one 8-byte entry per group that holds a strong
    // (or undecided) pixel to its own log -- dense stores; kernels_chain.hpp merges the logs of a frame
    uint2* wlog;               // [waves][kWlogCap] (row << 16 | group, frame in super row << 16 | undecided << 8 | strong); nullptr: off
    uint32_t* wlog_n;          // [waves] entries a wave wanted to write (more than kWlogCap: overflow)
    uint4* wpix;               // [waves][kWlogCap] the entry's eight (masked) pixels: the sparse launch never gathers from the image
    // hand-over to the next streaming kernel (ffs_submit.hip, tuning "dense_overlap"): the launch's LAST workgroup -- dispatch is in
    // order -- writes handoff_seq here as it starts; the other dense HIP stream waits for that value before ITS kernel, which then
    // flows into the slots this launch's last round of waves leaves.  nullptr: off.
    uint32_t* handoff;
    uint32_t handoff_seq;
    int dbg_prio;              // tuning "stream_prio": the 16-bit streaming kernel raises its waves' issue priority (s_setprio 3)
    int dbg;                   // timing experiments (-DFFS_EXPERIMENTS builds only; results are wrong when set)
    // the window (ffs_params.kernel_half_x / _y, 1..7): the general-window kernel (kernels_window.hpp) and k_exact's runtime-window
    // gather (exact_strong_w); the 7x7 kernels above have it built in
    int kx, ky;
    int w_strips, w_band_rows, w_bands;   // general-window kernel: a wave per (strip of 62 eight-pixel groups, band of rows, frame)
    float w_kS, w_kB;          // its float32 screens: nsig_s^2 (1 - 2^-16), nsig_b^2 (1 - 2^-16); 0 = screen off
                               // (a gain batch: w_kS carries the gain, gain nsig_s^2 (1 - 2^-16) -- DESIGN.md section 3.3d)
    // the detector gain (ffs_ctx_set_gain): 0 = off; > 0 = the gain instantiations decide with the variance
    // gain * mean (baseline.cpp:241-247, :539-543, :709-715).  No other kernel reads these.
    double gain;
    float g_gain, g_nb;        // float32 screen of a > c under gain: (float)gain and (float)nsig_b; g_gain = 0 = screen off
    // the per-pixel gain map (ffs_ctx_set_gain_map): float32 rows of pitch_px entries, gm_pitch bytes apart; only the
    // kGainMap instantiations read it, each pixel's decision with the entry of its CENTRE (baseline.cpp:244-245, :541, :714).  Such a batch
    // has gain = 0, w_kS without a gain inside (the kernel multiplies by the pixel's) and g_gain unused; g_nb = 0 = nsig_b outside the screen's range.
    const float* gain_map;
    uint32_t gm_pitch;
    // the runs of rows the mask leaves without a valid pixel (launch_geometry.hpp: empty_runs_of, built with the mask tables): the waves of
    // the streaming kernels trim them off their band's two ends (trim_band).  By value, so a launch carries the runs of the mask its
    // tables were built from.
    EmptyRuns empty_runs;
};
// the gain-map entry of pixel (x, y), 0 <= x < pitch_px
__device__ __forceinline__ float gain_at(const ThresholdArgs& a, int x, int y) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(a.gain_map) + (uint64_t)y * a.gm_pitch + (uint64_t)x * 4u);
}

// The streaming launch's units (launch_geometry.hpp has the map: stream_unit_of, log_slot_of), for the arguments of a launch
__host__ __device__ inline uint32_t stream_units(const ThresholdArgs& a) { return stream_units_of(a.n_bands, a.n_strips); }
__host__ __device__ inline uint32_t stream_chunk(const ThresholdArgs& a) { return stream_chunk_of(a.n_bands, a.n_strips); }   // units per XCD; grid.x = 8 chunks
__device__ __forceinline__ bool stream_unit(const ThresholdArgs& a, uint32_t bid, int& strip, int& band) {
    return stream_unit_of(bid, a.n_bands, a.n_strips, strip, band);
}
// where the log of (super row y, band, strip) lies in wlog / wlog_n / wpix
__host__ __device__ inline uint32_t log_slot(const ThresholdArgs& a, uint32_t y, uint32_t band, uint32_t strip) {
    return log_slot_of(a.n_bands, a.n_strips, y, band, strip);
}

// ---- what a batch tells the host when a plan did not hold it: the overflow flags -----------------------------------------
// Bits of a batch's status word (the block's status word, or a frame's flag word when the sparse stage was one launch per frame).
// ffs_wait.hip (decide_recovery) has their precedence; DESIGN.md section 3.4d has the table.
constexpr uint32_t kOvfStrongCap = 1u;    // a frame holds more strong pixels than `cap` (compaction, one-launch stages' tail): that frame again on a one-frame stream
constexpr uint32_t kOvfCompCap = 2u;      // a frame holds more components than `max_comp` (k_finalize_roots, one-launch stages' tail): that frame again on a one-frame stream
constexpr uint32_t kOvfCorruptLz4 = 4u;   // an LZ4 block did not decode to its block size (kernels_decode.hpp): the wait fails, FFS_ERR_INVALID
constexpr uint32_t kOvfBrightList = 8u;   // the bright-window list overflowed (k_bright_fix, k_frame_chain phase B): the batch again, threshold path 1
constexpr uint32_t kOvfRuns = 16u;        // a frame's runs are beyond the one launch's LDS (k_frame_chain<RUNS>): the batch again through the grid-wide kernels, and so the stream's later dense batches
constexpr uint32_t kOvfWaveLog = 32u;     // a wave log or the list of undecided pixels overflowed (k_frame_chain<LOG>, k_band_cc): the batch again through the plane, and the stream stays with it
constexpr uint32_t kOvfLdsForest = 64u;   // a frame beyond the LDS forest met on the log path (k_frame_chain<LOG>): this batch again through the plane
constexpr uint32_t kOvfBandPlan = 128u;   // a band beyond the band stage's plan (k_band_cc, k_frame_merge): the batch again through k_frame_chain, bands off for 32 batches
constexpr uint32_t kOvfCorruptByteOffset = 256u;   // a byte-offset chunk holds fewer than W * H elements (kernels_byteoffset.hpp): the wait fails, FFS_ERR_INVALID
// A different field, why a component is no reflection (kRecTooSmall, kRecTooSpread), is in sweep_plan.hpp, whose record classification reads it.

// ---- the counter block of a stream (B = max_batch) -------------------------------------------------------------------------
// [B] strong pixels | [B] components | [B][kSummaryWords] summary | [1] status word | [B] per-frame flag words, as 32-bit words.
// The device block ends behind the status word (one copy brings it back); the pinned host block also has the per-frame flag
// words, which the one-launch sparse stages write themselves -- such a batch's status is their OR (ffs_wait.hip: batch_overflow).
constexpr int kSummaryWords = 8;
constexpr uint32_t kSumBoxes = 0, kSumStrongFiltered = 1, kSumReflections = 2, kSumFilteredSize = 3, kSumFilteredSep = 4;   // slots of a frame's summary
__host__ __device__ constexpr size_t counts_strong_at(size_t) { return 0; }
__host__ __device__ constexpr size_t counts_comp_at(size_t B) { return B; }
__host__ __device__ constexpr size_t counts_summary_at(size_t B) { return 2 * B; }
__host__ __device__ constexpr size_t counts_status_at(size_t B) { return (2 + kSummaryWords) * B; }
__host__ __device__ constexpr size_t counts_frame_flags_at(size_t B) { return counts_status_at(B) + 1; }
__host__ __device__ constexpr size_t counts_device_words(size_t B) { return counts_status_at(B) + 1; }
__host__ __device__ constexpr size_t counts_host_words(size_t B) { return counts_frame_flags_at(B) + B; }

// ---- strong-pixel lists and connected components -------------------------------------------------
// 2D only (round 2): the accumulator of a component sits at the list index of its ROOT (its smallest
// member, always the first pixel of a horizontal run), so no pass has to number the components before
// they can be reduced.  k_emit_list_w resets the accumulator of every run start.
struct CompAcc2 {
    unsigned long long sum_i, sum_xi, sum_yi, peak;
    uint32_t x_min, x_max, y_min, y_max;
    uint32_t num_pixels, pad;
};

// 2D record as it crosses PCIe (40 bytes instead of the 56 of ffs_reflection: the z fields are constants
// for a single frame and the coordinates fit 16 bits); ffs_wait() widens it again.
struct WireRec2 {
    uint16_t x_min, x_max, y_min, y_max;
    uint32_t npx_flags;        // num_pixels | flags << 30
    float com_x, com_y;
    uint16_t peak_x, peak_y;
    uint32_t peak_intensity;
    float peak_centroid_distance;
    unsigned long long sum_intensity;
};

struct CclArgs {
    const void* image;
    uint64_t frame_stride;
    uint32_t pitch;
    uint8_t* bits;             // strong bit planes
    int clear_bits;            // clear every plane word after reading it (k_stream_u16 needs an all-zero plane)
    const uint32_t* tile_counts;
    uint32_t* num_strong;      // [n]
    uint32_t* row_off;         // [n][H+1] list offset of the first strong pixel of each image row
    uint32_t* list_k;          // [n][cap] ascending linear index y*W + x
    uint32_t* list_i;          // [n][cap] intensity
    uint32_t* parent;          // [n][cap]
    uint32_t* comp_id;         // [n][cap] component number of each ROOT entry
    uint32_t* n_comp;          // [n]
    uint32_t* overflow;        // [1] status word: kOvfStrongCap / kOvfCompCap when a frame exceeded cap / max_comp
    int W, H, pitch_px;
    uint32_t mpitch;
    uint64_t plane_frame_stride;
    int n_tiles;
    uint32_t cap;              // list capacity per frame
    uint32_t max_comp;         // record capacity per frame
    int pixel_bytes;
    CompAcc2* acc2;            // [n][cap] or null: reset the accumulator of every run start (k_reduce_roots)
    uint32_t* summary;         // [n][8]: with acc2, the compaction zeroes n_comp and summary (the root-indexed kernels add into them)
    uint8_t* strong_bytes;     // byte masks [n][H][bpitch]: the compaction sets the 1s (the threshold kernels zero-fill)
    uint32_t bpitch;
    uint64_t bytes_frame_stride;
    int dense_bytes;           // write the byte mask at all (only when somebody asked for it)
    int need_lists;            // the strong-pixel lists (k, intensity) have a reader after the launch (host copy, 3D stack); 0: the launch that
                               // merges wave logs keeps them to itself (1.15 M scattered 4-byte stores per batch less)
    uint32_t* occ;             // see ThresholdArgs; null or use_occ == 0: the whole plane is read
    uint32_t occ_frame_words, occ_spr;
    int use_occ;
};

// Per-component accumulator (device) -- reduced with 64-bit integer atomics so the result
// is independent of arrival order (the reference's double sums of half-integer * integer
// terms are exact, connected_components.hpp:86-90, so integer sums reproduce them bit for bit).
struct CompAcc {
    unsigned long long sum_i;    // sum I
    unsigned long long sum_xi;   // sum (2x+1) I
    unsigned long long sum_yi;   // sum (2y+1) I
    unsigned long long sum_zi;   // sum (2z+1) I
    unsigned long long peak;     // (I << 32) | ~(position rank): max => highest I, then smallest (z,y,x)
    uint32_t x_min, x_max, y_min, y_max;
    int32_t z_min, z_max;
    uint32_t num_pixels;
    uint32_t root;               // list index of the minimum vertex (label order key)
};

// A segment is one independent labelling problem: a frame (2D) or a whole z-stack (3D).
struct SegArgs {
    const uint32_t* list_k;   // per segment: ascending (z, k)
    const uint32_t* list_i;
    uint32_t* parent;
    uint32_t* comp_id;        // 3D only: component number of each root entry
    const uint32_t* seg_n;    // [n_seg] entries per segment
    uint64_t seg_stride;      // entries between segment starts
    uint32_t* n_comp;         // [n_seg]
    CompAcc* acc;             // [n_seg][max_comp]
    uint32_t max_comp;
    uint32_t* overflow;
    uint32_t W, H;
    const uint32_t* row_off;  // 2D only: [n_seg][H+1] per-row list offsets (may be null)
    // 3D only
    const uint32_t* slice_begin;  // [n_slices + 1] entry offsets of each slice inside the segment
    int n_slices;
    const uint32_t* zs;           // slice of every entry (k_stack_gather), or null
    // finalize
    uint32_t min_spot_size;
    float max_sep;
    void* recs;               // ffs_reflection, packed: segment s starts at sum_{q<s} n_comp[q]
    uint32_t* summary;        // [n_seg][8]: n_boxes, n_strong_filtered, n_refl, n_filt_size, n_filt_sep
    // 2D, accumulators at the root (k_reduce_roots / k_finalize_roots)
    CompAcc2* acc2;           // [n_seg][seg_stride]
    uint32_t* chunk_roots;    // [n_seg][chunks_max] roots per chunk of kRootChunk list entries
    uint32_t chunks_max;
    // 2D: the compaction has consumed the per-tile counts; k_union zeroes them (and the bright-list count) again, which
    // is what the next batch's streaming kernel adds into
    uint32_t* zero_counts;    // [n_seg][zero_per_seg], or null
    uint32_t zero_per_seg;
    uint32_t* zero_word;      // one more word to clear, or null
};

// (StackSlice, one row of the 3D stack's copy tables, is in sweep_plan.hpp, which has no HIP in it and fills them)

// Matches ffs_reflection in include/ffs_hip.h
struct ReflOut {
    uint32_t x_min, x_max, y_min, y_max;
    int32_t z_min, z_max;
    int32_t num_pixels;
    float com_x, com_y, com_z;
    uint32_t peak_x, peak_y;
    int32_t peak_z;
    uint32_t peak_intensity;
    float peak_centroid_distance;
    uint32_t flags;
    unsigned long long sum_intensity;
};

// Inclusive prefix sum over the 64 lanes in six DPP adds (row_shr 1/2/4/8 inside the rows of 16, then row_bcast:15 and
// row_bcast:31 carry the row totals on) instead of six ds_bpermute round trips.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2 and 3
    return v;
}

// Pixel j of the 16 bytes a lane loaded: PX = 8 pixels of 16 bits or 4 of 32
template <int PX>
__device__ __forceinline__ uint32_t lane_pixel(const uint4& v, int j) {
    if constexpr (PX == 8) {
        const uint32_t w = j < 2 ? v.x : j < 4 ? v.y : j < 6 ? v.z : v.w;
        return (j & 1) ? w >> 16 : w & 0xFFFFu;
    } else {
        return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
    }
}

}  // namespace ffsamd
