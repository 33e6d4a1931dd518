// launch_geometry.hpp -- the launch geometry of the threshold stage as plain integer arithmetic: the frame layout, how the streaming
// kernels cut a batch into super rows, strips and bands, the general-window kernel's and the extended first pass's strips and bands,
// how many wave logs and band slots a launch needs, the unit map the kernels invert, and the row bands and the pixel-count rule of the
// per-frame products.  No HIP header: host code, the kernels (through ffs_device.h) and a plain C++ test program
// (tests/launch_geometry_check.cc) compile the same text.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <utility>

#include "tuning.hpp"

#if defined(__HIPCC__)
#define FFS_HD __host__ __device__
#else
#define FFS_HD
#endif

namespace ffsamd {

// ---- frame layout in HBM ---------------------------------------------------------------------
// Pixels:      [frame][y][pitch_px] of PixelT, rows `pitch` bytes apart (multiple of 128 B).
// Bit planes:  [frame][y][mpitch] bytes, 1 bit per pixel, LSB first (bit x&7 of byte x>>3);
//              bits for x >= W are always 0.  Used for: valid-pixel mask (one plane per
//              context, frame-invariant), candidate plane, strong plane (candidate plane
//              filtered in place).
// Byte mask:   [frame][y][bpitch] bytes 0/1 -- the reference kernel's result_strong layout
//              (spotfinder/kernels/thresholding.cu:233), kept as the drop-in contract.
struct Layout {
    int W, H;
    int pitch_px;        // multiple of 64, >= W
    uint32_t pitch;      // bytes per pixel row (default layout)
    uint32_t mpitch;     // bytes per bit-plane row  = pitch_px / 8
    uint32_t bpitch;     // bytes per byte-mask row  = pitch_px
    uint64_t frame_stride;       // bytes between frames (default layout)
    uint64_t plane_frame_stride; // bytes between frames of a bit plane = H * mpitch
    uint64_t bytes_frame_stride; // bytes between frames of the byte mask = H * bpitch
};
inline Layout default_layout(uint32_t width, uint32_t height, int pixel_bytes) {
    Layout L{};
    L.W = (int)width;
    L.H = (int)height;
    L.pitch_px = ((int)width + 127) / 128 * 128;  // byte-mask rows start on 128-byte lines
    L.pitch = (uint32_t)L.pitch_px * (uint32_t)pixel_bytes;
    L.mpitch = (uint32_t)L.pitch_px / 8;
    L.bpitch = (uint32_t)L.pitch_px;
    L.frame_stride = (uint64_t)L.pitch * height;
    L.plane_frame_stride = (uint64_t)L.mpitch * height;
    L.bytes_frame_stride = (uint64_t)L.bpitch * height;
    return L;
}
// the mask tables of the streaming kernels (ThresholdArgs::ginfo): one dword per lane group of 16 bytes of pixels -- 8 pixels
// (16-bit) or 4 pixels (32-bit)
inline uint32_t ginfo_pitch(const Layout& L, int pixel_bytes) { return (uint32_t)L.pitch_px * (uint32_t)pixel_bytes / 4; }   // bytes per ginfo row
inline int groups_per_row(const Layout& L, int pixel_bytes) { return pixel_bytes == 2 ? (L.W + 7) / 8 : (L.W + 3) / 4; }       // lane groups per frame row

// ---- the constants the geometry and the kernels share ---------------------------------------------------------------
// Streaming threshold kernels (kernels_stream.hpp): one wave64 marches down a column strip; a lane holds 16 bytes of a pixel row
// (8 pixels of 16 bits, 4 of 32).  Lanes 0 and 63 are halo (their windows are incomplete), lanes 1..62 own output.
constexpr int kSOwned = 62;
// General-window kernel (kernels_window.hpp): a lane holds one eight-pixel group (16 / 32 bytes) of a row; lanes 1..62 own output
constexpr int kWinOwned = 62;
// Extended first pass, one pixel per lane (kernels_extended.hpp)
constexpr int kExtOwnedPx = 56;    // lanes 4..59 of a wave own output
// The sparse stage in small workgroups (kernels_band.hpp): the LDS plan a launch geometry has to fit
constexpr int kBandMaxRows = 128;       // rows of a band (the streaming kernel's geometry: 72-80 for Eiger frames)
constexpr int kBandCw = 1024;           // (row, strip) counters: rows * strips of the frame
constexpr int kMergeMaxBands = 128;
constexpr int kBandSplitRows = 96;      // a streaming band taller than this is cut into sub-bands of equal height, a wave each

// ---- streaming kernels ----------------------------------------------------------------------------------------------
// Bands of two heights (tuning "band_taper"): bands 0 .. band_split - 1 are band_rows tall, the rest band_rows2 (ThresholdArgs has
// the why).  band_split = n_bands: uniform.
struct StreamGeometry {
    int group_frames;   // frames laid side by side in one super row (group bytes < 2 GiB)
    int n_groups;       // super rows of the launch: grid.y
    int n_strips, n_bands;
    int band_rows, band_rows2, band_split;
};
inline StreamGeometry stream_geometry(const Layout& L, int pixel_bytes, uint64_t frame_stride, uint32_t n_frames, const Tuning& tune) {
    StreamGeometry a{};
    const int gpf = groups_per_row(L, pixel_bytes);
    {   // Streaming kernels: frames side by side in one super row, as many as keep every buffer of the group below 2 GiB.
        // Bands: enough waves to fill the 256 CUs several times over, bands no shorter than 72 rows (the 6-row warm-up of
        // every band stays below 8 %).  The default stays a multiple of eight bands (what rounds 1-4's round-robin map, band = xcd + 8 k,
        // needed: with 29 bands three XCDs had a band less to do than the others, 511 us per 32 Eiger frames against 430-440 with 48
        // or 56); the unit map of round 5 (stream_unit_of, below) balances any number -- tuning "stream_bands".
        const uint64_t per_frame = std::max<uint64_t>(frame_stride, L.bytes_frame_stride);
        a.group_frames = (int)std::max<uint64_t>(1, std::min<uint64_t>(n_frames, ((1ull << 31) - 1) / per_frame));
        a.group_frames = std::min(a.group_frames, tune.frames_per_group);
        a.n_groups = ((int)n_frames + a.group_frames - 1) / a.group_frames;
        const long long lanes = (long long)a.group_frames * (gpf + 1);
        const long long lines = (long long)a.group_frames * (L.bpitch / 128);  // byte-mask lines to zero per row
        const int lines_per_wave = pixel_bytes == 2 ? 4 : 2;  // a wave zero-fills 512 / 256 bytes of the byte mask per row
        a.n_strips = (int)std::max<long long>((lanes + kSOwned - 1) / kSOwned, (lines + lines_per_wave - 1) / lines_per_wave);
        const long long per_band = std::max<long long>(1, (long long)a.n_strips * a.n_groups);
        long long nb = std::max<long long>(1, std::min<long long>(tune.target_waves / per_band, L.H / 72));
        if (nb >= 8) nb = nb / 8 * 8;
        // tuning "stream_bands" > 0: that many bands (any number: the unit map balances the XCDs)
        if (tune.stream_bands > 0) nb = std::max<long long>(1, std::min<long long>(tune.stream_bands, L.H / 8));
        a.band_rows = (int)std::min<long long>(1024, (L.H + nb - 1) / nb);
        a.n_bands = (L.H + a.band_rows - 1) / a.band_rows;
        a.band_rows2 = a.band_rows;
        a.band_split = a.n_bands;
        // Tapered bands (tuning "band_taper" = t per cent, 0 = off): the last two bands of every XCD are t % as tall as the others.
        // The waves of a launch all take about the same time and there are 3-4 times as many of them as the machine has slots, so
        // the last round leaves slots idle; handed out last and short, the final waves fill that tail with less work each.
        const int taper = tune.band_taper;
        if (taper > 0 && taper < 100 && nb >= 32 && nb % 8 == 0 && a.n_bands == (int)nb) {
            const int K = (int)nb / 8;                       // bands per XCD
            const int K2 = 2, K1 = K - K2;
            // 8 (K1 h1 + K2 h2) >= H with h2 = taper h1 / 100
            const double h1f = (double)L.H / (8.0 * (K1 + K2 * taper / 100.0));
            int h1 = std::min(1024, (int)std::ceil(h1f));
            int h2 = (int)std::ceil((L.H / 8.0 - (double)K1 * h1) / K2);
            while (h2 < 24) { --h1; h2 = (int)std::ceil((L.H / 8.0 - (double)K1 * h1) / K2); }
            if (h1 >= h2 && h2 >= 24 && 8 * (K1 * h1 + K2 * h2) >= L.H && 8 * K1 * h1 < L.H) {
                a.band_rows = h1;
                a.band_rows2 = h2;
                a.band_split = 8 * K1;
                a.n_bands = a.band_split + (L.H - a.band_split * h1 + h2 - 1) / h2;
            }
        }
    }
    return a;
}
// strips a frame's groups can touch (a frame's groups start anywhere in a strip of the super row)
inline uint32_t strips_per_frame(const Layout& L, int pixel_bytes) { return (uint32_t)groups_per_row(L, pixel_bytes) / (uint32_t)kSOwned + 2u; }
// logs of a launch: one per (super row, band, strip) -- log_slot_of()
inline size_t stream_log_slots(const StreamGeometry& g) { return (size_t)g.n_groups * (size_t)g.n_bands * (size_t)g.n_strips; }
// ... and of the largest launch any batch of 1 .. max_batch frames can make: what the wave logs of a stream are sized for
inline size_t max_stream_log_slots(const Layout& L, int pixel_bytes, uint64_t frame_stride, uint32_t max_batch, const Tuning& tune) {
    size_t slots = 0;
    for (uint32_t nf = 1; nf <= max_batch; ++nf) slots = std::max(slots, stream_log_slots(stream_geometry(L, pixel_bytes, frame_stride, nf, tune)));
    return slots;
}

// The sparse stage in small workgroups (kernels_band.hpp): a band of the streaming launch as `sub` bands of the sparse stage, each of
// at most sub_rows rows
struct BandSplit { int sub = 1, sub_rows = 0; };
inline BandSplit band_split(const StreamGeometry& g) {
    const int rows = std::max(g.band_rows, g.band_rows2), sub = (rows + kBandSplitRows - 1) / kBandSplitRows;
    return {sub, (rows + sub - 1) / sub};
}
// ... whose LDS plan holds this launch geometry
inline bool band_plan_holds(const StreamGeometry& g, const Layout& L, int pixel_bytes) {
    const uint32_t strips = strips_per_frame(L, pixel_bytes);
    const BandSplit split = band_split(g);
    const int sub = split.sub, sub_rows = split.sub_rows;
    return !(sub_rows > kBandMaxRows || (uint32_t)sub_rows * std::min(strips, 16u) > (uint32_t)kBandCw || g.n_bands * sub > kMergeMaxBands || L.W > 65535);
}
// (frame, band) pairs of a launch of n_frames frames, and of the largest any batch of 1 .. max_batch frames can make
inline uint32_t band_slots(const StreamGeometry& g, uint32_t n_frames) { return n_frames * (uint32_t)(g.n_bands * band_split(g).sub); }
inline uint32_t max_band_slots(const Layout& L, int pixel_bytes, uint64_t frame_stride, uint32_t max_batch, const Tuning& tune) {
    uint32_t slots = 0;
    for (uint32_t nf = 1; nf <= max_batch; ++nf) slots = std::max(slots, band_slots(stream_geometry(L, pixel_bytes, frame_stride, nf, tune), nf));
    return slots;
}

// ---- general-window kernel ------------------------------------------------------------------------------------------
struct WindowGeometry { int w_strips, w_band_rows, w_bands; };   // a wave per (strip of 62 eight-pixel groups, band of rows, frame)
inline WindowGeometry window_geometry(const Layout& L, uint32_t n_frames, int ky) {
    WindowGeometry a{};
    {   // the general-window kernel: strips of 62 owned eight-pixel groups; bands at least 6 windows tall (the 2ky + 1 warm-up rows
        // of a band stay below a sixth of its rows), as many as fill the machine about four times over
        const int g8 = (L.W + 7) / 8;
        a.w_strips = (g8 + kWinOwned - 1) / kWinOwned;
        const long long per_band = std::max<long long>(1, (long long)a.w_strips * n_frames);
        const int min_rows = std::max(32, 6 * (2 * ky + 1));
        const long long nb = std::max<long long>(1, std::min<long long>(16384 / per_band, std::max(1, L.H / min_rows)));
        a.w_band_rows = (int)((L.H + nb - 1) / nb + 7) / 8 * 8;
        a.w_bands = (L.H + a.w_band_rows - 1) / a.w_band_rows;
    }
    return a;
}

// ---- extended dispersion, first pass (k_ext_first) --------------------------------------------------------------------
struct ExtGeometry { int ext_strips, ext_band_rows, ext_bands; };
inline ExtGeometry ext_geometry(const Layout& L, uint32_t n_frames) {
    ExtGeometry a{};
    a.ext_strips = (L.pitch_px + kExtOwnedPx - 1) / kExtOwnedPx;
    {   // one pixel per lane: bands of 64..256 rows keep the 6-row warm-up below 10 %
        const long long ext_target = 8192;
        long long er = ((long long)L.H * a.ext_strips * n_frames + 4 * ext_target - 1) / (4 * ext_target);
        er = std::max<long long>(64, std::min<long long>(er, 256));
        a.ext_band_rows = (int)er;
        a.ext_bands = (L.H + a.ext_band_rows - 1) / a.ext_band_rows;
    }
    return a;
}

// ---- per-frame products: bands of contiguous rows, a workgroup each (k_radial, k_radthr_hist) ---------------------------
// About target_groups workgroups a launch and at most max_bands bands a frame, all of band_rows rows but the last; forced > 0: that many
// bands instead, clamped to 1..H (0: the launch chooses).
inline void uniform_row_bands(int H, uint32_t n_frames, uint32_t target_groups, uint32_t max_bands, int forced, uint32_t& n_bands, uint32_t& band_rows) {
    const uint32_t h = (uint32_t)H;
    const uint32_t want = forced > 0 ? std::clamp<uint32_t>((uint32_t)forced, 1u, h)
                                     : std::clamp<uint32_t>((target_groups + n_frames - 1) / n_frames, 1u, std::min(h, max_bands));
    band_rows = (h + want - 1) / want;
    n_bands = (h + band_rows - 1) / band_rows;
}
// (frame, band) pairs of the largest launch any batch of 1 .. max_batch frames can make where the launch chooses its bands
inline size_t max_uniform_band_slots(int H, uint32_t max_batch, uint32_t target_groups, uint32_t max_bands) {
    size_t slots = 0;
    for (uint32_t nf = 1; nf <= max_batch; ++nf) {
        uint32_t nb = 0, rows = 0;
        uniform_row_bands(H, nf, target_groups, max_bands, 0, nb, rows);
        slots = std::max(slots, (size_t)nf * nb);
    }
    return slots;
}
// The pixel-count rule of the per-frame products, the per-spot background and the window scope's neighbour limit: a pixel counts when
// p < counting_limit.  max_valid (>= 0) is inclusive and holds under both of its scopes; on top of it, and alone without a max_valid,
// stands the oracle's p < 2^24 for 32-bit pixels (16-bit pixels never reach it).
inline uint32_t counting_limit(long long max_valid) {
    return max_valid >= 0 ? (uint32_t)std::min<long long>(max_valid, (1ll << 24) - 1) + 1u : 1u << 24;
}

// ---- the unit map: what the kernels invert ----------------------------------------------------------------------------
// first row of band b for a (split, rows, rows2) geometry -- see ThresholdArgs::band_split
FFS_HD inline int band_first_row(int band, int band_rows, int band_rows2, int band_split) {
    return band < band_split ? band * band_rows : band_split * band_rows + (band - band_split) * band_rows2;
}
// The streaming launch's units.  A unit = one wave = one band of one strip; units are numbered band after band (u = band * n_strips +
// strip) and dealt to the eight XCDs in eight contiguous chunks (workgroup b runs on XCD b % 8): the strips of a band -- neighbours that
// share halo columns and, frame after frame, the same rows of the mask tables -- share an L2, and ANY number of bands is balanced over
// the XCDs.  (Rounds 1-5 dealt the bands round-robin, band = xcd + 8 k, which wanted a multiple of eight bands; the chunks measure
// 0.5-1 % faster on the same box, profiles/r06e_map_variants.log.)
FFS_HD inline uint32_t stream_units_of(int n_bands, int n_strips) { return (uint32_t)n_bands * (uint32_t)n_strips; }
FFS_HD inline uint32_t stream_chunk_of(int n_bands, int n_strips) { return (stream_units_of(n_bands, n_strips) + 7u) / 8u; }   // units per XCD; grid.x = 8 chunks
FFS_HD inline bool stream_unit_of(uint32_t bid, int n_bands, int n_strips, int& strip, int& band) {
    const uint32_t u = (bid & 7u) * stream_chunk_of(n_bands, n_strips) + (bid >> 3);
    band = (int)(u / (uint32_t)n_strips);
    strip = (int)(u - (uint32_t)band * (uint32_t)n_strips);
    return u < stream_units_of(n_bands, n_strips);
}
// where the log of (super row y, band, strip) lies in wlog / wlog_n / wpix: the strips of a band side by side
FFS_HD inline uint32_t log_slot_of(int n_bands, int n_strips, uint32_t y, uint32_t band, uint32_t strip) {
    return (y * (uint32_t)n_bands + band) * (uint32_t)n_strips + strip;
}

// ---- the rows a mask leaves empty: what a streaming wave trims off its band's two ends ----------------------------------
// A row without a valid pixel has no strong pixel (a masked centre never passes the predicate), and to the windows of its neighbours
// it is a row of zeros whether it is loaded or not.  A wave of the streaming kernels therefore starts at its band's first row WITH a
// valid pixel and stops behind the last one: the geometry above -- bands, grid, log slots -- stays what it
// is, the wave only runs fewer rows.  The runs travel by value in the kernel arguments (ThresholdArgs::empty_runs), per launch.
constexpr int kEmptyRunSlots = 16;
struct EmptyRuns {
    uint32_t n;                          // runs kept
    uint16_t run[kEmptyRunSlots][2];     // (first row, end row), end exclusive; sorted by first row; the slots behind n are (0, 0), which cover nothing
};
// The kEmptyRunSlots longest maximal runs of rows with flags[y] == 0, sorted by first row.  Keeping
// fewer runs than the mask has is always correct: it only trims less.  Frames taller than the 16-bit rows hold: no runs.
inline EmptyRuns empty_runs_of(const uint8_t* flags, int H) {
    EmptyRuns r{};
    if (H > 65535) return r;
    for (int y = 0; y < H;) {
        if (flags[y]) { ++y; continue; }
        int end = y;
        while (end < H && !flags[end]) ++end;
        int at = (int)r.n;
        if (at == kEmptyRunSlots) {   // full: in place of the shortest kept run, where this one is longer
            at = 0;
            for (int k = 1; k < kEmptyRunSlots; ++k)
                if (r.run[k][1] - r.run[k][0] < r.run[at][1] - r.run[at][0]) at = k;
            if (end - y <= r.run[at][1] - r.run[at][0]) at = -1;
        } else {
            ++r.n;
        }
        if (at >= 0) { r.run[at][0] = (uint16_t)y; r.run[at][1] = (uint16_t)end; }
        y = end;
    }
    for (int i = 1; i < (int)r.n; ++i)   // by first row (insertion sort: at most 16 entries)
        for (int k = i; k > 0 && r.run[k][0] < r.run[k - 1][0]; --k) {
            std::swap(r.run[k][0], r.run[k - 1][0]);
            std::swap(r.run[k][1], r.run[k - 1][1]);
        }
    return r;
}
// Rows yb0 .. yb1 - 1 of a band without the kept runs that cover its first and its last row: [yb0', yb1') inside the band, every row
// of the band with a valid pixel inside it; a band without one gives yb0' == yb1'.  One pass each way: the runs are sorted, so a raised
// yb0 can only fall into a later run and a lowered yb1 into an earlier one.  Scalar arithmetic on 16 argument words, once per wave.
struct BandRows { int yb0, yb1; };
FFS_HD inline BandRows trim_band(const EmptyRuns& r, int yb0, int yb1) {
    if (yb0 >= yb1) return {yb0, yb1};
    int lo = yb0, hi = yb1;
    if (r.n != 0) {   // (a mask without an empty row -- most detectors' -- pays one compare)
        for (int k = 0; k < kEmptyRunSlots; ++k)
            if ((int)r.run[k][0] <= lo && lo < (int)r.run[k][1]) lo = (int)r.run[k][1];
        for (int k = kEmptyRunSlots - 1; k >= 0; --k)
            if ((int)r.run[k][0] < hi && hi <= (int)r.run[k][1]) hi = (int)r.run[k][0];
    }
    lo = lo < yb1 ? lo : yb1;
    hi = hi > lo ? hi : lo;
    return {lo, hi};
}

}  // namespace ffsamd
