// launch_geometry_check.cc -- the launch geometry (csrc/launch_geometry.hpp) without a GPU: built and run by tests/test_launch_geometry.py
// (g++ with the address and undefined-behaviour sanitizers, against that header alone).  Walks a sweep of frame shapes, pixel sizes, frame
// strides and tuning values; prints one line of geometry per case and batch size -- the test compares them with
// tests/golden/launch_geometry.json, recorded from the arithmetic as it stood inside make_threshold_args -- and checks on every case what
// the kernels and the buffer sizing rely on.  A line that starts with "FAIL" names a broken invariant; the exit status is then 1.
#include <climits>
#include <cstdio>
#include <vector>

#include "launch_geometry.hpp"

using namespace ffsamd;

static int g_failed = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            ++g_failed;                               \
            std::printf("FAIL %s: ", #cond);          \
            std::printf(__VA_ARGS__);                 \
            std::printf("\n");                        \
        }                                             \
    } while (0)

struct Shape { uint32_t W, H, max_batch; };
struct Tune { int frames_per_group; long long target_waves; int stream_bands, band_taper; };

// bands of `rows` rows each, the kernels' way (band b starts at b * rows, the last one ends at H): they tile 0 .. H-1
static void check_uniform_bands(const char* what, int H, int rows, int bands) {
    CHECK(rows >= 1 && bands >= 1 && (long long)(bands - 1) * rows < H && (long long)bands * rows >= H, "%s H %d rows %d bands %d", what, H, rows, bands);
}

static void check_stream(const Layout& L, int px, uint64_t fstride, uint32_t nf, const StreamGeometry& g) {
    // every band is 1..1024 rows, and the bands tile 0 .. H-1 exactly once
    int next = 0;
    for (int b = 0; b < g.n_bands; ++b) {
        const int y0 = band_first_row(b, g.band_rows, g.band_rows2, g.band_split);
        const int y1 = std::min(band_first_row(b + 1, g.band_rows, g.band_rows2, g.band_split), L.H);
        CHECK(y0 == next && y1 - y0 >= 1 && y1 - y0 <= 1024, "band %d of %d: rows %d..%d, expected start %d", b, g.n_bands, y0, y1, next);
        next = y1;
    }
    CHECK(next == L.H, "bands end at row %d of %d", next, L.H);
    // tapered bands: the conditions the search accepts a taper on (eight XCDs, two short bands each), or the uniform geometry
    const bool uniform = g.band_rows2 == g.band_rows && g.band_split == g.n_bands;
    if (!uniform) {
        const int h1 = g.band_rows, h2 = g.band_rows2;
        CHECK(g.band_split % 8 == 0 && h1 >= h2 && h2 >= 24 && g.band_split * h1 + 16 * h2 >= L.H && g.band_split * h1 < L.H,
              "taper: rows %d / %d, split %d, H %d", h1, h2, g.band_split, L.H);
    }
    // super rows: the groups hold the batch's frames, the last one at least one; every buffer of a group stays below 2^31 bytes
    CHECK(g.group_frames >= 1 && (long long)g.n_groups * g.group_frames >= (long long)nf && (long long)nf > (long long)(g.n_groups - 1) * g.group_frames,
          "%d groups of %d frames for %u frames", g.n_groups, g.group_frames, nf);
    const uint64_t largest = std::max<uint64_t>({fstride, L.frame_stride, L.plane_frame_stride, L.bytes_frame_stride});
    CHECK((uint64_t)g.group_frames * largest < (1ull << 31), "a group of %d frames of %llu bytes", g.group_frames, (unsigned long long)largest);
    // the strips cover the super row's lanes (a separator group behind every frame) and its byte-mask lines
    const long long lanes = (long long)g.group_frames * (groups_per_row(L, px) + 1), lines = (long long)g.group_frames * (L.bpitch / 128);
    CHECK((long long)g.n_strips * kSOwned >= lanes && (long long)g.n_strips * (px == 2 ? 4 : 2) >= lines, "%d strips for %lld lanes, %lld lines", g.n_strips, lanes, lines);
    // the unit map: the workgroups 0 .. 8 * chunk - 1 of a super row are every (band, strip) exactly once, the rest are not real
    const uint32_t units = (uint32_t)g.n_bands * (uint32_t)g.n_strips, chunk = stream_chunk_of(g.n_bands, g.n_strips);
    std::vector<uint8_t> seen(units, 0);
    uint32_t real = 0, twice = 0, outside = 0;
    for (uint32_t bid = 0; bid < 8u * chunk; ++bid) {
        int strip = -1, band = -1;
        if (!stream_unit_of(bid, g.n_bands, g.n_strips, strip, band)) continue;
        ++real;
        if (strip < 0 || strip >= g.n_strips || band < 0 || band >= g.n_bands) { ++outside; continue; }
        if (seen[(size_t)band * g.n_strips + strip]++) ++twice;
    }
    CHECK(8u * chunk >= units && real == units && twice == 0 && outside == 0, "unit map: %u units, %u real, %u twice, %u outside", units, real, twice, outside);
    // the logs: (super row, band, strip) -> slot is one to one onto 0 .. stream_log_slots - 1
    const size_t slots = stream_log_slots(g);
    std::vector<uint8_t> taken(slots, 0);
    size_t bad = 0;
    for (int y = 0; y < g.n_groups; ++y)
        for (int b = 0; b < g.n_bands; ++b)
            for (int k = 0; k < g.n_strips; ++k) {
                const uint32_t slot = log_slot_of(g.n_bands, g.n_strips, (uint32_t)y, (uint32_t)b, (uint32_t)k);
                if (slot >= slots || taken[slot]++) ++bad;
            }
    CHECK(slots == (size_t)g.n_groups * units && bad == 0, "log slots: %zu, %zu outside or taken twice", slots, bad);
}

static void stream_case(const Shape& sh, int px, uint64_t fstride, const Tune& t) {
    const Layout L = default_layout(sh.W, sh.H, px);
    if (fstride == 0) fstride = L.frame_stride;
    Tuning tune;
    tune.frames_per_group = t.frames_per_group;
    tune.target_waves = t.target_waves;
    tune.stream_bands = t.stream_bands;
    tune.band_taper = t.band_taper;
    size_t most_logs = 0;
    uint32_t most_bands = 0;
    for (uint32_t nf = 1; nf <= sh.max_batch; ++nf) {
        const StreamGeometry g = stream_geometry(L, px, fstride, nf, tune);
        const BandSplit split = band_split(g);
        std::printf("S %u %u %d %llu %d %lld %d %d %u | %d %d %d %d %d %d %d | %d %d %d\n", sh.W, sh.H, px, (unsigned long long)fstride, t.frames_per_group,
                    t.target_waves, t.stream_bands, t.band_taper, nf, g.group_frames, g.n_groups, g.n_strips, g.n_bands, g.band_rows, g.band_rows2,
                    g.band_split, split.sub, split.sub_rows, band_plan_holds(g, L, px) ? 1 : 0);
        check_stream(L, px, fstride, nf, g);
        CHECK(split.sub >= 1 && split.sub * split.sub_rows >= std::max(g.band_rows, g.band_rows2) && split.sub_rows <= kBandSplitRows, "sub-bands %d of %d rows", split.sub, split.sub_rows);
        most_logs = std::max(most_logs, stream_log_slots(g));
        most_bands = std::max(most_bands, band_slots(g, nf));
        CHECK(band_slots(g, nf) == nf * (uint32_t)g.n_bands * (uint32_t)split.sub, "band slots %u", band_slots(g, nf));
    }
    const size_t max_logs = max_stream_log_slots(L, px, fstride, sh.max_batch, tune);
    const uint32_t max_bands = max_band_slots(L, px, fstride, sh.max_batch, tune);
    CHECK(max_logs == most_logs && max_bands == most_bands, "sizing: logs %zu against %zu, band slots %u against %u", max_logs, most_logs, max_bands, most_bands);
    CHECK(strips_per_frame(L, px) == (uint32_t)groups_per_row(L, px) / 62u + 2u && ginfo_pitch(L, px) == L.pitch / 4, "strips per frame, ginfo pitch");
}

static void window_ext_case(const Shape& sh) {
    const Layout L = default_layout(sh.W, sh.H, 2);   // (neither geometry reads the pixel size)
    for (uint32_t nf = 1; nf <= sh.max_batch; ++nf) {
        for (int ky : {1, 3, 7}) {
            const WindowGeometry w = window_geometry(L, nf, ky);
            std::printf("W %u %u %d %u | %d %d %d\n", sh.W, sh.H, ky, nf, w.w_strips, w.w_band_rows, w.w_bands);
            check_uniform_bands("window", L.H, w.w_band_rows, w.w_bands);
            CHECK(w.w_strips * kWinOwned * 8 >= L.W && w.w_band_rows % 8 == 0, "window: %d strips, bands of %d rows", w.w_strips, w.w_band_rows);
        }
        const ExtGeometry e = ext_geometry(L, nf);
        std::printf("E %u %u %u | %d %d %d\n", sh.W, sh.H, nf, e.ext_strips, e.ext_band_rows, e.ext_bands);
        check_uniform_bands("extended", L.H, e.ext_band_rows, e.ext_bands);
        CHECK(e.ext_strips * kExtOwnedPx >= L.pitch_px && e.ext_band_rows >= 64 && e.ext_band_rows <= 256, "extended: %d strips, bands of %d rows", e.ext_strips, e.ext_band_rows);
    }
}

// The row bands of the per-frame products (uniform_row_bands) under the constants of their two launches -- the radial profile's 2048 groups and
// 64 bands, the radial-profile threshold's histogram's 512 and 64 -- chosen and forced: they tile the frame, a chosen count keeps to its
// bound, and no batch of 1 .. max_batch frames has more (frame, band) pairs than the partials are sized for.
static void row_bands_case(const Shape& sh) {
    const int H = (int)sh.H;
    const uint32_t pairs[2][2] = {{2048u, 64u}, {512u, 64u}};
    for (const auto& k : pairs) {
        const size_t slots = max_uniform_band_slots(H, sh.max_batch, k[0], k[1]);
        for (uint32_t nf = 1; nf <= sh.max_batch; ++nf)
            for (int forced : {0, 1, 2, 5, H, H + 7}) {
                uint32_t nb = 0, rows = 0;
                uniform_row_bands(H, nf, k[0], k[1], forced, nb, rows);
                check_uniform_bands("row bands", H, (int)rows, (int)nb);
                if (forced > 0) continue;
                CHECK(nb <= std::max(1u, std::min((uint32_t)H, k[1])), "row bands: H %d, %u frames, %u groups: %u bands of at most %u", H, nf, k[0], nb, k[1]);
                CHECK((size_t)nf * nb <= slots, "row bands: H %d, %u frames x %u bands against %zu slots", H, nf, nb, slots);
            }
    }
}

// counting_limit against the expression as it stood at its five call sites
static void counting_limit_case() {
    for (long long mv : {-1ll, 0ll, 1ll, 65534ll, 65535ll, (1ll << 24) - 2, (1ll << 24) - 1, 1ll << 24, 1ll << 31, LLONG_MAX}) {
        const uint32_t was = mv >= 0 ? (uint32_t)std::min<long long>(mv, (1ll << 24) - 1) + 1u : 1u << 24;
        const uint32_t is = counting_limit(mv);
        CHECK(is == was && is != 0u && is <= (1u << 24), "counting_limit(%lld) = %u, was %u", mv, is, was);
    }
}

int main() {
    const Tuning dflt;
    const int F = dflt.frames_per_group;
    const long long T = dflt.target_waves;
    std::vector<Shape> shapes = {
        {4148, 4362, 32},   // Eiger 16M
        {3072, 3072, 32},   // Jungfrau 9M as the benchmark lays it out
        {640, 1800, 8}, {1000, 300, 8}, {1203, 517, 8}, {700, 160, 8}, {700, 2400, 8},
    };
    for (uint32_t W : {1u, 7u, 8u, 9u, 495u, 496u, 497u, 65535u}) shapes.push_back({W, 100, 4});
    for (uint32_t H : {1u, 7u, 71u, 72u, 73u, 143u, 144u, 1024u, 1025u, 4480u, 4481u}) shapes.push_back({512, H, 4});
    shapes.push_back({16384, 16384, 4});   // (32-bit: one frame per group under the 2 GiB limit; 16-bit: three)
    const std::vector<Tune> tunes = {
        {F, T, 0, 0},  {1, T, 0, 0},  {3, T, 0, 0},   {F, 22, 0, 0},   {F, 40, 0, 0},   {1, 40, 0, 0},
        {F, T, 3, 0},  {F, T, 5, 0},  {F, T, 7, 0},   {F, T, 11, 0},   {F, T, 200, 0},
        {F, T, 0, 50}, {F, T, 0, 99}, {F, T, 40, 50}, {F, T, 200, 50}, {F, T, 200, 99},
    };
    for (const Shape& sh : shapes) {
        for (int px : {2, 4}) {
            const uint64_t dense = default_layout(sh.W, sh.H, px).frame_stride;
            for (const Tune& t : tunes) stream_case(sh, px, 0, t);
            for (size_t i = 0; i < 3; ++i) stream_case(sh, px, dense + 4096, tunes[i]);   // padded frames: default, and both frames_per_group cuts
            if (sh.max_batch == 32) stream_case(sh, px, 1ull << 28, tunes[0]);            // ... and padded so far that the 2 GiB limit cuts the groups
        }
        window_ext_case(sh);
        row_bands_case(sh);
    }
    counting_limit_case();
    for (int rows : {47, 50, 74, 75, 96, 97, 100, 104, 150, 173, 1024}) {   // uniform bands of that height as the sparse stage's sub-bands
        const BandSplit split = band_split(StreamGeometry{1, 1, 1, 1, rows, rows, 1});
        std::printf("B %d | %d %d\n", rows, split.sub, split.sub_rows);
    }
    std::printf("%s\n", g_failed ? "FAILED" : "OK");
    return g_failed ? 1 : 0;
}
