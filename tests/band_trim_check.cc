// band_trim_check.cc -- the rows a streaming wave trims off its band's two ends (csrc/launch_geometry.hpp: empty_runs_of, trim_band) without a
// GPU: built and run by tests/test_band_trim.py (g++ with the address and undefined-behaviour sanitizers, against that header alone).
// Brute force over every frame height up to 48 rows, every band height and a few thousand flag vectors, built and random; then the
// Eiger-16M mask's module gaps under the bench geometry, printed band by band.  A line that starts with "FAIL" names a broken property;
// the exit status is then 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "launch_geometry.hpp"

using namespace ffsamd;

static int g_failed = 0;
static long long g_cases = 0, g_vectors = 0, g_many_runs = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            if (++g_failed <= 20) {                   \
                std::printf("FAIL %s: ", #cond);      \
                std::printf(__VA_ARGS__);             \
                std::printf("\n");                    \
            }                                         \
        }                                             \
    } while (0)

// the maximal runs of rows without a valid pixel, the slow way
struct Run { int first, end; };
static std::vector<Run> all_runs(const std::vector<uint8_t>& flags) {
    std::vector<Run> out;
    const int H = (int)flags.size();
    for (int y = 0; y < H; ++y)
        if (!flags[y] && (y == 0 || flags[y - 1])) {
            int e = y;
            while (e < H && !flags[e]) ++e;
            out.push_back({y, e});
        }
    return out;
}

static std::string show(const std::vector<uint8_t>& flags) {
    std::string s;
    for (uint8_t f : flags) s += f ? '1' : '.';
    return s;
}

// what empty_runs_of keeps: maximal runs of the mask, sorted, all of them when they fit, else none shorter than one it left out
static void check_runs(const std::vector<uint8_t>& flags, const EmptyRuns& r) {
    const std::vector<Run> all = all_runs(flags);
    const std::string f = show(flags);
    CHECK(r.n <= (uint32_t)kEmptyRunSlots && r.n == std::min<size_t>(all.size(), kEmptyRunSlots), "%u runs kept of %zu in %s", r.n, all.size(), f.c_str());
    int shortest_kept = 1 << 30;
    std::vector<uint8_t> kept(all.size(), 0);
    for (int k = 0; k < kEmptyRunSlots; ++k) {
        const int first = r.run[k][0], end = r.run[k][1];
        if (k >= (int)r.n) {
            CHECK(first == 0 && end == 0, "slot %d behind the %u kept runs is (%d, %d) in %s", k, r.n, first, end, f.c_str());
            continue;
        }
        bool found = false;
        for (size_t i = 0; i < all.size(); ++i)
            if (all[i].first == first && all[i].end == end) { found = true; kept[i] = 1; }
        CHECK(found, "kept run %d (%d, %d) is no maximal run of %s", k, first, end, f.c_str());
        CHECK(k == 0 || (int)r.run[k - 1][1] < first, "kept run %d (%d, %d) not behind run %d in %s", k, first, end, k - 1, f.c_str());
        shortest_kept = std::min(shortest_kept, end - first);
    }
    for (size_t i = 0; i < all.size(); ++i)
        CHECK(kept[i] || all[i].end - all[i].first <= shortest_kept, "run (%d, %d) left out, a kept one has %d rows: %s", all[i].first, all[i].end, shortest_kept, f.c_str());
}

// the three properties of trim_band on every band of `rows` rows
static void check_bands(const std::vector<uint8_t>& flags, const EmptyRuns& r, int rows) {
    const int H = (int)flags.size();
    const bool all_kept = all_runs(flags).size() <= (size_t)kEmptyRunSlots;
    for (int y0 = 0; y0 < H; y0 += rows) {
        const int y1 = std::min(y0 + rows, H);
        const BandRows t = trim_band(r, y0, y1);
        ++g_cases;
        // inside the band
        CHECK(y0 <= t.yb0 && t.yb0 <= t.yb1 && t.yb1 <= y1, "band %d..%d -> %d..%d in %s", y0, y1, t.yb0, t.yb1, show(flags).c_str());
        // every row of the band with a valid pixel is inside the result
        for (int y = y0; y < y1; ++y)
            CHECK(!flags[y] || (t.yb0 <= y && y < t.yb1), "band %d..%d -> %d..%d leaves out valid row %d of %s", y0, y1, t.yb0, t.yb1, y, show(flags).c_str());
        // every run kept: the result starts and ends on a valid row, or is empty
        if (all_kept && y0 <= t.yb0 && t.yb0 <= t.yb1 && t.yb1 <= y1)
            CHECK(t.yb0 == t.yb1 || (flags[t.yb0] && flags[t.yb1 - 1]), "band %d..%d -> %d..%d starts or ends on an empty row of %s", y0, y1, t.yb0, t.yb1, show(flags).c_str());
    }
}

static void check_vector(const std::vector<uint8_t>& flags) {
    const int H = (int)flags.size();
    const EmptyRuns r = empty_runs_of(flags.data(), H);
    ++g_vectors;
    if (all_runs(flags).size() > (size_t)kEmptyRunSlots) ++g_many_runs;
    check_runs(flags, r);
    for (int rows = 1; rows <= H; ++rows) check_bands(flags, r, rows);
}

static void brute_force() {
    std::mt19937 rng(20250921u);
    for (int H = 1; H <= 48; ++H) {
        std::vector<uint8_t> f((size_t)H);
        // all-empty and all-valid frames
        std::fill(f.begin(), f.end(), 0); check_vector(f);
        std::fill(f.begin(), f.end(), 1); check_vector(f);
        // runs touching row 0 and row H - 1, of every length, alone and together
        for (int k = 1; k < H; ++k) {
            std::fill(f.begin(), f.end(), 1);
            std::fill(f.begin(), f.begin() + k, 0); check_vector(f);
            std::fill(f.begin(), f.end(), 1);
            std::fill(f.end() - k, f.end(), 0); check_vector(f);
            if (2 * k < H) { std::fill(f.begin(), f.begin() + k, 0); check_vector(f); }
        }
        // a run equal to a whole band (check_vector walks every band height, this one among them), the bands beside it valid, and with
        // the run a row longer at either end
        for (int rows = 1; rows <= H; ++rows)
            for (int pick = 0; pick < 3; ++pick) {   // the first band, one in the middle, the last
                const int nb = (H + rows - 1) / rows, b = pick == 0 ? 0 : pick == 1 ? nb / 2 : nb - 1;
                if ((pick == 1 && (b == 0 || b == nb - 1)) || (pick == 2 && b == 0)) continue;
                const int y0 = b * rows, y1 = std::min(y0 + rows, H);
                for (int grow = 0; grow < 4; ++grow) {
                    std::fill(f.begin(), f.end(), 1);
                    std::fill(f.begin() + std::max(0, y0 - (grow & 1)), f.begin() + std::min(H, y1 + (grow >> 1)), 0);
                    check_vector(f);
                }
            }
        // single valid rows between runs: valid rows every `step` rows, nothing else
        for (int step = 2; step <= 7; ++step)
            for (int phase = 0; phase < step; ++phase) {
                for (int y = 0; y < H; ++y) f[(size_t)y] = (y % step == phase) ? 1 : 0;
                check_vector(f);
            }
        // more than 16 runs (from 33 rows on): every other row empty, and runs of two lengths so that the builder has to choose
        for (int phase = 0; phase < 2; ++phase) {
            for (int y = 0; y < H; ++y) f[(size_t)y] = (y + phase) & 1;
            check_vector(f);
            for (int y = 0; y < H; ++y) f[(size_t)y] = (y % 5 == phase || y % 5 == 3) ? 1 : 0;
            check_vector(f);
        }
        // ... and every other row empty but for a few rows flipped
        for (int rep = 0; rep < 8; ++rep) {
            for (int y = 0; y < H; ++y) f[(size_t)y] = (y + rep) & 1;
            for (int flip = 0; flip < 1 + rep / 2; ++flip) f[rng() % (unsigned)H] ^= 1;
            check_vector(f);
        }
        // random vectors at several densities of valid rows
        for (int rep = 0; rep < 48; ++rep) {
            static const unsigned kPerMille[6] = {500, 500, 300, 700, 100, 900};
            const unsigned per_mille = kPerMille[rep % 6];
            for (int y = 0; y < H; ++y) f[(size_t)y] = rng() % 1000u < per_mille ? 1 : 0;
            check_vector(f);
        }
    }
    std::printf("brute force: %lld flag vectors (%lld with more than %d runs), %lld bands\n", g_vectors, g_many_runs, kEmptyRunSlots, g_cases);
}

// The Eiger-16M mask (seven module gaps of 38 rows) under the bench geometry: 56 bands of 78 rows.  Prints "E band:rows ..." for the bands
// that lose rows and the sums the issue's arithmetic rests on.
static void eiger() {
    const int H = 4362, rows = 78, bands = 56;
    std::vector<uint8_t> f((size_t)H, 1);
    for (int k = 0; k < 7; ++k)
        for (int y = 512 + 550 * k; y <= 549 + 550 * k; ++y) f[(size_t)y] = 0;
    const EmptyRuns r = empty_runs_of(f.data(), H);
    CHECK(r.n == 7u, "Eiger: %u runs", r.n);
    CHECK((bands - 1) * rows < H && bands * rows >= H, "Eiger: %d bands of %d rows", bands, rows);
    int trimmed = 0, empty_rows = 0;
    std::printf("E");
    for (int b = 0; b < bands; ++b) {
        const int y0 = band_first_row(b, rows, rows, bands), y1 = std::min(band_first_row(b + 1, rows, rows, bands), H);
        const BandRows t = trim_band(r, y0, y1);
        const int cut = (y1 - y0) - (t.yb1 - t.yb0);
        if (cut) std::printf(" %d:%d", b, cut);
        trimmed += cut;
    }
    for (uint8_t v : f) empty_rows += v ? 0 : 1;
    std::printf("\nEiger: %d rows trimmed of %d empty rows, %d wave rows a strip\n", trimmed, empty_rows, H + 6 * bands);
    CHECK(trimmed == 266 && empty_rows == 266 && H + 6 * bands == 4698, "Eiger: %d trimmed, %d empty", trimmed, empty_rows);
    // a frame taller than 16-bit rows hold: no runs, nothing trimmed
    std::vector<uint8_t> tall(70000, 0);
    const EmptyRuns none = empty_runs_of(tall.data(), (int)tall.size());
    const BandRows t = trim_band(none, 100, 200);
    CHECK(none.n == 0u && t.yb0 == 100 && t.yb1 == 200, "H > 65535: %u runs, band 100..200 -> %d..%d", none.n, t.yb0, t.yb1);
}

int main() {
    brute_force();
    eiger();
    CHECK(g_vectors >= 3000 && g_many_runs >= 30,   // (every other row empty, 34 to 48 rows, either phase: 17 runs or more)
          "%lld vectors, %lld with more than 16 runs", g_vectors, g_many_runs);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
