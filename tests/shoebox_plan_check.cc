// shoebox_plan_check.cc -- the host's decisions about a summation-integration job (csrc/shoebox_plan.hpp) without a GPU: built and run by
// tests/test_shoebox_plan.py (g++ with the address and undefined-behaviour sanitizers).  Every property is held against a restatement written
// here:
//   1. every refusal of a table entry, each with a text that says why, and the first bad entry of a table by its index; entries at the
//      edges of what is allowed (1024 wide, touching the padded image by one pixel) are taken;
//   2. every refusal of a job: algorithm, the two deltas, the geometry;
//   3. the index against a brute-force filter -- z_min < b && z_max > a, in the order of z_min -- on tables with nested, identical and
//      disjoint z-ranges, a very long box early in the order and random ones, for windows before, after, across and inside the scan and
//      empty windows; the span a query looks at never leaves out a box, and skips the boxes that ended before the window when none of their
//      predecessors is long;
//   4. n = 0;  5. the bytes of device state.
// Prints "FAIL ..." lines and a final "OK".
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "shoebox_plan.hpp"

using namespace ffsamd;

static int g_failures = 0;
static void expect(bool ok, const std::string& what) {
    if (!ok && ++g_failures <= 40) std::printf("FAIL %s\n", what.c_str());
}

static const double kS0[3] = {0.0, 0.0, -1.0};
static const int W = 96, H = 80;

static ShoeboxEntry good() {
    ShoeboxEntry b{};
    b.s1[0] = 0.1, b.s1[1] = 0.2, b.s1[2] = -0.97;
    b.phi = 0.3;
    b.x_min = 10, b.x_max = 20, b.y_min = 5, b.y_max = 9, b.z_min = 0, b.z_max = 3;
    return b;
}
static void refused(const ShoeboxEntry& b, const char* needle, const std::string& what) {
    const std::string why = shoebox_entry_refusal(b, kS0, W, H);
    expect(!why.empty() && why.find(needle) != std::string::npos, what + ": got \"" + why + "\"");
}
static void taken(const ShoeboxEntry& b, const std::string& what) {
    const std::string why = shoebox_entry_refusal(b, kS0, W, H);
    expect(why.empty(), what + ": refused, \"" + why + "\"");
}

static void check_entries() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    taken(good(), "a plain box");
    ShoeboxEntry b = good();
    b.x_max = b.x_min;
    refused(b, "empty or reversed", "x empty");
    b = good(), b.y_max = b.y_min - 1;
    refused(b, "empty or reversed", "y reversed");
    b = good(), b.z_max = b.z_min;
    refused(b, "empty or reversed", "z empty");
    b = good(), b.x_min = -500, b.x_max = 524;
    taken(b, "1024 wide");
    b.x_max = 525;
    refused(b, "wider", "1025 wide");
    b = good(), b.y_min = -500, b.y_max = 524;
    taken(b, "1024 high");
    b.y_max = 525;
    refused(b, "higher", "1025 high");
    b = good(), b.x_min = std::numeric_limits<int32_t>::min(), b.x_max = std::numeric_limits<int32_t>::max();
    refused(b, "wider", "the widest box there is (no overflow in its width)");
    // the padded image is [-1024, W + 1024) x [-1024, H + 1024): a box that shares one pixel with it is taken
    b = good(), b.x_min = -1030, b.x_max = -1023;
    taken(b, "touches the padded image on the left");
    b.x_max = -1024;
    refused(b, "outside the image", "left of the padded image");
    b = good(), b.x_min = W + 1023, b.x_max = W + 1030;
    taken(b, "touches the padded image on the right");
    b.x_min = W + 1024;
    refused(b, "outside the image", "right of the padded image");
    b = good(), b.y_min = -1030, b.y_max = -1024;
    refused(b, "outside the image", "above the padded image");
    b = good(), b.y_min = H + 1024, b.y_max = H + 1030;
    refused(b, "outside the image", "below the padded image");
    b = good(), b.y_min = H + 1023, b.y_max = H + 1030;
    taken(b, "touches the padded image at the bottom");
    for (int k = 0; k < 3; ++k) {
        b = good(), b.s1[k] = nan;
        refused(b, "s1", "s1 NaN");
        b = good(), b.s1[k] = -inf;
        refused(b, "s1", "s1 infinite");
    }
    b = good(), b.phi = inf;
    refused(b, "phi", "phi infinite");
    b = good(), b.phi = nan;
    refused(b, "phi", "phi NaN");
    b = good(), b.s1[0] = 0.0, b.s1[1] = 0.0, b.s1[2] = -2.0;
    refused(b, "parallel", "s1 parallel to s0");
    b.s1[2] = 0.0;
    refused(b, "parallel", "s1 zero");
    b = good(), b.z_min = -100, b.z_max = -50;
    taken(b, "a z-range before the scan (it simply never meets an image)");

    std::vector<ShoeboxEntry> t(5, good());
    std::string why;
    expect(shoebox_table_refusal(t.data(), 5, kS0, W, H, why) == -1, "a good table");
    expect(shoebox_table_refusal(t.data(), 0, kS0, W, H, why) == -1, "an empty table");
    t[3].phi = nan, t[4].x_max = t[4].x_min;
    expect(shoebox_table_refusal(t.data(), 5, kS0, W, H, why) == 3 && why.find("phi") != std::string::npos, "the first bad entry is named");
}

static void check_job() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    ShoeboxGeometry g{};
    const double D[9] = {1, 0, -4.8, 0, -1, 4.0, 0, 0, -200};
    for (int i = 0; i < 9; ++i) g.d_matrix[i] = D[i];
    g.pixel_size_mm[0] = g.pixel_size_mm[1] = 0.1, g.wavelength = 1.0, g.s0[2] = -1.0, g.rot_axis[0] = 1.0, g.osc_start_deg = 0.0, g.osc_width_deg = 0.1;
    expect(shoebox_job_refusal(g, kShoeboxEllipsoid, 1e-3, 2e-3).empty() && shoebox_job_refusal(g, kShoeboxDials, 1e-3, 2e-3).empty(), "a plain job");
    expect(shoebox_job_refusal(g, 2, 1e-3, 2e-3).find("algorithm") != std::string::npos && shoebox_job_refusal(g, -1, 1e-3, 2e-3).find("algorithm") != std::string::npos,
           "unknown algorithms");
    for (double bad : {0.0, -1e-3, inf, nan}) {
        expect(shoebox_job_refusal(g, 0, bad, 2e-3).find("delta_b") != std::string::npos, "delta_b " + std::to_string(bad));
        expect(shoebox_job_refusal(g, 0, 1e-3, bad).find("delta_m") != std::string::npos, "delta_m " + std::to_string(bad));
    }
    for (int i = 0; i < 20; ++i) {
        double v[20];   // (the struct is twenty doubles)
        std::memcpy(v, &g, sizeof v);
        v[i] = nan;
        ShoeboxGeometry h;
        std::memcpy(&h, v, sizeof h);
        expect(shoebox_job_refusal(h, 0, 1e-3, 2e-3).find("not finite") != std::string::npos, "geometry entry " + std::to_string(i) + " NaN");
    }
    ShoeboxGeometry h = g;
    h.wavelength = 0.0;
    expect(shoebox_job_refusal(h, 0, 1e-3, 2e-3).find("positive") != std::string::npos, "wavelength 0");
    h = g, h.pixel_size_mm[1] = -0.1;
    expect(shoebox_job_refusal(h, 0, 1e-3, 2e-3).find("positive") != std::string::npos, "a negative pixel size");
}

static std::vector<ShoeboxEntry> table_of(const std::vector<std::pair<int, int>>& z) {
    std::vector<ShoeboxEntry> t;
    for (auto [a, b] : z) {
        ShoeboxEntry e = good();
        e.z_min = a, e.z_max = b;
        t.push_back(e);
    }
    return t;
}

static void check_index(const std::vector<ShoeboxEntry>& t, const std::string& name, int lo_w, int hi_w) {
    ShoeboxIndex ix;
    ix.build(t.data(), (uint32_t)t.size());
    expect(ix.order.size() == t.size(), name + ": the order holds every box");
    for (size_t k = 1; k < ix.order.size(); ++k) {
        const ShoeboxEntry &p = t[ix.order[k - 1]], &q = t[ix.order[k]];
        expect(p.z_min < q.z_min || (p.z_min == q.z_min && ix.order[k - 1] < ix.order[k]), name + ": sorted by z_min, ties by index");
        expect(ix.run_max[k] >= ix.run_max[k - 1] && ix.run_max[k] >= q.z_max, name + ": the running maximum");
    }
    std::vector<uint32_t> got;
    for (int a = lo_w; a <= hi_w; ++a)
        for (int b = a - 1; b <= hi_w + 1; ++b) {
            ix.query(a, b, got);
            std::vector<uint32_t> want;
            for (uint32_t k : ix.order)
                if (a < b && t[k].z_min < b && t[k].z_max > a) want.push_back(k);
            expect(got == want, name + ": window [" + std::to_string(a) + ", " + std::to_string(b) + ")");
        }
}

static void check_indices() {
    check_index(table_of({{0, 10}, {1, 9}, {2, 8}, {3, 7}, {4, 6}}), "nested", -3, 13);
    check_index(table_of({{4, 6}, {3, 7}, {2, 8}, {1, 9}, {0, 10}}), "nested, table order reversed", -3, 13);
    check_index(table_of({{2, 5}, {2, 5}, {2, 5}, {2, 5}}), "identical", -1, 8);
    check_index(table_of({{0, 2}, {2, 4}, {4, 6}, {8, 9}, {20, 22}}), "disjoint", -2, 25);
    check_index(table_of({{0, 1000}, {1, 2}, {2, 3}, {3, 4}, {50, 51}, {60, 62}}), "a very long box early in the order", -2, 70);
    check_index(table_of({{-10, -5}, {-3, 2}, {30, 40}}), "boxes before and after the windows", -12, 45);
    check_index({}, "n = 0", -2, 3);
    std::mt19937 rng(7);
    for (int round = 0; round < 20; ++round) {
        std::vector<std::pair<int, int>> z;
        const int n = 1 + (int)(rng() % 60);
        for (int i = 0; i < n; ++i) {
            const int a = (int)(rng() % 40) - 5;
            z.push_back({a, a + 1 + (int)(rng() % (round % 4 == 0 ? 30 : 4))});
        }
        check_index(table_of(z), "random " + std::to_string(round), -8, 70);
    }
    // without a long box ahead of them, the boxes that ended before the window are not looked at: the span is short
    std::vector<std::pair<int, int>> z;
    for (int i = 0; i < 1000; ++i) z.push_back({i, i + 2});
    const std::vector<ShoeboxEntry> t = table_of(z);
    ShoeboxIndex ix;
    ix.build(t.data(), (uint32_t)t.size());
    size_t lo, hi;
    ix.span(500, 508, lo, hi);
    expect(lo == 499 && hi == 508, "the span of [500, 508) over 1000 short boxes is [499, 508), got [" + std::to_string(lo) + ", " + std::to_string(hi) + ")");
    ix.span(-5, 0, lo, hi);
    expect(lo == hi, "a window before the scan looks at nothing");
    ix.span(2000, 2010, lo, hi);
    expect(lo == hi, "a window after the scan looks at nothing");
}

int main() {
    check_entries();
    check_job();
    check_indices();
    expect(shoebox_state_bytes() == 48 + 1024, "1072 bytes of device state a shoebox");
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
