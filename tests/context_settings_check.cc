// context_settings_check.cc -- a context's settings and the rules of its setters (csrc/context_settings.hpp) without a GPU: built and run by
// tests/test_context_settings.py (g++ with the address and undefined-behaviour sanitizers, against that header alone).  Four parts:
//   1. every refusal's text against a literal -- the six pair rules from either caller, and every range refusal;
//   2. both halves of a pair rule agree: from every consistent state of a small space, a single call is accepted exactly when it leaves a
//      consistent state, and a refused call says the rule its result would break.  "Consistent" is restated here (broken_rule), not read
//      from the header's table;
//   3. reachability: breadth-first over accepted calls from the defaults, every state reached is consistent;
//   4. snapshot_of copies every member, and radthr_bins follows the algorithm.
// No named exception to part 2 was needed: the setters behave as that property says everywhere in the space.
// Prints "FAIL ..." lines and a final "OK".
#include <cmath>
#include <cstdio>
#include <deque>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "context_settings.hpp"

using namespace ffsamd;

static int g_failures = 0;
static void fail(const std::string& what) {
    std::printf("FAIL %s\n", what.c_str());
    ++g_failures;
}
static void expect_text(const std::string& what, const std::string& got, const std::string& want) {
    if (got != want) fail(what + ": got \"" + got + "\", want \"" + want + "\"");
}

// ---- the texts, as the library has always said them -------------------------------------------------------------------------------------
// [rule][0]: the first caller's text, [rule][1]: the second's; rule 1's two texts end with the bins of the map
enum Rule { kNoMap = 0, kWideMap = 1, kFlavourScope = 2, kFlavourGain = 3, kGainAndMap = 4, kFlavourMap = 5, kExtendedWindow = 6, kNone = -1 };
static const char* const kPairText[6][2] = {
    {"ffs_ctx_set_params: the radial_profile algorithm needs a radial bin map (ffs_ctx_set_radial_bins) and the context has none",
     "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which needs the map: set another algorithm first"},
    {"ffs_ctx_set_params: the radial_profile algorithm takes a radial bin map of at most 128 bins and the context's has ",
     "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which takes at most 128 bins, got "},
    {"ffs_ctx_set_params: extended_flavour 1 cannot be combined with the window scope of max_valid (ffs_ctx_set_max_valid_scope): the device-flavour erosion skips "
     "masked neighbours by the static mask",
     "ffs_ctx_set_max_valid_scope: the window scope cannot be combined with extended_flavour 1: the device-flavour erosion skips masked neighbours by the static mask"},
    {"ffs_ctx_set_params: extended_flavour 1 cannot be combined with a detector gain (ffs_ctx_set_gain): the reference's device kernels, which that flavour copies, "
     "have no gain",
     "ffs_ctx_set_gain: a detector gain cannot be combined with extended_flavour 1: the reference's device kernels, which that flavour copies, have no gain"},
    {"ffs_ctx_set_gain: a gain map is set (ffs_ctx_set_gain_map): drop it with ffs_ctx_set_gain_map(ctx, NULL) first",
     "ffs_ctx_set_gain_map: a scalar gain is set (ffs_ctx_set_gain): switch it off with ffs_ctx_set_gain(ctx, 0) first"},
    {"ffs_ctx_set_params: extended_flavour 1 cannot be combined with a gain map (ffs_ctx_set_gain_map): the reference's device kernels, which that flavour copies, "
     "have no gain",
     "ffs_ctx_set_gain_map: a gain map cannot be combined with extended_flavour 1: the reference's device kernels, which that flavour copies, have no gain"},
};
static const char* const kExtendedWindowText =
    "ffs_ctx_set_params: the extended dispersion algorithm needs the 7x7 window (kernel_half_x = kernel_half_y = 3): its erosion and final pass derive from it";
static const Setter kPairCallers[6][2] = {{Setter::kParams, Setter::kRadialBins},    {Setter::kParams, Setter::kRadialBins}, {Setter::kParams, Setter::kMaxValidScope},
                                          {Setter::kParams, Setter::kGain},          {Setter::kGain, Setter::kGainMap},      {Setter::kParams, Setter::kGainMap}};

// ---- one call of one setter: what the header says to it, and what the setter stores when it is accepted ----------------------------------
struct Call {
    Setter kind = Setter::kParams;
    ffs_params params = default_params();   // kParams
    double gain = 0.0;                      // kGain
    bool on = false;                        // kGainMap: a map, not NULL
    int scope = FFS_MAX_VALID_CENTRE;       // kMaxValidScope
    uint32_t bins = 0;                      // kRadialBins: 0 = NULL
    std::string ask(const ContextSettings& s) const {
        switch (kind) {
            case Setter::kParams: return set_params(s, params);
            case Setter::kGain: return set_gain(s, gain);
            case Setter::kGainMap: return set_gain_map(s, on);
            case Setter::kMaxValidScope: return set_max_valid_scope(s, scope);
            case Setter::kRadialBins: return set_radial_bins(s, bins != 0, bins);
        }
        return "?";
    }
    void store(ContextSettings& s) const {
        switch (kind) {
            case Setter::kParams: s.params = params; break;
            case Setter::kGain: s.gain = gain; break;
            case Setter::kGainMap: s.gain_map = on; break;
            case Setter::kMaxValidScope: s.max_valid_scope = scope; break;
            case Setter::kRadialBins: s.radial_bins = bins; break;
        }
    }
    std::string name() const {
        switch (kind) {
            case Setter::kParams:
                return "set_params(algorithm " + std::to_string(params.algorithm) + ", flavour " + std::to_string(params.extended_flavour) + ", half "
                       + std::to_string(params.kernel_half_x) + ")";
            case Setter::kGain: return "set_gain(" + std::to_string(gain) + ")";
            case Setter::kGainMap: return std::string("set_gain_map(") + (on ? "map" : "NULL") + ")";
            case Setter::kMaxValidScope: return "set_max_valid_scope(" + std::to_string(scope) + ")";
            case Setter::kRadialBins: return "set_radial_bins(" + std::to_string(bins) + ")";
        }
        return "?";
    }
};
static Call call_params(int algorithm, int flavour, int half) {
    Call c;
    c.kind = Setter::kParams;
    c.params.algorithm = algorithm;
    c.params.extended_flavour = flavour;
    c.params.kernel_half_x = c.params.kernel_half_y = half;
    return c;
}
static Call call_gain(double g) { Call c; c.kind = Setter::kGain; c.gain = g; return c; }
static Call call_gain_map(bool on) { Call c; c.kind = Setter::kGainMap; c.on = on; return c; }
static Call call_scope(int scope) { Call c; c.kind = Setter::kMaxValidScope; c.scope = scope; return c; }
static Call call_bins(uint32_t bins) { Call c; c.kind = Setter::kRadialBins; c.bins = bins; return c; }

// ---- the state space of parts 2 and 3 -----------------------------------------------------------------------------------------------------
static const int kAlgorithms[3] = {FFS_ALGO_DISPERSION, FFS_ALGO_DISPERSION_EXTENDED, FFS_ALGO_RADIAL_PROFILE};
static const int kFlavours[2] = {0, 1};
static const int kScopes[2] = {FFS_MAX_VALID_CENTRE, FFS_MAX_VALID_WINDOW};
static const double kGains[2] = {0.0, 2.5};
static const bool kMaps[2] = {false, true};
static const uint32_t kBins[5] = {0, 100, 128, 129, 1024};
static const int kHalves[2] = {3, 4};   // the default window, and 9 x 9 (half sizes 4 x 4)

static std::vector<Call> all_calls() {
    std::vector<Call> calls;
    for (int a : kAlgorithms)
        for (int f : kFlavours)
            for (int h : kHalves) calls.push_back(call_params(a, f, h));
    for (double g : kGains) calls.push_back(call_gain(g));
    for (bool m : kMaps) calls.push_back(call_gain_map(m));
    for (int s : kScopes) calls.push_back(call_scope(s));
    for (uint32_t b : kBins) calls.push_back(call_bins(b));
    return calls;
}
// The first rule the state breaks, in the order ffs_ctx_set_params has always checked (the window of the extended algorithm among its range
// checks, then the map, the scope, the gain, the gain map); the one pair without the parameters, gain and gain map, comes between the two it
// cannot coincide with in a state one call away from a consistent one.  Stated on its own, not through the header's table.
static int broken_rule(const ContextSettings& s) {
    const ffs_params& p = s.params;
    if (p.algorithm == FFS_ALGO_DISPERSION_EXTENDED && !(p.kernel_half_x == 3 && p.kernel_half_y == 3)) return kExtendedWindow;
    if (p.algorithm == FFS_ALGO_RADIAL_PROFILE && s.radial_bins == 0) return kNoMap;
    if (p.algorithm == FFS_ALGO_RADIAL_PROFILE && s.radial_bins > 128) return kWideMap;
    if (p.extended_flavour == 1 && s.max_valid_scope == FFS_MAX_VALID_WINDOW) return kFlavourScope;
    if (p.extended_flavour == 1 && s.gain > 0.0) return kFlavourGain;
    if (s.gain > 0.0 && s.gain_map) return kGainAndMap;
    if (p.extended_flavour == 1 && s.gain_map) return kFlavourMap;
    return kNone;
}
static std::string rule_text(int rule, Setter caller, const ContextSettings& after) {
    if (rule == kExtendedWindow) return kExtendedWindowText;
    const int side = caller == kPairCallers[rule][0] ? 0 : 1;
    if (caller != kPairCallers[rule][side]) return "(rule " + std::to_string(rule) + " does not name this setter)";
    return std::string(kPairText[rule][side]) + (rule == kWideMap ? std::to_string(after.radial_bins) : std::string());
}
static std::string describe(const ContextSettings& s) {
    return "[algorithm " + std::to_string(s.params.algorithm) + " flavour " + std::to_string(s.params.extended_flavour) + " half " + std::to_string(s.params.kernel_half_x)
           + " scope " + std::to_string(s.max_valid_scope) + " gain " + std::to_string(s.gain) + " map " + std::to_string((int)s.gain_map) + " bins "
           + std::to_string(s.radial_bins) + "]";
}
static long state_key(const ContextSettings& s) {
    return ((((((long)s.params.algorithm * 2 + s.params.extended_flavour) * 16 + s.params.kernel_half_x) * 2 + s.max_valid_scope) * 2 + (s.gain > 0.0 ? 1 : 0)) * 2
            + (s.gain_map ? 1 : 0)) * 2048 + (long)s.radial_bins;
}

// ---- 1. texts ---------------------------------------------------------------------------------------------------------------------------------
static void check_pair_texts() {
    // for each rule: the call that sets one side from the defaults, then the other side's call is refused -- and the other way round
    struct Scenario { int rule; Call first, second; };   // `first` is the rule's first caller's setting, `second` its second caller's
    const Scenario scenarios[6] = {
        {kNoMap, call_params(FFS_ALGO_RADIAL_PROFILE, 0, 3), call_bins(0)},
        {kWideMap, call_params(FFS_ALGO_RADIAL_PROFILE, 0, 3), call_bins(129)},
        {kFlavourScope, call_params(FFS_ALGO_DISPERSION, 1, 3), call_scope(FFS_MAX_VALID_WINDOW)},
        {kFlavourGain, call_params(FFS_ALGO_DISPERSION, 1, 3), call_gain(2.5)},
        {kGainAndMap, call_gain(2.5), call_gain_map(true)},
        {kFlavourMap, call_params(FFS_ALGO_DISPERSION, 1, 3), call_gain_map(true)},
    };
    for (const Scenario& sc : scenarios)
        for (int order = 0; order < 2; ++order) {
            const Call& a = order == 0 ? sc.first : sc.second;
            const Call& b = order == 0 ? sc.second : sc.first;
            ContextSettings s;
            s.params = default_params();
            if (sc.rule <= kWideMap && order == 0) s.radial_bins = 100;   // (the algorithm can only be set over a map: the second call then drops or widens it)
            const std::string what = "rule " + std::to_string(sc.rule) + ", " + a.name() + " then " + b.name();
            if (sc.rule == kNoMap && order == 1) {   // "no map" is the default: there is no first call to make
                expect_text(what, b.ask(s), kPairText[kNoMap][0]);
                continue;
            }
            expect_text(what + " (first call)", a.ask(s), "");
            a.store(s);
            expect_text(what, b.ask(s), std::string(kPairText[sc.rule][order == 0 ? 1 : 0]) + (sc.rule == kWideMap ? "129" : ""));
        }
}
static void check_range_texts() {
    ContextSettings s;
    s.params = default_params();
    auto with = [&](auto&& change) { ffs_params p = default_params(); change(p); return set_params(s, p); };
    const std::string halves = "ffs_ctx_set_params: kernel_half_x / kernel_half_y must be in 1..7 (0 = 3)";
    expect_text("kernel_half_x -1", with([](ffs_params& p) { p.kernel_half_x = -1; }), halves);
    expect_text("kernel_half_x 8", with([](ffs_params& p) { p.kernel_half_x = 8; }), halves);
    expect_text("kernel_half_y -1", with([](ffs_params& p) { p.kernel_half_y = -1; }), halves);
    expect_text("kernel_half_y 8", with([](ffs_params& p) { p.kernel_half_y = 8; }), halves);
    expect_text("kernel_half 0 x 7", with([](ffs_params& p) { p.kernel_half_x = 0; p.kernel_half_y = 7; }), "");
    const std::string counts = "ffs_ctx_set_params: need 2 <= min_count <= (2*kernel_half_x+1)*(2*kernel_half_y+1) (49 for the 7x7 window), nsig_b >= 0, nsig_s >= 0, threshold >= 0";
    expect_text("min_count 1", with([](ffs_params& p) { p.min_count = 1; }), counts);
    expect_text("min_count 50 in 7x7", with([](ffs_params& p) { p.min_count = 50; }), counts);
    expect_text("min_count 49 in 7x7", with([](ffs_params& p) { p.min_count = 49; }), "");
    expect_text("min_count 10 in 3x3", with([](ffs_params& p) { p.kernel_half_x = p.kernel_half_y = 1; p.min_count = 10; }), counts);
    expect_text("min_count 9 in 3x3", with([](ffs_params& p) { p.kernel_half_x = p.kernel_half_y = 1; p.min_count = 9; }), "");
    expect_text("min_count 50 in 0x0 = 7x7", with([](ffs_params& p) { p.kernel_half_x = p.kernel_half_y = 0; p.min_count = 50; }), counts);
    expect_text("nsig_b < 0", with([](ffs_params& p) { p.nsig_b = -0.5; }), counts);
    expect_text("nsig_s < 0", with([](ffs_params& p) { p.nsig_s = -0.5; }), counts);
    expect_text("threshold < 0", with([](ffs_params& p) { p.threshold = -1.0; }), counts);
    const std::string unknown = "ffs_ctx_set_params: unknown algorithm / extended_flavour";
    expect_text("algorithm 3", with([](ffs_params& p) { p.algorithm = 3; }), unknown);
    expect_text("algorithm -1", with([](ffs_params& p) { p.algorithm = -1; }), unknown);
    expect_text("flavour 2", with([](ffs_params& p) { p.extended_flavour = 2; }), unknown);
    expect_text("extended, 9x9", with([](ffs_params& p) { p.algorithm = FFS_ALGO_DISPERSION_EXTENDED; p.kernel_half_x = p.kernel_half_y = 4; }), kExtendedWindowText);
    expect_text("extended, 7x5", with([](ffs_params& p) { p.algorithm = FFS_ALGO_DISPERSION_EXTENDED; p.kernel_half_y = 2; }), kExtendedWindowText);
    expect_text("extended, 0x0 = 7x7", with([](ffs_params& p) { p.algorithm = FFS_ALGO_DISPERSION_EXTENDED; p.kernel_half_x = p.kernel_half_y = 0; }), "");
    // (the order of one call's checks: the halves before the counts, the extended window before the unknown flavour, ranges before pairs)
    expect_text("halves before counts", with([](ffs_params& p) { p.kernel_half_x = 8; p.min_count = 1; }), halves);
    expect_text("window before flavour", with([](ffs_params& p) { p.algorithm = FFS_ALGO_DISPERSION_EXTENDED; p.kernel_half_x = 4; p.extended_flavour = 2; }), kExtendedWindowText);
    expect_text("ranges before pairs", with([](ffs_params& p) { p.algorithm = FFS_ALGO_RADIAL_PROFILE; p.min_count = 1; }), counts);

    const std::string gain = "ffs_ctx_set_gain: the gain must be finite and >= 0 (0 = off: pixel values are photon counts)";
    expect_text("gain -1", set_gain(s, -1.0), gain);
    expect_text("gain nan", set_gain(s, std::nan("")), gain);
    expect_text("gain inf", set_gain(s, std::numeric_limits<double>::infinity()), gain);
    expect_text("gain 0", set_gain(s, 0.0), "");
    const std::string scope = "ffs_ctx_set_max_valid_scope: scope must be FFS_MAX_VALID_CENTRE (0) or FFS_MAX_VALID_WINDOW (1)";
    expect_text("scope 2", set_max_valid_scope(s, 2), scope);
    expect_text("scope -1", set_max_valid_scope(s, -1), scope);
    const std::string n_iqr = "ffs_ctx_set_radial_threshold: n_iqr must be finite and in 0 .. 2^20 (the cutoff median + n_iqr * iqr is a uint32)";
    expect_text("n_iqr -1", set_radial_threshold(s, -1.0), n_iqr);
    expect_text("n_iqr nan", set_radial_threshold(s, std::nan("")), n_iqr);
    expect_text("n_iqr inf", set_radial_threshold(s, std::numeric_limits<double>::infinity()), n_iqr);
    expect_text("n_iqr 2^20 + 1", set_radial_threshold(s, 1048577.0), n_iqr);
    expect_text("n_iqr 2^20", set_radial_threshold(s, 1048576.0), "");
    expect_text("n_iqr 0", set_radial_threshold(s, 0.0), "");
    expect_text("blur 3", set_radial_blur(s, 3), "ffs_ctx_set_radial_blur: blur must be FFS_RADIAL_BLUR_NONE (0), _NARROW (1) or _WIDE (2), got 3");
    expect_text("blur -1", set_radial_blur(s, -1), "ffs_ctx_set_radial_blur: blur must be FFS_RADIAL_BLUR_NONE (0), _NARROW (1) or _WIDE (2), got -1");
    for (int blur : {0, 1, 2}) expect_text("blur " + std::to_string(blur), set_radial_blur(s, blur), "");
    expect_text("n_bins 0", set_radial_bins(s, true, 0), "ffs_ctx_set_radial_bins: n_bins must be in 1..1024, got 0");
    expect_text("n_bins 1025", set_radial_bins(s, true, 1025), "ffs_ctx_set_radial_bins: n_bins must be in 1..1024, got 1025");
    expect_text("n_bins 1", set_radial_bins(s, true, 1), "");
    expect_text("n_bins 1024", set_radial_bins(s, true, 1024), "");
    expect_text("NULL map, n_bins 5000", set_radial_bins(s, false, 5000), "");
    ContextSettings r = s;   // under the radial_profile algorithm, over a map of 100 bins
    r.params.algorithm = FFS_ALGO_RADIAL_PROFILE;
    r.radial_bins = 100;
    expect_text("radial_profile, NULL map", set_radial_bins(r, false, 0),
                "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which needs the map: set another algorithm first");
    expect_text("radial_profile, 129 bins", set_radial_bins(r, true, 129),
                "ffs_ctx_set_radial_bins: the context's parameters say the radial_profile algorithm, which takes at most 128 bins, got 129");
    expect_text("radial_profile, 1025 bins: the range first", set_radial_bins(r, true, 1025), "ffs_ctx_set_radial_bins: n_bins must be in 1..1024, got 1025");
    expect_text("radial_profile, 128 bins", set_radial_bins(r, true, 128), "");
    ContextSettings w = s;
    w.radial_bins = 1024;
    expect_text("set_params over 1024 bins", with([](ffs_params&) {}), "");
    {
        ffs_params p = default_params();
        p.algorithm = FFS_ALGO_RADIAL_PROFILE;
        expect_text("radial_profile over 1024 bins", set_params(w, p),
                    "ffs_ctx_set_params: the radial_profile algorithm takes a radial bin map of at most 128 bins and the context's has 1024");
    }
    const std::string jf = "ffs_ctx_set_jungfrau_calibration: raw Jungfrau words convert to 32-bit photon counts: the context must have pixel_bytes 4";
    expect_text("calibration, 16-bit context", set_jungfrau_calibration(s, true), jf);
    expect_text("no calibration, 16-bit context", set_jungfrau_calibration(s, false), "");
    ContextSettings s32 = s;
    s32.pixel_bytes = 4;
    expect_text("calibration, 32-bit context", set_jungfrau_calibration(s32, true), "");
    // the entry text of the gain map, the bin map and the calibration, on rows of 16
    expect_text("entry_text float", entry_text(87, 16, 0.0f), "entry 87 (x = 7, y = 5) is 0.000000");
    expect_text("entry_text uint16", entry_text(87, 16, (uint16_t)100), "entry 87 (x = 7, y = 5) is 100");
    expect_text("entry_text first", entry_text(0, 16, -1.5f), "entry 0 (x = 0, y = 0) is -1.500000");
}

// ---- 2. both halves agree ---------------------------------------------------------------------------------------------------------------------
static void check_halves_agree() {
    const std::vector<Call> calls = all_calls();
    size_t consistent = 0, accepted = 0, refused = 0;
    for (int a : kAlgorithms) for (int f : kFlavours) for (int h : kHalves) for (int sc : kScopes) for (double g : kGains) for (bool m : kMaps) for (uint32_t b : kBins) {
        ContextSettings s;
        s.params = call_params(a, f, h).params;
        s.max_valid_scope = sc;
        s.gain = g;
        s.gain_map = m;
        s.radial_bins = b;
        if (broken_rule(s) != kNone) continue;
        ++consistent;
        for (const Call& call : calls) {
            ContextSettings after = s;
            call.store(after);
            if (state_key(after) == state_key(s)) continue;   // (not a change)
            const int rule = broken_rule(after);
            const std::string got = call.ask(s);
            const std::string want = rule == kNone ? std::string() : rule_text(rule, call.kind, after);
            if (got != want) fail("from " + describe(s) + " " + call.name() + ": got \"" + got + "\", want \"" + want + "\"");
            ++(rule == kNone ? accepted : refused);
        }
    }
    // (the space is not vacuous: 3 x 2 x 2 x 2 x 2 x 2 x 5 = 480 states)
    if (consistent < 100 || accepted < 500 || refused < 500)
        fail("part 2 walked " + std::to_string(consistent) + " consistent states, " + std::to_string(accepted) + " accepted and " + std::to_string(refused) + " refused calls");
}

// ---- 3. reachability ----------------------------------------------------------------------------------------------------------------------------
static void check_reachable_states() {
    const std::vector<Call> calls = all_calls();
    ContextSettings start;
    start.params = default_params();
    std::set<long> seen{state_key(start)};
    std::deque<ContextSettings> todo{start};
    while (!todo.empty()) {
        const ContextSettings s = todo.front();
        todo.pop_front();
        if (broken_rule(s) != kNone) fail("reached " + describe(s) + ", which breaks rule " + std::to_string(broken_rule(s)));
        for (const Call& call : calls) {
            if (!call.ask(s).empty()) continue;
            ContextSettings next = s;
            call.store(next);
            if (seen.insert(state_key(next)).second) todo.push_back(next);
        }
    }
    if (seen.size() < 100) fail("part 3 reached only " + std::to_string(seen.size()) + " states");
}

// ---- 4. the snapshot ------------------------------------------------------------------------------------------------------------------------------
static void check_snapshot() {
    ContextSettings s;
    s.params = default_params();
    s.params.min_count = 5;
    s.params.nsig_b = 4.5;
    s.params.nsig_s = 2.5;
    s.params.threshold = 7.0;
    s.params.max_valid = 65000;
    s.params.min_spot_size = 4;
    s.params.min_spot_size_3d = 6;
    s.params.max_peak_centroid_separation = 3.5f;
    s.params.want_reflections = 0;
    s.params.want_strong_list = 1;
    s.params.want_strong_mask = 1;
    s.params.algorithm = FFS_ALGO_RADIAL_PROFILE;
    s.params.extended_flavour = 1;
    s.params.kernel_half_x = 2;
    s.params.kernel_half_y = 5;
    s.max_valid_scope = FFS_MAX_VALID_WINDOW;
    s.gain = 2.5;
    s.gain_map = true;
    s.radial_bins = 77;
    s.n_iqr = 3.25;
    s.radial_blur = FFS_RADIAL_BLUR_WIDE;
    s.pixel_stats = true;
    s.jungfrau_calibration = true;
    s.pixel_bytes = 4;
    const ParamSnapshot b = snapshot_of(s);
    const ffs_params &p = b.params, &q = s.params;
    if (p.min_count != q.min_count || p.nsig_b != q.nsig_b || p.nsig_s != q.nsig_s || p.threshold != q.threshold || p.max_valid != q.max_valid
        || p.min_spot_size != q.min_spot_size || p.min_spot_size_3d != q.min_spot_size_3d || p.max_peak_centroid_separation != q.max_peak_centroid_separation
        || p.want_reflections != q.want_reflections || p.want_strong_list != q.want_strong_list || p.want_strong_mask != q.want_strong_mask
        || p.algorithm != q.algorithm || p.extended_flavour != q.extended_flavour || p.kernel_half_x != q.kernel_half_x || p.kernel_half_y != q.kernel_half_y)
        fail("snapshot: params");
    if (b.max_valid_scope != FFS_MAX_VALID_WINDOW) fail("snapshot: max_valid_scope");
    if (b.gain != 2.5) fail("snapshot: gain");
    if (!b.gain_map) fail("snapshot: gain_map");
    if (b.radial_bins != 77) fail("snapshot: radial_bins");
    if (!b.pixel_stats) fail("snapshot: pixel_stats");
    if (b.radthr_bins != 77) fail("snapshot: radthr_bins under radial_profile");
    if (b.n_iqr != 3.25) fail("snapshot: n_iqr");
    if (b.radial_blur != FFS_RADIAL_BLUR_WIDE) fail("snapshot: radial_blur");
    for (int algorithm : {FFS_ALGO_DISPERSION, FFS_ALGO_DISPERSION_EXTENDED}) {
        s.params.algorithm = algorithm;
        const ParamSnapshot o = snapshot_of(s);
        if (o.radthr_bins != 0 || o.radial_bins != 77) fail("snapshot: radthr_bins / radial_bins under algorithm " + std::to_string(algorithm));
    }
    const ParamSnapshot d = snapshot_of(ContextSettings{});   // (and the defaults are the snapshot's own)
    const ParamSnapshot e;
    if (d.max_valid_scope != e.max_valid_scope || d.gain != e.gain || d.gain_map != e.gain_map || d.radial_bins != e.radial_bins || d.pixel_stats != e.pixel_stats
        || d.radthr_bins != e.radthr_bins || d.n_iqr != e.n_iqr || d.radial_blur != e.radial_blur)
        fail("snapshot: defaults");
}

int main() {
    check_pair_texts();
    check_range_texts();
    check_halves_agree();
    check_reachable_states();
    check_snapshot();
    if (g_failures) return 1;
    std::printf("OK\n");
    return 0;
}
