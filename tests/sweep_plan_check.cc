// sweep_plan_check.cc -- the arithmetic of rotation sweeps and of the exchange between GPUs (csrc/sweep_plan.hpp) without a GPU: built and run by
// tests/test_sweep_plan.py (g++ with the address and undefined-behaviour sanitizers, against that header alone).  Every property is held
// against a restatement written here -- sums over the frames where the header keeps a running offset, literals where there are few cases:
//   1. batch placement, exhaustive over 0-4 frames x counts {0, 1, 5} x every overflow mask x local / remote x arrived {0, 7};
//   2. the room rule at its edges, and that every accepted batch is placed inside 32 bits; the growth rule;
//   3. the finish plan: tables, begin[], total, biggest and the launch sizes at their steps and caps;
//   4. record classification;
//   5. the gather layout, exhaustive over 1-4 streams x devices {0, 1, 2} x rows {0, 1, 3} x every communicator order, with both refusals;
//      the places the driver reads (distinct_devices + gather_layout, as host/spotfinder.cc calls them) against the places the library
//      writes, both restated as the two programs computed them before they shared the header;
//   6. the two transport decisions against their truth tables.
// Prints "FAIL ..." lines and a final "OK".
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "sweep_plan.hpp"

using namespace ffsamd;

static int g_failures = 0;
static void fail(const std::string& what) {
    if (++g_failures <= 40) std::printf("FAIL %s\n", what.c_str());
}
static void expect(bool ok, const std::string& what) {
    if (!ok) fail(what);
}
template <typename A, typename B>
static void expect_eq(const A& got, const B& want, const std::string& what) {
    if ((long long)got != (long long)want)   // (every value compared here is below 2^63)
        fail(what + ": got " + std::to_string((long long)got) + ", want " + std::to_string((long long)want));
}
static bool same_row(const StackSlice& a, const StackSlice& b) { return a.src == b.src && a.dst == b.dst && a.n == b.n && a.z == b.z; }

// the intervals [at[i], at[i] + n[i]) tile [from, to): sorted by start, each begins where the one before ended
static bool tiles(std::vector<uint64_t> at, const std::vector<uint64_t>& n, uint64_t from, uint64_t to) {
    std::vector<size_t> order(at.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return at[a] != at[b] ? at[a] < at[b] : n[a] < n[b]; });
    uint64_t cur = from;
    for (size_t i : order) {
        if (at[i] != cur) return false;
        cur += n[i];
    }
    return cur == to;
}

// ---- 1. placement ---------------------------------------------------------------------------------------------------------------------------
static void check_placement_of(uint64_t arrived, const std::vector<BatchFrame>& fr, const std::string& tag) {
    const size_t nf = fr.size();
    const BatchPlacement loc = place_batch(arrived, fr, false), rem = place_batch(arrived, fr, true);
    uint64_t sum = 0, packed = 0;
    uint32_t biggest = 0;
    bool host_lists = false;
    for (const BatchFrame& f : fr) {
        sum += f.n;
        if (!f.overflow) { packed += f.n; biggest = std::max(biggest, f.n); }
        if (f.overflow && f.n) host_lists = true;
    }
    std::vector<uint64_t> counts(nf);
    for (size_t f = 0; f < nf; ++f) counts[f] = fr[f].n;
    for (const BatchPlacement* p : {&loc, &rem}) {
        const std::string t = tag + (p == &loc ? " local" : " remote");
        expect(p->dst.size() == nf && p->table.size() == nf, t + ": sizes");
        if (p->dst.size() != nf || p->table.size() != nf) return;
        expect_eq(p->end, arrived + sum, t + ": end");
        expect_eq(p->packed, packed, t + ": packed");
        expect_eq(p->biggest, biggest, t + ": biggest");
        expect(p->host_lists == host_lists, t + ": host_lists");
        expect(tiles(p->dst, counts, arrived, arrived + sum), t + ": the destinations do not tile [arrived, end)");
        for (size_t f = 0; f < nf; ++f) {
            expect_eq(p->table[f].n, fr[f].overflow ? 0u : fr[f].n, t + ": table n");
            expect(p->table[f].src == 0 && p->table[f].z == 0, t + ": table src / z");
        }
    }
    for (size_t f = 0; f < nf; ++f) {
        uint64_t before = 0, packed_before = 0, overflow_before = 0;
        for (size_t g = 0; g < f; ++g) {
            before += fr[g].n;
            (fr[g].overflow ? overflow_before : packed_before) += fr[g].n;
        }
        expect_eq(loc.dst[f], arrived + before, tag + " local: frame order");
        expect_eq(loc.table[f].dst, arrived + before, tag + " local: table dst is absolute");
        // remote: the packed frames first, in frame order, in [arrived, arrived + packed); the overflow frames behind them, in frame order
        expect_eq(rem.dst[f], fr[f].overflow ? arrived + packed + overflow_before : arrived + packed_before, tag + " remote: place");
        if (!fr[f].overflow) {
            expect(rem.dst[f] + fr[f].n <= arrived + packed, tag + " remote: a packed frame lies outside the packed range");
            expect_eq(rem.table[f].dst, packed_before, tag + " remote: the pack row is the offset in the pack");
            expect_eq(rem.table[f].dst, rem.dst[f] - arrived, tag + " remote: the pack row is dst - arrived");
            expect_eq(rem.table[f].n, loc.table[f].n, tag + " remote: the pack row's n is the local row's");
            if (overflow_before == 0) expect_eq(rem.table[f].dst, loc.table[f].dst - arrived, tag + " remote: pack row = local row - arrived");
        }
    }
}
static void check_placement() {
    const uint32_t counts[3] = {0, 1, 5};
    for (uint64_t arrived : {0ull, 7ull})
        for (int nf = 0; nf <= 4; ++nf) {
            int combos = 1;
            for (int f = 0; f < nf; ++f) combos *= 3;
            for (int cc = 0; cc < combos; ++cc)
                for (int mask = 0; mask < (1 << nf); ++mask) {
                    std::vector<BatchFrame> fr((size_t)nf);
                    std::string tag = "placement arrived " + std::to_string(arrived) + " [";
                    for (int f = 0, c = cc; f < nf; ++f, c /= 3) {
                        fr[(size_t)f] = BatchFrame{counts[c % 3], ((mask >> f) & 1) != 0};
                        tag += std::to_string(fr[(size_t)f].n) + (fr[(size_t)f].overflow ? "o " : " ");
                    }
                    check_placement_of(arrived, fr, tag + "]");
                }
        }
    // a literal: frames of 5, 1 (overflowed), 0, 5 entries behind 7 arrived
    const std::vector<BatchFrame> fr = {{5, false}, {1, true}, {0, false}, {5, false}};
    const BatchPlacement loc = place_batch(7, fr, false), rem = place_batch(7, fr, true);
    expect(loc.dst == std::vector<uint64_t>({7, 12, 13, 13}) && loc.end == 18, "placement literal: local dst");
    expect(rem.dst == std::vector<uint64_t>({7, 17, 12, 12}) && rem.end == 18 && rem.packed == 10, "placement literal: remote dst");
    expect(same_row(loc.table[0], StackSlice{0, 7, 5, 0}) && same_row(loc.table[1], StackSlice{0, 12, 0, 0}) && same_row(loc.table[3], StackSlice{0, 13, 5, 0}),
           "placement literal: local table");
    expect(same_row(rem.table[0], StackSlice{0, 0, 5, 0}) && rem.table[1].n == 0 && same_row(rem.table[3], StackSlice{0, 5, 5, 0}), "placement literal: pack table");
}

// ---- 2. room and growth ---------------------------------------------------------------------------------------------------------------------
static void check_room_and_growth() {
    const uint64_t two32 = 1ull << 32, two30 = 1ull << 30;
    struct Case { uint64_t arrived, more, max_total; bool room; };
    const Case cases[] = {
        {0, two30, 0, true},            {0, two30 + 1, 0, false},        {two30 - 5, 5, 0, true},         {two30 - 5, 6, 0, false},   // 0 means 2^30
        {0, 100, 100, true},            {0, 101, 100, false},            {60, 40, 100, true},             {60, 41, 100, false},       // max_total, + 1
        {0, two32 - 2, 1ull << 33, true}, {0, two32 - 1, 1ull << 33, false}, {two32 - 10, 8, 1ull << 33, true}, {two32 - 10, 9, 1ull << 33, false},   // 2^32 - 2, - 1
        {0, two32 - 2, two32 - 1, true},  {0, two32 - 1, two32 - 1, false},  {0, two32, ~0ull, false},          {0, 0, 0, true},
        {100, 0, 100, true},            {101, 0, 100, false},
    };
    for (const Case& c : cases)
        expect(stack_has_room(c.arrived, c.more, c.max_total) == c.room,
               "room: arrived " + std::to_string(c.arrived) + " more " + std::to_string(c.more) + " max_total " + std::to_string(c.max_total));
    // every accepted batch is placed inside 32 bits: the fullest stack the rule accepts, every small batch, both placements
    const uint32_t counts[3] = {0, 1, 5};
    for (int cc = 0; cc < 27; ++cc)
        for (int mask = 0; mask < 8; ++mask) {
            std::vector<BatchFrame> fr(3);
            uint64_t more = 0;
            for (int f = 0, c = cc; f < 3; ++f, c /= 3) { fr[(size_t)f] = BatchFrame{counts[c % 3], ((mask >> f) & 1) != 0}; more += fr[(size_t)f].n; }
            const uint64_t arrived = two32 - 2 - more;
            expect(stack_has_room(arrived, more, 1ull << 33) && !stack_has_room(arrived + 1, more, 1ull << 33), "room: the fullest stack");
            for (bool remote : {false, true}) {
                const BatchPlacement p = place_batch(arrived, fr, remote);
                for (size_t f = 0; f < 3; ++f) {
                    expect(p.dst[f] + fr[f].n <= 0xFFFFFFFFull, "room: an accepted batch's destination leaves 32 bits");
                    if (!remote) expect_eq((uint64_t)p.table[f].dst, p.dst[f], "room: a table row lost bits");
                }
                expect(p.end <= two32 - 2, "room: end");
            }
        }
    const size_t grow[5][2] = {{0, 1024}, {1, 1024}, {682, 1024}, {683, 1024}, {1024, 1536}};
    for (const auto& g : grow) expect_eq(pool_growth(g[0]), g[1], "growth at " + std::to_string(g[0]));
}

// ---- 3. the finish plan ---------------------------------------------------------------------------------------------------------------------
static void check_finish_tables(const std::vector<HeldSlice>& held, const std::string& tag) {
    const FinishPlan p = plan_finish(held, 512);
    expect(p.table.size() == held.size() && p.begin.size() == held.size() + 1, tag + ": sizes");
    if (p.table.size() != held.size() || p.begin.size() != held.size() + 1) return;
    uint64_t total = 0;
    uint32_t biggest = 0;
    for (size_t z = 0; z < held.size(); ++z) {
        uint64_t before = 0;
        for (size_t y = 0; y < z; ++y) before += held[y].n;
        expect_eq(p.begin[z], before, tag + ": begin");
        expect(same_row(p.table[z], StackSlice{held[z].off, (uint32_t)before, held[z].n, (uint32_t)z}), tag + ": table row " + std::to_string(z));
        total += held[z].n;
        biggest = std::max(biggest, held[z].n);
    }
    expect_eq(p.begin[held.size()], total, tag + ": begin's last entry");
    expect_eq(p.total, total, tag + ": total");
    expect_eq(p.biggest, biggest, tag + ": biggest");
}
static void check_finish() {
    // arrival offsets that are not in frame order; dead entries between them (frame ids added twice left [7, 13) and [20, 30) behind); an
    // empty slice in the middle; one slice; none
    check_finish_tables({{13, 3}, {0, 4}, {4, 3}}, "finish: out of order");
    check_finish_tables({{30, 6}, {0, 7}, {13, 7}}, "finish: dead entries");
    check_finish_tables({{5, 2}, {7, 0}, {0, 5}}, "finish: an empty slice");
    check_finish_tables({{0, 9}}, "finish: one slice");
    check_finish_tables({{3, 0}}, "finish: one empty slice");
    check_finish_tables({}, "finish: no slice");
    expect_eq(plan_finish({{30, 6}, {0, 7}, {13, 7}}, 512).total, 20, "finish: total counts live entries only");
    // launch sizes: N entries in one slice -> chunks of 512, blocks of 256 entries capped at 4096, copy blocks capped at 64, the caps on chunks
    struct Grid { uint32_t N, chunks, entry, gather, reduce, finalize; };
    const Grid grids[] = {
        {1, 1, 1, 1, 1, 1},           {256, 1, 1, 1, 1, 1},          {257, 1, 2, 2, 1, 1},           {512, 1, 2, 2, 1, 1},
        {513, 2, 3, 3, 2, 2},         {16128, 32, 63, 63, 32, 32},   {16129, 32, 64, 64, 32, 32},    {16385, 33, 65, 64, 33, 33},
        {524288, 1024, 2048, 64, 1024, 1024},   {524289, 1025, 2049, 64, 1025, 1024},   {1048576, 2048, 4096, 64, 2048, 1024},
        {1048577, 2049, 4096, 64, 2048, 1024},  {4000000000u, 7812500, 4096, 64, 2048, 1024},
    };
    for (const Grid& g : grids) {
        const FinishPlan p = plan_finish({{0, g.N}}, 512);
        const std::string tag = "finish grids at N = " + std::to_string(g.N);
        expect_eq(p.chunks, g.chunks, tag + ": chunks");
        expect_eq(p.entry_blocks, g.entry, tag + ": entry blocks");
        expect_eq(p.gather_blocks, g.gather, tag + ": gather blocks");
        expect_eq(p.reduce_blocks, g.reduce, tag + ": reduce blocks");
        expect_eq(p.finalize_blocks, g.finalize, tag + ": finalize blocks");
        expect_eq(list_copy_blocks(g.N), g.gather, tag + ": copy blocks");
    }
    expect_eq(list_copy_blocks(0), 0, "copy blocks of an empty list");
    expect_eq(plan_finish({{0, 300}, {300, 700}}, 512).gather_blocks, 3, "finish: gather blocks follow the biggest slice, not the total");
}

// ---- 4. classification ----------------------------------------------------------------------------------------------------------------------
struct Rec { uint32_t pad, flags; };
static void check_classification() {
    struct Case { std::vector<uint32_t> flags; std::vector<int32_t> kept; uint32_t small, spread; };
    const Case cases[] = {
        {{0, 1, 2, 3, 0}, {0, -1, -1, -1, 1}, 2, 1},   // both flags: too small is asked first
        {{1, 2, 3}, {-1, -1, -1}, 2, 1},               // none kept
        {{0, 0, 0}, {0, 1, 2}, 0, 0},                  // all kept
        {{}, {}, 0, 0},
    };
    for (const Case& c : cases) {
        std::vector<Rec> recs;
        for (uint32_t f : c.flags) recs.push_back(Rec{77u, f});
        const RecordClasses got = classify_records(recs.data(), (uint32_t)recs.size());
        expect(got.kept_index == c.kept, "classification: kept_index");
        expect_eq(got.n_too_small, c.small, "classification: too small");
        expect_eq(got.n_too_spread, c.spread, "classification: too spread");
        expect_eq(got.n_kept, std::count_if(c.kept.begin(), c.kept.end(), [](int32_t k) { return k >= 0; }), "classification: kept");
        for (uint32_t comp = 0; comp < recs.size(); ++comp) expect_eq(signal_reflection(got, comp), c.kept[comp], "classification: a signal's reflection");
        expect_eq(signal_reflection(got, (uint32_t)recs.size()), -1, "classification: a component index = n_calc");
        expect_eq(signal_reflection(got, 0xFFFFFFFFu), -1, "classification: a component index beyond n_calc");
    }
}

// ---- 5. the gather layout -------------------------------------------------------------------------------------------------------------------
// where the LIBRARY put stream i's rows before the header: ranks by position in the communicator, one message per rank in stream order
static std::vector<uint64_t> library_places(const std::vector<int>& dev, const std::vector<uint64_t>& rows, const std::vector<int>& comm) {
    std::vector<uint64_t> place(dev.size());
    for (size_t i = 0; i < dev.size(); ++i) {
        const size_t ri = (size_t)(std::find(comm.begin(), comm.end(), dev[i]) - comm.begin());
        uint64_t at = 0;
        for (size_t j = 0; j < dev.size(); ++j) {
            const size_t rj = (size_t)(std::find(comm.begin(), comm.end(), dev[j]) - comm.begin());
            if (rj < ri || (rj == ri && j < i)) at += rows[j];
        }
        place[i] = at;
    }
    return place;
}
// where the DRIVER looked for GPU g's rows before the header: its own ranks (distinct devices in order of appearance), rank after rank, GPU order inside
static std::vector<uint64_t> driver_places(const std::vector<int>& dev, const std::vector<uint64_t>& rows) {
    std::vector<int> distinct, gpu_rank(dev.size());
    for (size_t g = 0; g < dev.size(); ++g) {
        size_t r = 0;
        while (r < distinct.size() && distinct[r] != dev[g]) ++r;
        if (r == distinct.size()) distinct.push_back(dev[g]);
        gpu_rank[g] = (int)r;
    }
    std::vector<uint64_t> row_at(dev.size());
    uint64_t at = 0;
    for (int r = 0; r < (int)dev.size(); ++r)
        for (size_t g = 0; g < dev.size(); ++g)
            if (gpu_rank[g] == r) { row_at[g] = at; at += rows[g]; }
    return row_at;
}
static void check_gather_of(const std::vector<int>& dev, const std::vector<uint64_t>& rows) {
    const size_t n = dev.size();
    std::vector<int> present;
    for (int d = 0; d <= 2; ++d)
        if (std::find(dev.begin(), dev.end(), d) != dev.end()) present.push_back(d);
    std::string tag = "gather [";
    for (size_t i = 0; i < n; ++i) tag += std::to_string(dev[i]) + ":" + std::to_string(rows[i]) + " ";
    uint64_t sum = 0;
    for (uint64_t r : rows) sum += r;
    std::vector<int> comm = present;   // (sorted: the first permutation)
    do {
        std::string t = tag + "] comm";
        for (int d : comm) t += " " + std::to_string(d);
        const GatherLayout g = gather_layout(dev, rows, comm);
        expect(g.refusal == GatherRefusal::kNone, t + ": refused");
        if (g.refusal != GatherRefusal::kNone) continue;
        expect_eq(g.total, sum, t + ": total");
        const std::vector<uint64_t> want = library_places(dev, rows, comm);
        std::vector<uint64_t> got(n);
        for (size_t i = 0; i < n; ++i) {
            got[i] = g.row_at(i);
            expect_eq(got[i], want[i], t + ": place of stream " + std::to_string(i));
            expect_eq(comm[(size_t)g.rank[i]], dev[i], t + ": rank");
            expect_eq(g.row_at(i), g.rank_at[(size_t)g.rank[i]] + g.in_rank[i], t + ": row_at");
        }
        expect(tiles(got, rows, 0, sum), t + ": the places do not tile [0, total)");
        for (size_t r = 0; r < comm.size(); ++r) {
            uint64_t per = 0;
            int leader = -1;
            for (size_t i = 0; i < n; ++i)
                if (dev[i] == comm[r]) { per += rows[i]; if (leader < 0) leader = (int)i; }
            expect_eq(g.per_rank[r], per, t + ": per_rank");
            expect_eq(g.leader[r], leader, t + ": leader");
            expect_eq(g.rank_at[r + 1] - g.rank_at[r], per, t + ": rank_at");
        }
        // the two refusals: a communicator with a device no stream is on, and one without the device of some stream
        std::vector<int> more = comm;
        more.insert(more.begin() + (long)(comm.size() / 2), 7);
        expect(gather_layout(dev, rows, more).refusal == GatherRefusal::kRankWithoutStream, t + " + 7: not refused for the rank without a stream");
        std::vector<int> fewer(comm.begin(), comm.end() - 1);
        const GatherLayout off = gather_layout(dev, rows, fewer);
        const size_t first_off = (size_t)(std::find(dev.begin(), dev.end(), comm.back()) - dev.begin());
        expect(off.refusal == GatherRefusal::kStreamOffCommunicator && off.refused_stream == first_off, t + " - last: not refused at the first stream off it");
    } while (std::next_permutation(comm.begin(), comm.end()));
    // the driver: its communicator is what ffs_multi_init makes of its device list, and it reads GPU g's rows at row_at(g)
    const std::vector<int> driver_comm = distinct_devices(dev);
    const GatherLayout g = gather_layout(dev, rows, driver_comm);
    const std::vector<uint64_t> lib = library_places(dev, rows, driver_comm), drv = driver_places(dev, rows);
    for (size_t i = 0; i < n; ++i) {
        expect_eq(g.row_at(i), lib[i], tag + "]: the driver's place is not the library's");
        expect_eq(g.row_at(i), drv[i], tag + "]: the driver's place is not where it used to look");
        expect_eq(rank_of_device(driver_comm, dev[i]), g.rank[i], tag + "]: rank_of_device");
    }
    if (present.size() == 1) {   // all on one device (what the GPU tests see): stream order
        uint64_t at = 0;
        for (size_t i = 0; i < n; ++i) { expect_eq(g.row_at(i), at, tag + "]: one device is stream order"); at += rows[i]; }
    }
}
static void check_gather() {
    const uint64_t row_choices[3] = {0, 1, 3};
    for (int n = 1; n <= 4; ++n) {
        int combos = 1;
        for (int i = 0; i < n; ++i) combos *= 9;
        for (int cc = 0; cc < combos; ++cc) {
            std::vector<int> dev((size_t)n);
            std::vector<uint64_t> rows((size_t)n);
            for (int i = 0, c = cc; i < n; ++i, c /= 9) { dev[(size_t)i] = c % 3; rows[(size_t)i] = row_choices[(c / 3) % 3]; }
            check_gather_of(dev, rows);
        }
    }
    expect(distinct_devices({1, 0, 1}) == std::vector<int>({1, 0}) && distinct_devices({2, 2, 0, 2, 1, 0}) == std::vector<int>({2, 0, 1}) && distinct_devices({}).empty(),
           "distinct_devices: order of first appearance");
    // streams on devices 1, 0, 1 with 2, 5 and 7 rows
    const GatherLayout a = gather_layout({1, 0, 1}, {2, 5, 7}, {1, 0});
    expect(a.refusal == GatherRefusal::kNone && a.rank == std::vector<int>({0, 1, 0}) && a.leader == std::vector<int>({0, 1}) &&
               a.in_rank == std::vector<uint64_t>({0, 0, 2}) && a.per_rank == std::vector<uint64_t>({9, 5}) && a.rank_at == std::vector<uint64_t>({0, 9, 14}) &&
               a.total == 14 && a.row_at(0) == 0 && a.row_at(1) == 9 && a.row_at(2) == 2,
           "gather literal: devices 1,0,1 in communicator [1,0]");
    const GatherLayout b = gather_layout({1, 0, 1}, {2, 5, 7}, {0, 1});
    expect(b.refusal == GatherRefusal::kNone && b.rank == std::vector<int>({1, 0, 1}) && b.leader == std::vector<int>({1, 0}) &&
               b.in_rank == std::vector<uint64_t>({0, 0, 2}) && b.per_rank == std::vector<uint64_t>({5, 9}) && b.rank_at == std::vector<uint64_t>({0, 5, 14}) &&
               b.total == 14 && b.row_at(0) == 5 && b.row_at(1) == 0 && b.row_at(2) == 7,
           "gather literal: devices 1,0,1 in communicator [0,1]");
    const GatherLayout off = gather_layout({0, 2, 3}, {1, 1, 1}, {0, 1});   // both apply: the stream off the communicator is found first
    expect(off.refusal == GatherRefusal::kStreamOffCommunicator && off.refused_stream == 1, "gather literal: a stream's device is not in the communicator");
    expect(gather_layout({0, 0}, {1, 1}, {0, 1}).refusal == GatherRefusal::kRankWithoutStream, "gather literal: every rank needs a stream");
}

// ---- 6. transport ---------------------------------------------------------------------------------------------------------------------------
static void check_transport() {
    // (wanted rccl, distinct devices, communicators) -> what ffs_multi_transport says
    struct Case { bool want; size_t n; bool comms; Transport t; };
    const Case cases[] = {
        {false, 1, false, kTransportNone}, {false, 1, true, kTransportNone}, {false, 2, false, kTransportPeer}, {false, 2, true, kTransportPeer},
        {true, 1, false, kTransportNone},  {true, 1, true, kTransportRccl},  {true, 2, false, kTransportPeer},  {true, 2, true, kTransportRccl},
        {true, 8, false, kTransportPeer},  {false, 8, true, kTransportPeer},
    };
    for (const Case& c : cases)
        expect(reported_transport(c.want, c.n, c.comms) == c.t,
               "reported transport: want " + std::to_string(c.want) + " devices " + std::to_string(c.n) + " comms " + std::to_string(c.comms));
    expect(kTransportNone == 0 && kTransportPeer == 1 && kTransportRccl == 2, "transport values");
    // bits of the index, high to low: communicators, source in it, home in it, rccl wanted, two devices, forced
    const std::string table = std::string(60, '0') + "0111";
    for (int i = 0; i < 64; ++i) {
        const bool comms = i & 32, src = i & 16, home = i & 8, want = i & 4, two = i & 2, forced = i & 1;
        const bool got = transfer_uses_rccl(comms, src ? (two ? 1 : 0) : -1, home ? 0 : -1, want, two ? 1 : 0, 0, forced);
        expect(got == (table[(size_t)i] == '1'), "transfer_uses_rccl at row " + std::to_string(i));
    }
}

int main() {
    check_placement();
    check_room_and_growth();
    check_finish();
    check_classification();
    check_gather();
    check_transport();
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
