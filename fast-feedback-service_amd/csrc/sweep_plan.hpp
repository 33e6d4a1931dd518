// sweep_plan.hpp -- the arithmetic of a rotation sweep and of the exchange between GPUs, without HIP: how the stack's buffers grow and when
// they are full, where a batch's strong-pixel lists land in the arrival buffers, the tables and launch sizes of ffs_stack3d_finish, which
// records become reflections, in which order the rows of ffs_multi_gather_rows arrive, and which transport a transfer takes.
// ffs_stack3d.hip and ffs_multi.hip allocate, copy and launch from what is decided here; host/spotfinder.cc reads the gathered rows by the
// same gather_layout the library writes them by.  A plain C++ test program (tests/sweep_plan_check.cc) holds every rule against a
// restatement over small exhaustive spaces.  DESIGN.md section 3.5.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ffsamd {

// One row of the 3D stack's copy tables (kernels_stack3d.hpp)
struct StackSlice {
    uint32_t src;   // offset in the arrival buffers (k_stack_gather) / in the stream's list of that frame (k_stack_append)
    uint32_t dst;   // offset in the destination buffers
    uint32_t n;     // entries
    uint32_t z;     // k_stack_gather: position of the slice in the stack
};

// Why a component is no reflection (filter_reflections): WireRec2::npx_flags >> 30 and ReflOut::flags
constexpr uint32_t kRecTooSmall = 1u;     // fewer pixels than min_spot_size
constexpr uint32_t kRecTooSpread = 2u;    // peak further than max_sep from the centre of mass

// ---- the stack's buffers ------------------------------------------------------------------------------------------------------------------
// a buffer too small for n entries is reallocated with this many
inline size_t pool_growth(size_t n) { return std::max<size_t>(n + n / 2, 1024); }

// Room for `more` entries behind the `arrived` ones (max_total as given to ffs_stack3d_create: 0 means 2^30).  Everything below that narrows a
// place in the arrival buffers to 32 bits does so for a batch this function accepted: arrived + more <= 2^32 - 2.
inline bool stack_has_room(uint64_t arrived, uint64_t more, uint64_t max_total) {
    const uint64_t limit = max_total ? max_total : (1ull << 30);
    return !(arrived + more > limit || arrived + more >= (1ull << 32) - 1);
}

// blocks of 256 threads along a list of `biggest` entries (k_stack_append, k_stack_gather: grid x; y is the frame or slice)
inline uint32_t list_copy_blocks(uint32_t biggest) { return std::min<uint32_t>(64, (biggest + 255) / 256); }

// ---- where a batch's lists land -----------------------------------------------------------------------------------------------------------
struct BatchFrame {
    uint32_t n;      // strong pixels of the frame
    bool overflow;   // it overflowed the stream's lists: its list is on the host (re-run on the one-frame stream), not in the device lists
};
struct BatchPlacement {
    std::vector<uint64_t> dst;       // per frame: its first entry in the arrival buffers; together the frames tile [arrived, end)
    std::vector<StackSlice> table;   // per frame, k_stack_append's row: n = 0 for an overflow frame, src and z 0; dst is absolute for a local
                                     // batch, and counted from `arrived` (= the offset in the pack) for a remote one
    uint64_t end = 0;                // `arrived` after the batch
    uint64_t packed = 0;             // entries of the frames that did not overflow
    uint32_t biggest = 0;            // ... and the longest of their lists
    bool host_lists = false;         // an overflow frame has entries: they go up from the host
};
// Local: frame order.  Remote: the frames that did not overflow are packed end to end on the source device and arrive in one transfer, so they
// come first, [arrived, arrived + packed), and the overflow frames' entries are placed behind them.
inline BatchPlacement place_batch(uint64_t arrived, const std::vector<BatchFrame>& frames, bool remote) {
    BatchPlacement p;
    p.dst.resize(frames.size());
    p.table.resize(frames.size());
    uint64_t at = arrived;
    for (int pass = 0; pass < 2; ++pass)   // remote: pass 0 places the packed frames, pass 1 the overflow frames; local: pass 0 places all
        for (size_t f = 0; f < frames.size(); ++f) {
            if (remote ? frames[f].overflow != (pass == 1) : pass == 1) continue;
            p.dst[f] = at;
            at += frames[f].n;
        }
    p.end = at;
    for (size_t f = 0; f < frames.size(); ++f) {
        const BatchFrame& fr = frames[f];
        p.table[f] = StackSlice{0u, (uint32_t)(p.dst[f] - (remote ? arrived : 0)), fr.overflow ? 0u : fr.n, 0u};
        if (fr.overflow) p.host_lists = p.host_lists || fr.n != 0;
        else { p.packed += fr.n; p.biggest = std::max(p.biggest, fr.n); }
    }
    return p;
}

// ---- ffs_stack3d_finish -------------------------------------------------------------------------------------------------------------------
struct HeldSlice {
    uint32_t off, n;   // where the frame's list lies in the arrival buffers (a frame added twice: the later list; the earlier one stays there, dead)
};
struct FinishPlan {
    std::vector<StackSlice> table;   // k_stack_gather's rows: src = arrival offset, dst = place in (z, k) order, n, z = rank of the frame id
    std::vector<uint32_t> begin;     // [slices + 1] the running sum of n: where each slice starts
    uint64_t total = 0;              // entries of the held slices
    uint32_t biggest = 0;            // the longest slice
    uint32_t chunks = 0;             // chunks of root_chunk entries
    uint32_t entry_blocks = 0;       // grids: k_union, k_stack_labels
    uint32_t gather_blocks = 0;      // k_stack_gather (x)
    uint32_t reduce_blocks = 0;      // k_reduce_roots3d
    uint32_t finalize_blocks = 0;    // k_finalize_roots3d
};
// `slices` in frame-id order (z = position); root_chunk: kRootChunk of the kernels
inline FinishPlan plan_finish(const std::vector<HeldSlice>& slices, uint32_t root_chunk) {
    FinishPlan p;
    p.table.reserve(slices.size());
    p.begin.reserve(slices.size() + 1);
    for (const HeldSlice& s : slices) {
        p.begin.push_back((uint32_t)p.total);
        p.table.push_back(StackSlice{s.off, (uint32_t)p.total, s.n, (uint32_t)p.table.size()});
        p.biggest = std::max(p.biggest, s.n);
        p.total += s.n;
    }
    p.begin.push_back((uint32_t)p.total);
    p.chunks = (uint32_t)((p.total + root_chunk - 1) / root_chunk);
    p.entry_blocks = (uint32_t)std::min<uint64_t>(4096, (p.total + 255) / 256);
    p.gather_blocks = list_copy_blocks(p.biggest);
    p.reduce_blocks = std::min<uint32_t>(p.chunks, 2048u);
    p.finalize_blocks = std::min<uint32_t>(p.chunks, 1024u);
    return p;
}

// Which records are reflections: kept_index[q] is record q's place among the kept ones, -1 for a filtered one (too small is asked first)
struct RecordClasses {
    std::vector<int32_t> kept_index;
    uint32_t n_kept = 0, n_too_small = 0, n_too_spread = 0;
};
template <typename Rec>
inline RecordClasses classify_records(const Rec* recs, uint32_t n_calc) {
    RecordClasses c;
    c.kept_index.assign(n_calc, -1);
    for (uint32_t q = 0; q < n_calc; ++q) {
        if (recs[q].flags & kRecTooSmall) ++c.n_too_small;
        else if (recs[q].flags & kRecTooSpread) ++c.n_too_spread;
        else c.kept_index[q] = (int32_t)c.n_kept++;
    }
    return c;
}
// the reflection of a signal whose component is `comp` (-1: none)
inline int32_t signal_reflection(const RecordClasses& c, uint32_t comp) { return comp < c.kept_index.size() ? c.kept_index[comp] : -1; }

// ---- the exchange: ranks, and where a stream's rows arrive ----------------------------------------------------------------------------------
// the distinct devices in order of first appearance: a device's rank in the communicator is its position here (ffs_multi_init)
inline std::vector<int> distinct_devices(const std::vector<int>& devices) {
    std::vector<int> distinct;
    for (int d : devices)
        if (std::find(distinct.begin(), distinct.end(), d) == distinct.end()) distinct.push_back(d);
    return distinct;
}
inline int rank_of_device(const std::vector<int>& comm_devices, int device) {
    const auto it = std::find(comm_devices.begin(), comm_devices.end(), device);
    return it == comm_devices.end() ? -1 : (int)(it - comm_devices.begin());
}

enum class GatherRefusal { kNone = 0, kStreamOffCommunicator, kRankWithoutStream };
// ffs_multi_gather_rows: streams that share a device share its rank and their rows go out as one message, so the rows arrive rank after rank
// and, inside a rank, stream after stream.
struct GatherLayout {
    GatherRefusal refusal = GatherRefusal::kNone;
    size_t refused_stream = 0;        // kStreamOffCommunicator: the first stream whose device the communicator does not have
    std::vector<int> rank;            // per stream
    std::vector<int> leader;          // per rank: its first stream (holds the rank's send buffer and count)
    std::vector<uint64_t> in_rank;    // per stream: where its rows start inside its rank's message
    std::vector<uint64_t> per_rank;   // per rank: rows of its message
    std::vector<uint64_t> rank_at;    // [ranks + 1] where a rank's message starts in the gathered table
    uint64_t total = 0;
    uint64_t row_at(size_t stream) const { return rank_at[(size_t)rank[stream]] + in_rank[stream]; }   // the stream's first row in the table
};
inline GatherLayout gather_layout(const std::vector<int>& stream_devices, const std::vector<uint64_t>& rows, const std::vector<int>& comm_devices) {
    const size_t n = stream_devices.size(), n_ranks = comm_devices.size();
    GatherLayout g;
    g.rank.assign(n, -1);
    g.leader.assign(n_ranks, -1);
    g.in_rank.assign(n, 0);
    g.per_rank.assign(n_ranks, 0);
    g.rank_at.assign(n_ranks + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const int r = g.rank[i] = rank_of_device(comm_devices, stream_devices[i]);
        if (r < 0) { g.refusal = GatherRefusal::kStreamOffCommunicator; g.refused_stream = i; return g; }
        if (g.leader[(size_t)r] < 0) g.leader[(size_t)r] = (int)i;
        g.in_rank[i] = g.per_rank[(size_t)r];
        g.per_rank[(size_t)r] += rows[i];
    }
    for (size_t r = 0; r < n_ranks; ++r) {
        if (g.leader[r] < 0) { g.refusal = GatherRefusal::kRankWithoutStream; return g; }   // (a collective: every rank takes part)
        g.rank_at[r + 1] = g.rank_at[r] + g.per_rank[r];
    }
    g.total = g.rank_at[n_ranks];
    return g;
}

// ---- which transport ------------------------------------------------------------------------------------------------------------------------
enum Transport { kTransportNone = 0, kTransportPeer = 1, kTransportRccl = 2 };
// what ffs_multi_transport reports after an ffs_multi_init that wanted RCCL or not, over n_distinct devices, with communicators or without
inline Transport reported_transport(bool want_rccl, size_t n_distinct, bool have_comms) {
    if (want_rccl && have_comms) return kTransportRccl;
    return n_distinct > 1 ? kTransportPeer : kTransportNone;
}
// whether a batch's lists go from src_device to home_device by RCCL send / recv (ranks: rank_of_device, -1 = not in the communicator);
// `forced`: the transport was given explicitly, and then RCCL is used even between contexts on one GPU
inline bool transfer_uses_rccl(bool have_comms, int rank_src, int rank_home, bool want_rccl, int src_device, int home_device, bool forced) {
    return have_comms && rank_src >= 0 && rank_home >= 0 && want_rccl && (src_device != home_device || forced);
}

}  // namespace ffsamd
