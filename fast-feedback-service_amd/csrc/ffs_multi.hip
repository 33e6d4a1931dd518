// ffs_multi.hip -- several GPUs in one process: ffs_multi_init and the process-wide exchange state (RCCL loaded with dlopen, one
// communicator per distinct device, the choice of transport), the transfer of a batch's packed lists into a 3D stack on another context
// (multi_move_packed, called by ffs_stack3d.hip), the gather of the spot rows (ffs_multi_gather_rows) and ffs_device_numa_node.
// Ranks, the order of the gathered rows and the choice of transport are decided in sweep_plan.hpp.
//
// Frames are independent, so a driver with one context per GPU needs no collective for stills.  A rotation
// sweep does have one exchange: every frame's strong-pixel list has to reach the GPU that owns the 3D stack.
// Transport between two different devices: RCCL point-to-point (ncclSend / ncclRecv inside one group, over
// xGMI) when librccl can be loaded and ffs_multi_init() built the communicators, else hipMemcpyPeerAsync.
// The reference has nothing to compare with: one process, one device (src/ffs/cuda_arg_parser.cc:56-61).
//
// Locking: ffs_multi_init() writes this state under g_multi_mu and must not run while batches are being added;
// the transfers only read it.  What serialises the use of the home rank's communicator is the stack's own mutex
// (every transfer into a stack holds it), and nothing in a transfer waits on the host: the receive (or peer copy)
// is ordered on the stack's stream, which ffs_stack3d_finish uses too.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is loaded with dlopen when several devices are in use

#include "ffs_internal.hpp"

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static std::mutex g_multi_mu;
static RcclApi g_rccl;
static std::vector<int> g_comm_devices;     // distinct devices, rank = position
static std::vector<ncclComm_t> g_comms;     // one communicator per rank (ncclCommInitAll)
static std::atomic<int> g_multi_transport{kTransportNone};
static bool g_want_rccl = true;             // FFS_GATHER / the transport argument, as given to ffs_multi_init
static bool g_gather_forced = false;        // ... explicitly (then RCCL is used even between contexts on one GPU)

static void rccl_load() {   // (a symbol the library does not have stays null)
    g_rccl.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!g_rccl.lib) g_rccl.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!g_rccl.lib) return;
    const struct { const char* name; void* slot; } symbols[] = {
        {"ncclCommInitAll", &g_rccl.CommInitAll}, {"ncclCommDestroy", &g_rccl.CommDestroy}, {"ncclGroupStart", &g_rccl.GroupStart},
        {"ncclGroupEnd", &g_rccl.GroupEnd},       {"ncclSend", &g_rccl.Send},               {"ncclRecv", &g_rccl.Recv},
        {"ncclAllGather", &g_rccl.AllGather},     {"ncclGetErrorString", &g_rccl.GetErrorString}};
    for (const auto& sym : symbols) *static_cast<void**>(sym.slot) = dlsym(g_rccl.lib, sym.name);
}
static std::string rccl_error(const char* what, ncclResult_t r) {
    return std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "failed");
}

extern "C" int ffs_multi_init(const int* devices, int n_devices, const char* transport) {
    if (!devices || n_devices <= 0) return FFS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(g_multi_mu);
    std::vector<int> distinct = distinct_devices(std::vector<int>(devices, devices + n_devices));
    const char* env = std::getenv("FFS_GATHER");   // "rccl" | "peer": how rotation lists travel (results are the same)
    const std::string want = transport ? transport : (env ? env : "rccl");
    g_gather_forced = transport != nullptr || env != nullptr;
    g_want_rccl = want == "rccl";
    if (!g_comms.empty() && distinct == g_comm_devices) {   // the communicators are there already: only the choice of transport may change
        g_multi_transport = reported_transport(g_want_rccl, distinct.size(), true);
        return FFS_OK;
    }
    if (!g_comms.empty() && g_rccl.CommDestroy) {
        for (ncclComm_t cm : g_comms) (void)g_rccl.CommDestroy(cm);
        g_comms.clear();
    }
    g_comm_devices = distinct;
    g_multi_transport = reported_transport(g_want_rccl, distinct.size(), false);
    if (!g_want_rccl) return FFS_OK;
    if (!g_rccl.lib) rccl_load();
    if (!g_rccl.lib || !g_rccl.CommInitAll || !g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
        return FFS_OK;  // no RCCL here: peer copies
    g_comms.assign(distinct.size(), nullptr);
    const ncclResult_t r = g_rccl.CommInitAll(g_comms.data(), (int)distinct.size(), distinct.data());
    if (r != ncclSuccess) {
        g_comms.clear();
        g_create_error = rccl_error("ncclCommInitAll", r);
        return FFS_OK;  // still usable through peer copies; ffs_multi_transport() tells which
    }
    g_multi_transport = reported_transport(g_want_rccl, distinct.size(), true);
    return FFS_OK;
}

extern "C" const char* ffs_multi_transport(void) {   // (string literals: nothing a later ffs_multi_init could invalidate)
    switch (g_multi_transport.load()) {
    case kTransportRccl: return "rccl";
    case kTransportPeer: return "peer";
    default: return "none";
    }
}

// NUMA node of a GPU (sysfs: /sys/bus/pci/devices/<bus id>/numa_node), -1 if unknown: where the driver should keep the
// worker threads that feed it, and their pinned buffers
extern "C" int ffs_device_numa_node(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char* p = bus; *p; ++p) *p = (char)std::tolower((unsigned char)*p);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f) return -1;
    int node = -1;
    if (std::fscanf(f, "%d", &node) != 1) node = -1;
    std::fclose(f);
    return node;
}

// ---- a batch's packed lists into a stack on another context ---------------------------------------------------------------------------------
// The two arrays packed on the stream's device (in s->st2) go to dst_k / dst_i on the home context's device, ordered on the stack's stream
// home_st.  The caller holds the stack's mutex.
int multi_move_packed(ffs_stream* s, ffs_ctx* c, hipStream_t home_st, uint32_t* dst_k, uint32_t* dst_i, uint64_t packed) {
    ffs_ctx* sc = s->ctx;       // source
    const int r_src = rank_of_device(g_comm_devices, sc->device), r_home = rank_of_device(g_comm_devices, c->device);
    if (transfer_uses_rccl(!g_comms.empty(), r_src, r_home, g_want_rccl, sc->device, c->device, g_gather_forced)) {
        // one group: the source rank sends on its stream (behind the pack), the home rank receives on the stack's stream
        ncclResult_t r = g_rccl.GroupStart();
        if (r == ncclSuccess) r = g_rccl.Send(s->d_pack_k, packed, ncclUint32, r_home, g_comms[r_src], s->st2);
        if (r == ncclSuccess) r = g_rccl.Recv(dst_k, packed, ncclUint32, r_src, g_comms[r_home], home_st);
        if (r == ncclSuccess) r = g_rccl.Send(s->d_pack_i, packed, ncclUint32, r_home, g_comms[r_src], s->st2);
        if (r == ncclSuccess) r = g_rccl.Recv(dst_i, packed, ncclUint32, r_src, g_comms[r_home], home_st);
        const ncclResult_t re = g_rccl.GroupEnd();
        if (r == ncclSuccess) r = re;
        if (r != ncclSuccess) return refuse(c->err, FFS_ERR_DEVICE, rccl_error("RCCL send/recv of the strong-pixel lists", r));
        return FFS_OK;
    }
    // peer copy (or plain device-to-device when both contexts sit on one GPU), in the stack's stream, behind the pack
    STK_TRY(c, hipEventRecord(s->ev_pack, s->st2));
    HIP_TRY(c, hipSetDevice(c->device));
    STK_TRY(c, hipStreamWaitEvent(home_st, s->ev_pack, 0));
    if (sc->device == c->device) {
        STK_TRY(c, hipMemcpyAsync(dst_k, s->d_pack_k, packed * 4, hipMemcpyDeviceToDevice, home_st));
        STK_TRY(c, hipMemcpyAsync(dst_i, s->d_pack_i, packed * 4, hipMemcpyDeviceToDevice, home_st));
    } else {
        STK_TRY(c, hipMemcpyPeerAsync(dst_k, c->device, s->d_pack_k, sc->device, packed * 4, home_st));
        STK_TRY(c, hipMemcpyPeerAsync(dst_i, c->device, s->d_pack_i, sc->device, packed * 4, home_st));
    }
    if (s->ev_sent && s->ev_sent_dev != c->device) {   // (an event is recorded in a stream of its own device)
        (void)hipEventDestroy(s->ev_sent);
        s->ev_sent = nullptr;
    }
    if (!s->ev_sent) {
        STK_TRY(c, hipEventCreateWithFlags(&s->ev_sent, hipEventDisableTiming));
        s->ev_sent_dev = c->device;
    }
    STK_TRY(c, hipEventRecord(s->ev_sent, home_st));
    s->sent_pending = true;
    return FFS_OK;
}

// ---- the gather of the per-frame spot lists over RCCL (BASELINE.json north_star) -------------------------
// One process, one context per GPU: after a batch each context holds its reflections' centre rows (frame id, x, y, z) on the host
// (ffs_stream_spot_centres).  The driver can simply read them there (`spotfinder --gather host`); this is the collective the
// north star names, on the communicators ffs_multi_init built: every rank's row count by ncclAllGather, then exactly the written
// rows by ncclSend / ncclRecv inside one group to the root's device, and one copy from there to the host.  Contexts that share a
// GPU share its rank: their rows go out as ONE message (one send per pair of ranks and group: two sends between the same pair were
// matched out of order with their receives in the one-GPU rehearsal).  Scratch per rank's first stream, allocated on first use, freed with it.
struct GatherScratch {
    float* d_rows = nullptr;            // this stream's rows on its device
    size_t rows_cap = 0;
    unsigned long long* d_cnt = nullptr;   // [1] this rank's count | [ranks] everybody's (behind it)
    float* d_all = nullptr;             // root only: every rank's rows, in stream order
    size_t all_cap = 0;
    hipStream_t st = nullptr;
};
static std::mutex g_gather_mu;
static std::map<ffs_stream*, GatherScratch> g_gather;   // (a handful of entries: one per stream that ever took part)

void gather_scratch_free(ffs_stream* s) {
    std::lock_guard<std::mutex> lock(g_gather_mu);
    auto it = g_gather.find(s);
    if (it == g_gather.end()) return;
    GatherScratch& g = it->second;
    if (g.st) (void)hipStreamSynchronize(g.st);
    if (g.d_rows) (void)hipFree(g.d_rows);
    if (g.d_cnt) (void)hipFree(g.d_cnt);
    if (g.d_all) (void)hipFree(g.d_all);
    if (g.st) (void)hipStreamDestroy(g.st);
    g_gather.erase(it);
}

static int multi_gather_rows_impl(ffs_stream* const* streams, uint32_t n, uint32_t root, float* rows4_out, uint32_t cap, uint32_t* n_rows) {
    ffs_ctx* rc = streams[root]->ctx;
    std::lock_guard<std::mutex> lock_multi(g_multi_mu);   // (the communicators are not ours alone: a rotation exchange may want them too)
    if (g_comms.empty() || !g_rccl.AllGather || !g_rccl.Send || !g_rccl.Recv) {
        rc->err = "ffs_multi_gather_rows: no RCCL communicators (ffs_multi_init with transport \"rccl\" first; ffs_multi_transport() tells)";
        return FFS_ERR_INVALID;
    }
    const int n_ranks = (int)g_comms.size();
    std::lock_guard<std::mutex> lock(g_gather_mu);
    // where every stream's rows go (sweep_plan.hpp).  The streams are asked one after the other, as ever: is it busy, then is its device known
    std::vector<int> devices(n);
    std::vector<uint64_t> rows(n);
    uint32_t first_busy = n;
    for (uint32_t i = 0; i < n; ++i) {
        devices[i] = streams[i]->ctx->device;
        rows[i] = streams[i]->centres.size() / 4;
        if (streams[i]->busy && first_busy == n) first_busy = i;
    }
    const GatherLayout lay = gather_layout(devices, rows, g_comm_devices);
    const bool off_comm = lay.refusal == GatherRefusal::kStreamOffCommunicator;
    if (first_busy < n && !(off_comm && lay.refused_stream < first_busy))
        return refuse(rc->err, FFS_ERR_INVALID, "ffs_multi_gather_rows: a stream has a batch in flight (call after ffs_wait)");
    if (off_comm) return refuse(rc->err, FFS_ERR_INVALID, "ffs_multi_gather_rows: a stream's device is not in the communicator");
    if (lay.refusal == GatherRefusal::kRankWithoutStream)
        return refuse(rc->err, FFS_ERR_INVALID, "ffs_multi_gather_rows: every rank of the communicator needs a stream (a collective)");
    const std::vector<uint64_t>&per_rank = lay.per_rank, &rank_at = lay.rank_at;
    const uint64_t total = lay.total;
    if (n_rows) *n_rows = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);
    if (total > cap) { rc->err = "ffs_multi_gather_rows: the rows do not fit `cap`"; return FFS_ERR_OVERFLOW; }
    const int root_rank = lay.rank[root];
    auto scratch_of = [&](int r) -> GatherScratch& { return g_gather[streams[(size_t)lay.leader[(size_t)r]]]; };   // of rank r: its first stream's
    auto device_of = [&](int r) { return streams[(size_t)lay.leader[(size_t)r]]->ctx->device; };
    // scratch of every rank's first stream: one message per rank -- the rows of all its contexts, one behind the other -- and the count
    for (int r = 0; r < n_ranks; ++r) {
        GatherScratch& g = scratch_of(r);
        STK_TRY(rc, hipSetDevice(device_of(r)));
        if (!g.st) STK_TRY(rc, hipStreamCreateWithFlags(&g.st, hipStreamNonBlocking));
        if (!g.d_cnt) STK_TRY(rc, hipMalloc(reinterpret_cast<void**>(&g.d_cnt), (size_t)(1 + n_ranks) * 8 + 256));
        if (per_rank[(size_t)r] > g.rows_cap) {
            STK_TRY(rc, hipStreamSynchronize(g.st));
            if (g.d_rows) (void)hipFree(g.d_rows);
            g.d_rows = nullptr;
            g.rows_cap = per_rank[(size_t)r] + per_rank[(size_t)r] / 2 + 1024;
            STK_TRY(rc, hipMalloc(reinterpret_cast<void**>(&g.d_rows), g.rows_cap * 16));
        }
        if (r == root_rank && total > g.all_cap) {
            STK_TRY(rc, hipStreamSynchronize(g.st));
            if (g.d_all) (void)hipFree(g.d_all);
            g.d_all = nullptr;
            g.all_cap = total + total / 2 + 1024;
            STK_TRY(rc, hipMalloc(reinterpret_cast<void**>(&g.d_all), g.all_cap * 16));
        }
        STK_TRY(rc, hipMemcpyAsync(g.d_cnt, &per_rank[(size_t)r], 8, hipMemcpyHostToDevice, g.st));
    }
    for (uint32_t i = 0; i < n; ++i) {   // every stream's rows onto its rank's device, into the rank's message
        if (!rows[i]) continue;
        GatherScratch& g = scratch_of(lay.rank[i]);
        STK_TRY(rc, hipSetDevice(streams[i]->ctx->device));
        STK_TRY(rc, hipMemcpyAsync(g.d_rows + lay.in_rank[i] * 4, streams[i]->centres.data(), rows[i] * 16, hipMemcpyHostToDevice, g.st));
    }
    {   // counts
        ncclResult_t r = g_rccl.GroupStart();
        for (int k = 0; k < n_ranks && r == ncclSuccess; ++k) {
            GatherScratch& g = scratch_of(k);
            (void)hipSetDevice(device_of(k));
            r = g_rccl.AllGather(g.d_cnt, g.d_cnt + 1, 1, ncclUint64, g_comms[(size_t)k], g.st);
        }
        const ncclResult_t re = g_rccl.GroupEnd();
        if (r != ncclSuccess || re != ncclSuccess)
            return refuse(rc->err, FFS_ERR_DEVICE, rccl_error("ncclAllGather of the row counts", r != ncclSuccess ? r : re));
    }
    // rows: exactly what was written, one message per rank, to the root's device.  The root's own message is a device copy; with the
    // transport forced to RCCL (ffs_multi_init(.., "rccl") / FFS_GATHER) it is sent to its own rank, which a one-GPU box can rehearse.
    GatherScratch& gr = scratch_of(root_rank);
    {
        ncclResult_t r = g_rccl.GroupStart();
        for (int k = 0; k < n_ranks && r == ncclSuccess; ++k) {
            if (!per_rank[(size_t)k] || (k == root_rank && !g_gather_forced)) continue;
            GatherScratch& g = scratch_of(k);
            (void)hipSetDevice(device_of(k));
            r = g_rccl.Send(g.d_rows, per_rank[(size_t)k] * 4, ncclFloat, root_rank, g_comms[(size_t)k], g.st);
            (void)hipSetDevice(rc->device);
            if (r == ncclSuccess) r = g_rccl.Recv(gr.d_all + rank_at[(size_t)k] * 4, per_rank[(size_t)k] * 4, ncclFloat, k, g_comms[(size_t)root_rank], gr.st);
        }
        const ncclResult_t re = g_rccl.GroupEnd();
        if (r != ncclSuccess || re != ncclSuccess)
            return refuse(rc->err, FFS_ERR_DEVICE, rccl_error("ncclSend / ncclRecv of the spot rows", r != ncclSuccess ? r : re));
    }
    STK_TRY(rc, hipSetDevice(rc->device));
    if (per_rank[(size_t)root_rank] && !g_gather_forced)
        STK_TRY(rc, hipMemcpyAsync(gr.d_all + rank_at[(size_t)root_rank] * 4, gr.d_rows, per_rank[(size_t)root_rank] * 16, hipMemcpyDeviceToDevice, gr.st));
    std::vector<unsigned long long> counts((size_t)n_ranks, 0);
    STK_TRY(rc, hipMemcpyAsync(counts.data(), gr.d_cnt + 1, (size_t)n_ranks * 8, hipMemcpyDeviceToHost, gr.st));
    if (total) STK_TRY(rc, hipMemcpyAsync(rows4_out, gr.d_all, total * 16, hipMemcpyDeviceToHost, gr.st));
    for (int r = 0; r < n_ranks; ++r) {   // (the senders' streams too: their scratch is reused by the next gather)
        STK_TRY(rc, hipSetDevice(device_of(r)));
        STK_TRY(rc, hipStreamSynchronize(scratch_of(r).st));
    }
    for (int r = 0; r < n_ranks; ++r)
        if (counts[(size_t)r] != per_rank[(size_t)r]) {
            rc->err = "ffs_multi_gather_rows: the gathered counts differ from what the ranks sent";
            return FFS_ERR_DEVICE;
        }
    return FFS_OK;
}

extern "C" int ffs_multi_gather_rows(ffs_stream* const* streams, uint32_t n_streams, uint32_t root, float* rows4_out, uint32_t cap, uint32_t* n_rows) {
    if (!streams || n_streams == 0 || root >= n_streams || !rows4_out) return FFS_ERR_INVALID;
    for (uint32_t i = 0; i < n_streams; ++i)
        if (!streams[i] || !handle_live(kHandleStream, streams[i])) return FFS_ERR_INVALID;
    return guarded(streams[root]->ctx, [&] { return multi_gather_rows_impl(streams, n_streams, root, rows4_out, cap, n_rows); });
}
