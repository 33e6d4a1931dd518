// ffs_internal.hpp -- what the translation units of libffs_hip.so share: the structs behind the opaque handles of
// include/ffs_hip.h, error plumbing, and the few functions one unit calls in another.  Host side only; the kernels
// live in kernels_*.hpp, each included by exactly one unit:
//   ffs_context.hip  contexts, masks (kernels_mask.hpp), the setters of parameters, scope, gain, gain map and calibration, tuning, streams
//   ffs_submit.hip   one batch (enqueue_batch: plan_batch decides its path once, a BatchPlan with the launch geometry and the threshold route; then the resets,
//                    the threshold stage and the sparse stage are launched from that plan), ffs_submit and ffs_submit_device
//                    (kernels_stream / threshold / extended / window / ccl / chain / band)
//   ffs_encoded.hip  encoded input from entry point to teardown: bitshuffle-LZ4, CBF byte-offset and raw Jungfrau chunks are staged, decoded on the
//                    device (kernels_decode / byteoffset / jungfrau) and handed to enqueue_batch; acts on the decisions of encoded_plan.hpp
//   ffs_products.hip the per-frame products, each from its setter to its accessor: the radial profile, the radial-profile threshold, the per-pixel
//                    statistics (kernels_radial / radthr / pixstats); ffs_submit.hip calls their launches at their places in a batch
//   ffs_wait.hip     ffs_wait: overflow re-runs (rerun_batch: the same batch again with a Rerun override), result assembly,
//                    result accessors
//   ffs_spotbg.hip   ffs_stream_spot_backgrounds: the per-spot constant background of the last waited batch (kernels_spotbg.hpp)
//   ffs_shoebox.hip  summation integration of shoeboxes in Kabsch space, from begin to end: the job on a context, ffs_stream_shoebox_fold, the sums
//                    (kernels_shoebox.hpp); acts on the decisions of shoebox_plan.hpp
//   ffs_predict.hip  scan prediction for a rotation sweep: ffs_predict_scan_settings and ffs_ctx_predict, a count pass, a scan and a write pass
//                    in a HIP stream of the call's own (kernels_predict.hpp); acts on the decisions of predict_plan.hpp
//   ffs_index.hip    the indexer's basis-vector search: the host-only ffs_index_* entries and ffs_ctx_index_grid / index_load_grid / index_peaks --
//                    scatter, three FFT passes, the statistics' trees, selection, union-find, per-root sums and records in a HIP stream of
//                    the call's own (kernels_index.hpp); acts on the decisions of index_plan.hpp
//   ffs_assign.hip   index assignment for candidate crystal settings: the host-only ffs_index_select / settings / absence_table / absence_detect /
//                    reindex and ffs_ctx_index_assign -- assign with a key table, place, fill, resolve the duplicates, reduce, pass by pass in a
//                    HIP stream of the call's own (kernels_assign.hpp); acts on the decisions of assign_plan.hpp
//   ffs_stack3d.hip  rotation sweeps: the device-resident 3D stack -- create and pool, append a batch's lists, finish (kernels_stack3d); acts on
//                    the decisions of sweep_plan.hpp
//   ffs_multi.hip    several GPUs in one process: RCCL loaded with dlopen, the communicators and the choice of transport (ffs_multi_init), the
//                    transfer of a batch's packed lists into a stack on another context, ffs_multi_gather_rows, ffs_device_numa_node; no kernels
//   ffs_bench.hip    measurement entry points (kernel timings, memory ceiling, native pipeline loop, sqrt self-test)
// Without HIP, shared with the kernels through ffs_device.h and compiled by a plain C++ test (tests/launch_geometry_check.cc):
//   launch_geometry.hpp  the frame layout, the launch geometry of the threshold stage (super rows, strips, bands; wave logs and band
//                        slots a launch needs), the unit map the kernels invert, the row bands and the pixel-count rule of the per-frame products
//   threshold_route.hpp  the predicate's variants, which instantiation of a kernel family serves one, and a batch's route through the
//                        threshold stage (tests/threshold_route_check.cc)
//   tuning.hpp           struct Tuning
//   context_settings.hpp  a context's settings (ContextSettings, ffs_ctx::settings), the rules every ffs_ctx_set_* asks before it changes anything --
//                        ranges, and the pairs of settings that do not combine, each stated once for both of its setters -- and what a batch
//                        takes of the settings at submit (ParamSnapshot, snapshot_of) (tests/context_settings_check.cc)
//   spot_background_model.hpp  the decisions of the per-spot background: quartile positions, status order, fence (tests/spot_background_check.cc)
//   spot_background_glm_model.hpp  the robust Poisson GLM of the same ring: status order, seed, IRLS step, its own exp and log (tests/spot_background_glm_check.cc)
//   radial_threshold_model.hpp the decisions of the radial-profile threshold (kernels_radthr.hpp, included by ffs_products.hip): status order and the
//                        cutoff's two separately rounded operations (tests/radial_threshold_check.cc)
//   encoded_plan.hpp     the decisions about a batch of encoded frames: bitshuffle's blocking, the chunk checks, where the chunks lie in the
//                        staging buffer and which ranges of it are copied, the block table, the byte-offset frame table (tests/encoded_plan_check.cc)
//   sweep_plan.hpp       rotation sweeps and the exchange (StackSlice lives here): the stack's growth and room rules, where a batch's lists land
//                        and its append table, the finish's tables and launch sizes, which records are reflections, ranks and the order of the
//                        gathered rows (host/spotfinder.cc reads them by the same function), the two transport decisions (tests/sweep_plan_check.cc)
//   radial_blur_model.hpp  the blur ahead of that threshold (ffs_ctx_set_radial_blur): weights, tap rule, v = S / Wn (tests/radial_blur_check.cc)
//   jungfrau_model.hpp   raw Jungfrau words to photon counts (ffs_ctx_set_jungfrau_calibration, FFS_CODEC_JUNGFRAU_RAW): stage, invalid words, the
//                        two float32 operations, rounding and clamp; the setter's ranges (kernels_jungfrau.hpp, included by ffs_encoded.hip;
//                        host/codecs.hpp; tests/jungfrau_check.cc)
//   jungfrau_pedestal_model.hpp  pedestals from dark frames (ffs_stream_jungfrau_pedestal_fold, ffs_jungfrau_pedestal_planes): which words count
//                        where, accumulators to pedestal / rms / ok planes, the re-pedestalled calibration (kernels_jfped.hpp, included by
//                        ffs_encoded.hip, which owns the fold from begin to end; host/codecs.hpp; tools/ffs_hosttool.cc; tests/jungfrau_pedestal_check.cc)
//   shoebox_model.hpp    summation integration: corner to Kabsch coordinates, the foreground decision, what a pixel adds to its reflection, the
//                        final sums (kernels_shoebox.hpp, included by ffs_shoebox.hip; tools/ffs_hosttool.cc; tests/shoebox_check.cc)
//   shoebox_plan.hpp     which shoebox tables are taken, the index over the boxes' z-ranges and the list a fold's launch receives
//                        (tests/shoebox_plan_check.cc)
//   predict_model.hpp    scan prediction: scan-point settings, candidate numbering and centring absences, the per-image ray, the impact on the
//                        panel and the extent in Kabsch space (kernels_predict.hpp, included by ffs_predict.hip; tools/ffs_hosttool.cc;
//                        tests/predict_check.cc)
//   predict_plan.hpp     which prediction calls are taken, the candidate box, the call's constants, the scan-point settings from libm's cos and
//                        sin, the whole rule on the CPU (tests/predict_plan_check.cc)
//   index_model.hpp      the indexer's basis-vector search: spot to reciprocal-lattice point, the map on the grid, the FFT's schedule, the
//                        statistics' tree, components and their records, the filter and the candidate vectors (kernels_index.hpp, included by
//                        ffs_index.hip; tools/ffs_hosttool.cc; tests/index_check.cc)
//   index_plan.hpp       which index calls are taken, the device buffers' sizes per n_points and the launches' shapes (tests/index_plan_check.cc)
//   assign_model.hpp     index assignment: the inverse by cofactors, a spot's index under a setting and its word, the duplicates' pair rule, the
//                        integer counts, the absence table, detect, reindex, selection and the settings from basis vectors (kernels_assign.hpp,
//                        included by ffs_assign.hip; tools/ffs_hosttool.cc; tests/assign_check.cc)
//   assign_plan.hpp      which assignment calls are taken, the settings a pass takes under workspace_bytes, the launches' shapes and the bytes
//                        of device state (tests/assign_plan_check.cc)
// No exception leaves the library (guarded()).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "ffs_hip.h"
#include "ffs_device.h"
#include "context_settings.hpp"
#include "encoded_plan.hpp"
#include "radial_threshold_model.hpp"
#include "threshold_route.hpp"
#include "tuning.hpp"

using namespace ffsamd;

// ---- errors ---------------------------------------------------------------------------------------------------
extern thread_local std::string g_create_error;   // ffs_last_error(NULL): failures before a context exists

// Error text is kept per calling thread (several worker threads drive their own streams of one
// context; a shared std::string would be a data race exactly when things go wrong).  `ctx->err = ...`
// and `ctx->err.c_str()` keep reading naturally at the call sites.
struct ThreadError {
    static std::string& text() {
        static thread_local std::string t;
        return t;
    }
    const ThreadError& operator=(const std::string& m) const { text() = m; return *this; }
    const ThreadError& operator=(const char* m) const { text() = m; return *this; }
    const char* c_str() const { return text().c_str(); }
    operator std::string() const { return text(); }
};

// ---- tuning: struct Tuning, tuning.hpp ---------------------------------------------------------------------------

struct ffs_stack3d;
struct ShoeboxJob;   // ffs_shoebox.hip
struct PredictState; // ffs_predict.hip
struct IndexState;   // ffs_index.hip
struct AssignState;  // ffs_assign.hip

// A few helper threads per context for ffs_wait's result assembly (wire records -> boxes, reflections, centre rows): one thread
// moves a batch's 7 MB (45 000 components of 32 Eiger frames) in 0.21 ms -- two thirds of the time the GPU takes for the batch, and
// the last waits of a run pay it on the clock.  Frames are independent (their slices of the output arrays follow from the
// per-frame summaries), so the caller and the helpers take frames off a shared counter.  Created on the first large batch; a
// wait that finds the pool busy (another stream's wait is using it) assembles on its own.
struct AssemblyPool {
    std::vector<std::thread> threads;
    std::mutex mu;                       // guards job / generation / stop
    std::condition_variable cv;
    std::mutex owner;                    // one wait at a time uses the helpers
    const std::function<void(uint32_t)>* job = nullptr;
    uint32_t n_items = 0;
    std::atomic<uint32_t> next{0}, done{0};
    std::atomic<int> active{0};          // helpers inside the current job (run() does not return before they have left it)
    uint64_t generation = 0;
    bool stop = false;
    void start(int n_threads);
    void run(uint32_t n, const std::function<void(uint32_t)>& fn);   // fn(i) for i in [0, n), on the caller and the helpers
    void stop_and_join();                // the helpers leave (after the job they are in) and are joined; run() then works on the caller alone
    ~AssemblyPool();
};

// A staging area the DMA engines can read: anonymous memory on transparent huge pages, registered with the runtime
// (tools/ubench/pin_cost.hip: 17 ms per 256 MB against 54 + 26 ms to allocate and free the same with hipHostMalloc, same
// 57 GB/s to the device); hipHostMalloc when registering is refused.
struct PinnedBuf {
    uint8_t* p = nullptr;      // the usable area (2 MiB aligned when mapped)
    size_t bytes = 0;
    void* map_base = nullptr;  // mmap'ed region (null: p came from hipHostMalloc)
    size_t map_len = 0;
};
PinnedBuf pinned_alloc(size_t bytes);   // p == nullptr on failure
void pinned_free(PinnedBuf& b);

// One thread per context that assembles the results of the context's batches as the GPU finishes them (ffs_wait.hip): ffs_wait then
// finds a batch's arrays ready instead of spending 0.1-0.2 ms on them -- which the waits at the END of a run, one behind the other
// with nothing left to hide them, paid on the clock.  Only batches that need nothing else from the host (no overflow, no list or
// mask copies); everything else is left to the caller's ffs_wait as before.
struct AheadThread {
    std::thread th;
    std::mutex mu;                 // guards q, stop and every stream's ahead_state
    std::condition_variable cv_work, cv_done;
    std::deque<ffs_stream*> q;     // registered batches, in submit order
    bool stop = false;
};

struct ffs_ctx {
    int device = 0;
    Tuning tune;
    Layout L{};
    ContextSettings settings;   // what the ffs_ctx_set_* calls have stored (context_settings.hpp); snapshot per batch
    uint32_t max_batch = 1;
    uint32_t cap = 0;       // strong pixels per frame
    uint32_t max_comp = 0;  // components per frame
    int n_tiles = 0;
    // ffs_ctx_set_gain_map: [H][pitch_px] float32, allocated at the first set and kept (entries beyond W are 1); settings.gain_map says whether
    // it is in force, gain_map_min / _max are the extremes of its W * H entries (what the screens' per-batch switches are decided from)
    float* d_gain_map = nullptr;
    float gain_map_min = 0.0f, gain_map_max = 0.0f;
    // ffs_ctx_set_jungfrau_calibration: six dense planes of jf_plane_stride floats (W * H rounded up to 8, so that the
    // kernel's last group loads inside them), pedestal G0 G1 G2 then factor G0 G1 G2, allocated at the first set and kept;
    // settings.jungfrau_calibration says whether one is in force.  Written only while no batch of the context is in flight.
    float* d_jf_cal = nullptr;
    size_t jf_plane_stride = 0;
    // ffs_ctx_jungfrau_pedestal_begin: the accumulators of the dark-frame fold, one allocation made at the first begin and
    // freed by _end or with the context: count[3] (uint32), sum[3], sum_sq[3] (uint64), dense planes jfped_stride entries apart (W * H rounded
    // up to 8: the kernel's last group stays inside them).  Null: not begun.  jfped_st: the context's own HIP stream, in which the fold
    // launches follow one another -- every launch reads, adds and writes the accumulators, two must never overlap; jfped_mu makes "wait for
    // the chunks, launch, count the frames" one step (folds come from distinct ffs_streams on distinct threads).
    uint8_t* d_jfped = nullptr;
    size_t jfped_stride = 0;
    uint64_t jfped_frames = 0;
    hipStream_t jfped_st = nullptr;
    std::mutex jfped_mu;
    // ffs_ctx_set_radial_bins: [H][pitch_px] uint16 bin entries, allocated at the first set and kept (entries beyond W
    // are 0xFFFF); settings.radial_bins says whether a map is in force and how many bins it has (0 = none).  Like the gain map it cannot change under a batch.
    uint16_t* d_radial_map = nullptr;
    uint8_t* d_radial_map8 = nullptr;   // the same rows in one byte an entry (0xFF: in no bin), behind the two-byte rows in the same allocation; written for maps of at most 255 bins
    // ffs_ctx_set_pixel_stats: the four accumulator planes are one allocation, made at the first start and kept (count,
    // max, sum, sum of squares, in that order; laid out in tiles: PixStatsLayout below).  settings.pixel_stats: batches submitted from now on are folded in;
    // stats_started: there has been a start, ffs_ctx_get_pixel_stats has something to hand out.  stats_st: the context's own HIP stream for the
    // launches (tuning "stats_stream" 0), made with the accumulators.  stats_mu: one launch at a time is put behind the previous one --
    // distinct ffs_streams are driven from distinct threads -- and adds its frames to stats_frames.
    uint8_t* d_stats = nullptr;
    bool stats_started = false;
    uint64_t stats_frames = 0;
    hipStream_t stats_st = nullptr;
    std::mutex stats_mu;
    // ffs_ctx_shoebox_begin: the open summation-integration job -- table, index, accumulators and a HIP stream of its
    // own -- or null.  shoebox_mu: begin, fold, the getters and end are one step each; a fold reads, adds and writes the accumulators, and folds
    // come from distinct ffs_streams on distinct threads.
    ShoeboxJob* shoebox = nullptr;
    std::mutex shoebox_mu;
    // ffs_ctx_predict: the HIP stream, events and device buffers its calls use, made by the first call and kept; a call
    // is one step under predict_mu.  Nothing of a batch is in here.
    PredictState* predict = nullptr;
    std::mutex predict_mu;
    // ffs_ctx_index_grid / index_load_grid / index_peaks: the same for the index calls, with the grids of the last n_points
    IndexState* index = nullptr;
    std::mutex index_mu;
    // ffs_ctx_index_assign: the same for index assignment; its device buffers live for one call
    AssignState* assign = nullptr;
    std::mutex assign_mu;
    uint8_t* d_maskbits = nullptr;
    uint8_t* d_ginfo = nullptr;  // per-group mask bits + window-count bounds (kernels_stream.hpp)
    uint8_t* d_mmap = nullptr;   // per-pixel window counts
    EmptyRuns empty_runs{};      // the rows the mask leaves empty (launch_geometry.hpp), rebuilt with the two tables above; every launch's arguments carry a copy
    hipStream_t dense_st = nullptr;  // sched 3: the one stream of the dense kernels
    // ... and its partner (tuning "dense_overlap", off: measured slower in the pipeline): the streaming kernels of the wave-log path take
    // the two alternately, each behind a wait for the value the previous launch's last workgroup writes into `d_handoff` (signal
    // memory) as it starts.  Both are made by the first launch that asks.  dense_mu: one launch at a time decides.
    hipStream_t dense_st2 = nullptr;
    uint32_t* d_handoff = nullptr;
    std::mutex dense_mu;
    uint32_t handoff_seq = 0;
    int handoff_last = -1;           // which of the two streams took the last launch of the chain
    hipStream_t up_st = nullptr;     // ... and the one stream of uploads and decoding
    hipStream_t sparse_st[2] = {nullptr, nullptr};  // ... the sparse launches of the context's streams, alternating
    int n_streams_made = 0;
    std::mutex stream_mu;            // guards the lazy creation of the shared streams, the stack pool, the event ring and the two lists below
    // What the context's users have created on it and not destroyed yet: ffs_ctx_destroy closes these first (a stream or a stack
    // keeps a pointer to its context), and the process's exit handler finds in-flight work through them (lifecycle, below).
    std::vector<ffs_stream*> live_streams;
    std::vector<ffs_stack3d*> live_stacks;
    std::vector<ffs_stack3d*> stack_pool;   // destroyed 3D stacks kept with their buffers for the next sweep (stream_mu)
    // Pinned host memory costs ~170 ms per GB to allocate and ~100 ms per GB to free, and the runtime serialises both
    // across threads (tools/ubench/alloc_cost.hip): the staging buffers of destroyed streams are kept for the next
    // stream of the context and freed with it (stream_mu).
    std::vector<struct PinnedBuf> pinned_pool;
    std::atomic<int> inflight{0};    // batches between submit and wait, over all ffs_streams of the context
    // Start events of the sparse launches (they ride on the dispatch): the next streaming kernel lets the newest one get
    // its CUs first.  The events belong to the CONTEXT (created with the first stream, destroyed with the context), so a
    // thread may wait on one while another thread destroys the ffs_stream that recorded it.
    static constexpr int kChainEvents = 16;
    hipEvent_t chain_ev[kChainEvents] = {};
    std::atomic<uint32_t> chain_ev_next{0};     // slots handed out so far
    std::atomic<int> chain_ev_newest{-1};       // slot of the newest recorded start, -1: none yet
    bool chain_ok = false;           // k_frame_chain may use its dynamic LDS on this device
    std::atomic<AssemblyPool*> assembly{nullptr};   // helper threads of ffs_wait (created on first use under stream_mu; read without it)
    std::atomic<AheadThread*> ahead{nullptr};       // assembles results as batches complete (created on first use under stream_mu)
    ThreadError err;  // the calling thread's most recent error on any context
};

struct OverflowFrame;

// What a stream keeps for encoded input (ffs_encoded.hip), all allocated on first use and freed by encoded_free.  d_comp: the device side of
// the staging area, d_comp_bytes long, regrown with the staged bytes.  bitshuffle-LZ4: the frame's blocking and the per-block tables
// (device and pinned host, max_batch frames).  CBF byte-offset: the frame table (device and pinned host, max_batch frames) and the three
// summary tables, which hold bo_tiles_cap tiles and follow the staged bytes as d_comp does.
struct EncodedState {
    uint8_t* d_comp = nullptr;
    size_t d_comp_bytes = 0;
    BshufBlocking blocking;
    BlockEntry *d_tab = nullptr, *h_tab = nullptr;
    BoFrame *d_bo_frames = nullptr, *h_bo_frames = nullptr;
    uint2 *d_bo_lane = nullptr, *d_bo_map = nullptr;
    uint4* d_bo_state = nullptr;
    size_t bo_tiles_cap = 0;
};

constexpr uint32_t kBrightCap = 1u << 20;  // entries of the bright-window list per batch (8 MB)

struct ffs_stream {
    ffs_ctx* ctx = nullptr;
    uint32_t max_batch = 1;   // frames per submit
    uint32_t cap = 0;         // strong pixels per frame the lists hold
    uint32_t max_comp = 0;    // components per frame the record buffers hold
    ffs_stream* big = nullptr;               // one-frame stream with room for frames that exceed cap / max_comp
    std::vector<OverflowFrame> ovf;          // such frames of the last batch, re-run on `big`
    bool lists_valid = true;                 // the last batch left its strong-pixel lists on the device
    bool log_off = false;                    // the wave logs could not serve a batch of this stream (dense frames, a log overflow): the plane from then on
    uint2* d_wlog = nullptr;                 // wave logs of the streaming kernel (allocated on first use, sized for the launch geometry)
    uint32_t* d_wlog_n = nullptr;
    uint4* d_wpix = nullptr;
    size_t wlog_waves = 0;
    // the sparse stage in small workgroups (kernels_band.hpp): what the band waves hand to the per-frame merge (allocated on first use)
    uint4* d_band_hdr = nullptr;
    uint8_t* d_band_acc = nullptr;
    uint32_t* d_band_seam = nullptr;
    uint32_t band_slots = 0;                 // (frame, band) pairs the three buffers hold
    uint32_t band_backoff = 0;               // batches this stream still sends through k_frame_chain after a band overflowed its plan (kOvfBandPlan: dense data)
    uint32_t path_bits = 0;                  // which launches the last batch took (ffs_stream_last_path)
    uint32_t reruns = 0;                     // times ffs_wait ran the last batch again (a plan that did not hold it)
    bool runs_overflowed = false;            // a frame's runs overflowed the one launch: dense batches of this stream take the grid-wide sparse kernels
    uint32_t *d_pack_k = nullptr, *d_pack_i = nullptr;  // a batch's lists packed end to end for another device's 3D stack
    StackSlice *d_pack_tab = nullptr, *h_pack_tab = nullptr;
    hipEvent_t ev_pack = nullptr;            // the packed lists are ready on the source device
    hipEvent_t ev_sent = nullptr;            // ... and have been copied out of the pack buffers (an event of device ev_sent_dev, the stack's)
    int ev_sent_dev = -1;
    bool sent_pending = false;
    hipStream_t st = nullptr;    // threshold kernels (+ H2D)
    hipStream_t st_up = nullptr; // uploads + decode; == st unless the dense kernels of the context share one stream
    bool st2_shared = false;
    bool st_shared = false;      // st is the context's dense stream (not ours to destroy)
    hipStream_t st2 = nullptr;   // compaction + connected components + D2H; == st unless the context has sparse streams
    hipEvent_t ev[7] = {};   // [6]: the compressed chunks and their block table are on the device
    // device (one allocation, d_slab, carved up at creation; the buffers of rarely used paths are allocated on first use)
    uint8_t* d_slab = nullptr;
    uint8_t* d_img = nullptr;
    uint8_t* d_bits = nullptr;
    uint8_t* d_sbytes = nullptr;
    uint8_t *d_dplane = nullptr, *d_eplane = nullptr;  // extended algorithm only (allocated on first use)
    // The first-pass plane must be all zero when the streaming kernel starts (it writes non-zero bytes only).  Two planes take
    // turns: the one the previous batch used is cleared in the sparse stream behind this batch's sparse launch -- done before
    // this batch's last event, i.e. before the stream's next submit -- instead of by a fill in the dense stream ahead of every
    // first pass; the last batch's plane stays readable (ffs_stream_debug_bitplane, --writeout).
    // Round 4: the signal-region plane has a twin too (the erosion then stores only the words that hold a pixel of the region); a
    // first-pass plane and a signal-region plane are ONE allocation (d_ext_pair), so one fill clears both.
    uint8_t* d_dplane2 = nullptr;
    uint8_t* d_eplane2 = nullptr;
    uint8_t* d_ext_pair[2] = {nullptr, nullptr};
    bool dplane2_clean = false;                        // the first-pass plane the NEXT batch takes is zero
    bool eplane2_clean = false;                        // ... and so is the signal-region plane behind it
    bool ext_e_clean = false;                          // this batch's signal-region plane is zero (make_threshold_args passes it on)
    EncodedState enc;                                  // encoded input (ffs_encoded.hip)
    // Without direct records: copied back speculatively with the counts (one wait instead of two): room for the most
    // records per frame seen so far on this stream, +25 %; ffs_wait fetches the rest if a batch exceeds it.
    uint32_t spec_recs_per_frame = 256;
    uint64_t spec_recs_copied = 0;
    std::thread job;          // ffs_submit_compressed's helper (block index + launches); joined by ffs_wait
    int job_rc = 0;
    std::string job_err;
    uint32_t *d_tile_counts = nullptr, *d_num_strong = nullptr, *d_row_off = nullptr;
    uint2* d_bright = nullptr;  // pixels the streaming kernels hand to k_bright_fix; their count sits behind the tile counts
    uint32_t *d_list_k = nullptr, *d_list_i = nullptr, *d_parent = nullptr;
    uint32_t *d_n_comp = nullptr, *d_overflow = nullptr, *d_summary = nullptr;
    CompAcc2* d_acc2 = nullptr;          // accumulators at the root's list index
    uint32_t* d_chunk_roots = nullptr;
    ReflOut* d_recs = nullptr;
    // pinned host
    uint8_t* h_img = nullptr;      // pinned staging: allocated on first use (ensure_host_staging), sized by what is asked for
    size_t h_img_bytes = 0;
    PinnedBuf h_img_buf;           // ... and how it was obtained
    uint32_t* h_counts = nullptr;  // the counter block (layout: ffs_device.h, counts_*_at; counts_host_words(max_batch) words)
    ReflOut* h_recs = nullptr;
    uint32_t* d_occ = nullptr;     // [max_batch][occ_frame_words] occupancy of the strong plane (one bit per 16-byte segment)
    uint32_t* h_counts_dev = nullptr;  // device-side address of h_counts (k_frame_chain writes the counters itself)
    bool ev1_pending = false;      // ev[1] (start of the threshold stage) has not been recorded yet for this batch
    bool ev3_is_ev4 = false;       // one event behind the sparse launch (k_frame_chain leaves nothing to copy)
    bool dev_input = false;        // this batch's frames were on the device already (ffs_submit_device): no upload, no ev[0]
    bool dense_valid = false;      // the byte masks of the last batch were produced
    bool chain_mode = false;       // this batch went through k_frame_chain: records at frame * max_comp, flags per frame
    ReflOut* h_recs_dev = nullptr;  // device-side address of h_recs when the records are written straight to the host
    bool direct_recs = false;
    bool bits_cleared = false;  // the last batch's compaction zeroed the strong plane again (the streaming kernels' invariant)
    bool bits_dirty = false;    // the strong plane may hold bits: the streaming kernels need it zeroed first
    bool counts_dirty = true;   // the per-tile counts (+ bright-list count) may be non-zero: the streaming kernels add into them
    bool occ_dirty = false;     // the occupancy bitmap may hold bits nobody will consume
    uint32_t *h_list_k = nullptr, *h_list_i = nullptr;
    uint8_t* h_mask = nullptr;
    // The radial profile (kernels_radial.hpp) of a batch whose snapshot has radial_bins (ParamSnapshot).  radial_todo: set by the submit entry
    // points -- the batch's first enqueue launches the profile and clears it, the re-runs inside ffs_wait find it off; radial_pending: a batch
    // is in flight whose profile (or the lack of one) ffs_wait has not handed out yet (set once its launches are enqueued).  The bands' partials
    // live on the device; the results are written straight into one of two pinned host buffers that take turns, so the profile ffs_wait handed
    // out stays readable while the next batch is in flight.  All allocated on first use and re-sized when a later map has more bins (a host
    // buffer somebody may still read is retired, and freed at the next wait).
    bool radial_todo = false, radial_pending = false;
    uint8_t* d_radial_part = nullptr;
    size_t radial_part_entries = 0;          // (frame, band, bin) triples the partials hold
    uint8_t *h_radial[2] = {nullptr, nullptr}, *h_radial_dev[2] = {nullptr, nullptr};
    uint32_t h_radial_bins = 0;              // bins per frame the two host buffers hold
    int radial_turn = 0;                     // the host buffer the next batch writes
    std::vector<uint8_t*> radial_retired;
    const uint8_t* radial_out = nullptr;     // what ffs_stream_radial_profile reads: the last waited batch's buffer, bins (0: no profile) and frames
    uint32_t radial_out_bins = 0, radial_out_frames = 0;
    // The radial-profile threshold (kernels_radthr.hpp) of a batch whose snapshot has radthr_bins.  All made by the stream's first such batch,
    // for kRadThrMaxBins shells and max_batch frames: the frames' histograms and cutoffs on the device, and two pinned host buffers of
    // ffs_radial_shell records that take turns like the profile's (a re-run inside ffs_wait writes the same records into the same buffer).
    // radthr_out: what ffs_stream_radial_thresholds reads, the last waited batch's buffer (null: that batch ran another algorithm).
    uint32_t *d_radthr_hist = nullptr, *d_radthr_cut = nullptr;
    ffs_radial_shell *h_radthr[2] = {nullptr, nullptr}, *h_radthr_dev[2] = {nullptr, nullptr};
    int radthr_turn = 0;
    const ffs_radial_shell* radthr_out = nullptr;
    uint32_t radthr_out_bins = 0, radthr_out_frames = 0;
    // The per-pixel statistics (kernels_pixstats.hpp) of a batch whose snapshot has pixel_stats.  stats_todo: set by the submit entry points --
    // the batch's first enqueue launches the kernel and clears it, the re-runs inside ffs_wait find it off; stats_join: that launch is not in
    // the batch's sparse stream, which waits for ev_stats (recorded behind it, made on first use) ahead of the batch's last event.
    bool stats_todo = false, stats_join = false;
    hipEvent_t ev_stats = nullptr;
    // ffs_stream_jungfrau_pedestal_fold: the two events around the stream's fold launches (its own, made on first use: the batch's events keep
    // the last batch's stage times)
    hipEvent_t jfped_ev[2] = {nullptr, nullptr};
    // The per-spot backgrounds (ffs_spotbg.hip, kernels_spotbg.hpp), all made by the first ffs_stream_spot_backgrounds
    // on the stream: a non-blocking HIP stream of the ffs_stream's own with two events around its launch, the boxes of the last batch's
    // reflections (pinned host, written by the call, and their copy on the device) and the records the kernel writes straight into pinned host
    // memory -- room for bg_cap reflections each, grown when a batch has more.  waited_ok: the last ffs_wait on the stream returned FFS_OK,
    // so results / refls / cur_img describe one batch (ffs_wait_impl sets it; ffs_decode_only*, which overwrite the stream's frames, clear it).
    bool waited_ok = false;
    hipStream_t bg_st = nullptr;
    hipEvent_t bg_ev[2] = {nullptr, nullptr};
    void *h_bg_boxes = nullptr, *d_bg_boxes = nullptr;
    ffs_spot_background *h_bg_out = nullptr, *h_bg_out_dev = nullptr;
    uint32_t bg_cap = 0;
    // ffs_stream_spot_backgrounds_glm shares all of the above but the records: its own pinned buffer, room for bg_glm_cap reflections
    ffs_spot_background_glm *h_bg_glm_out = nullptr, *h_bg_glm_out_dev = nullptr;
    uint32_t bg_glm_cap = 0;
    // state of the batch in flight
    bool busy = false;
    uint32_t n_frames = 0;
    int64_t first_id = 0;
    const void* cur_img = nullptr;
    size_t cur_pitch = 0, cur_fstride = 0;
    ParamSnapshot batch;
    float timings[5] = {0, 0, 0, 0, 0};
    bool timings_stale = false;              // the stage times of the last batch are still in its events (ffs_stream_timings reads them out)
    hipEvent_t timing_last = nullptr;
    // results
    std::vector<ffs_frame_result> results;
    std::vector<ffs_box> boxes;
    std::vector<ffs_reflection> refls;
#ifdef FFS_EXPERIMENTS
    unsigned long long *h_phase_ts = nullptr, *h_phase_ts_dev = nullptr;   // device timestamps of the sparse launch's phases (pinned, [B][8])
    double phase_sum[8] = {};       // accumulated phase durations, us (printed when the stream is destroyed; FFS_EXP_CHAIN_TS)
    unsigned long long phase_n = 0;
#endif
    std::vector<float> centres;   // (frame id bits, com_x, com_y, com_z) per reflection of the last batch, filled with `refls` (ffs_stream_spot_centres)
    // the same four for the batch in flight, filled by the context's AheadThread and swapped in by ffs_wait (what the last ffs_wait
    // returned stays valid until the next one)
    std::vector<ffs_frame_result> results_n;
    std::vector<ffs_box> boxes_n;
    std::vector<ffs_reflection> refls_n;
    std::vector<float> centres_n;
    int ahead_state = 0;          // 0: not registered, 1: queued / being assembled, 2: assembled into the *_n arrays, 3: left to the caller (AheadThread::mu)
};

// Results of a frame that did not fit the stream's lists, from its re-run on the one-frame stream
struct OverflowFrame {
    uint32_t frame = 0;
    ffs_frame_result res{};
    std::vector<ffs_box> boxes;
    std::vector<ffs_reflection> refls;
    std::vector<uint32_t> k, inten;
};

// the re-run of frame `f` among a batch's overflow frames, or null (`ovf` may be null: a batch assembled ahead of its wait has none)
static inline const OverflowFrame* overflow_frame(const std::vector<OverflowFrame>* ovf, uint32_t f) {
    if (ovf)
        for (const OverflowFrame& o : *ovf)
            if (o.frame == f) return &o;
    return nullptr;
}

// ---- no exception crosses the C ABI -----------------------------------------------------------------------
// The entry points that grow std::vectors (results, staging tables, masks) run inside a catch-all: an
// allocation failure or a length error becomes FFS_ERR_NOMEM with its text in ffs_last_error, instead of
// std::terminate -> abort() in the caller's process.
template <typename F>
static int guarded(ffs_ctx* c, F&& body) {
    try {
        return body();
    } catch (const std::exception& e) {
        if (c) c->err = std::string("exception inside libffs_hip: ") + e.what();
        else g_create_error = std::string("exception inside libffs_hip: ") + e.what();
        return FFS_ERR_NOMEM;
    } catch (...) {
        if (c) c->err = "unknown exception inside libffs_hip";
        return FFS_ERR_NOMEM;
    }
}

#define HIP_TRY(ctx, expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);             \
            return e_ == hipErrorOutOfMemory ? FFS_ERR_NOMEM : FFS_ERR_DEVICE;          \
        }                                                                               \
    } while (0)

// (the same, as the stack's and the exchange's units have always spelt it)
#define STK_TRY(c, expr)                                                        \
    do {                                                                        \
        hipError_t e_ = (expr);                                                 \
        if (e_ != hipSuccess) {                                                 \
            (c)->err = std::string(#expr) + ": " + hipGetErrorString(e_);       \
            return e_ == hipErrorOutOfMemory ? FFS_ERR_NOMEM : FFS_ERR_DEVICE;  \
        }                                                                       \
    } while (0)

// (a step that failed has left its text in the context's error: its code is passed on)
#define FFS_TRY(expr)                    \
    do {                                 \
        const int rc_ = (expr);          \
        if (rc_ != FFS_OK) return rc_;   \
    } while (0)

// a refusal: its text goes where the caller keeps errors (the context's text of the calling thread, or a helper thread's job_err)
template <typename Err>
static int refuse(Err& err, int rc, const std::string& text) { err = text; return rc; }

// ---- small helpers ------------------------------------------------------------------------------------------
// Where the per-pixel statistics lie (kernels_pixstats.hpp has the why): a lane owns px = 16 / pixel_bytes pixels of a row, lanes are numbered
// row by row, sixty-four of them are a tile, and in every plane a lane's entries are chunks of 16 B, chunk k of lane l of tile t at
// 16 B x ((t * chunks + k) * 64 + l).
struct PixStatsLayout {
    uint32_t px = 0, groups = 0, n_lanes = 0;
    size_t plane32 = 0, plane64 = 0;   // bytes of a plane of 32-bit entries (count, max) and of 64-bit entries (sum, sum of squares)
    size_t bytes() const { return 2 * plane32 + 2 * plane64; }
    // entry j (0 .. px - 1) of lane i in a plane of entry_bytes-byte entries, counted in entries
    size_t entry(uint32_t i, uint32_t j, uint32_t entry_bytes) const {
        const uint32_t per_chunk = 16u / entry_bytes, chunks = px / per_chunk;
        return (((size_t)(i >> 6) * chunks + j / per_chunk) * 64u + (i & 63u)) * per_chunk + j % per_chunk;
    }
};
static inline PixStatsLayout pixstats_layout(const ffs_ctx* c) {
    PixStatsLayout p;
    p.px = 16u / (uint32_t)c->settings.pixel_bytes;
    p.groups = ((uint32_t)c->L.W + p.px - 1) / p.px;
    p.n_lanes = p.groups * (uint32_t)c->L.H;
    const size_t tiles = ((size_t)p.n_lanes + 63) / 64;
    p.plane32 = tiles * 64 * p.px * 4;
    p.plane64 = tiles * 64 * p.px * 8;
    return p;
}
// What ffs_wait asks of the enqueue that runs a batch AGAIN because a plan did not hold it (ffs_wait.hip, rerun_batch); the default
// is a normal batch.  An argument of that one call: what a stream remembers beyond it (log_off, runs_overflowed, band_backoff) is
// in ffs_stream.
struct Rerun {
    int threshold_path = -1;   // >= 0: the threshold path of this enqueue (bright-list overflow -> 1)
    bool plane = false;        // takes the plane (a batch the wave logs could not serve)
    bool no_bands = false;     // takes k_frame_chain (the batch that raised kOvfBandPlan)
    bool grid = false;         // takes the grid-wide sparse kernels (a frame's runs overflowed the one launch)
};
// extended algorithm: the strip erosion stores only the non-zero words of a signal-region plane that was cleared behind the previous batch
static inline bool ext_sparse_erode(const Tuning& t) { return t.ext_erode != 0 && t.ext_e_sparse; }
static inline uint32_t occ_frame_words(const Layout& L) { return (uint32_t)(((uint64_t)L.H * (L.mpitch / 16) + 31) / 32 + 2); }  // (+2: the chain reads a word ahead)
// per-tile counts | ... | [last - 1] workgroups of k_frame_chain through with the bright list | [last] entries of the bright list;
// a multiple of 256 bytes so that one fill clears it
static inline size_t tile_counts_bytes(const ffs_stream* s) { return (((size_t)s->max_batch * s->ctx->n_tiles + 2) * 4 + 255) / 256 * 256; }
static inline void mark_busy(ffs_stream* s) {
    if (!s->busy) ++s->ctx->inflight;
    s->busy = true;
}
static inline void mark_idle(ffs_stream* s) {
    if (s->busy) --s->ctx->inflight;
    s->busy = false;
}
template <typename T>
static hipError_t dmalloc(T** p, size_t n_bytes) {
    return hipMalloc(reinterpret_cast<void**>(p), n_bytes + 256);
}
// What a setter may not do under a batch: FFS_OK while none of the context is in flight, else the refusal, `who` in front and `why` behind
static inline int refuse_in_flight(ffs_ctx* c, const char* who, const char* why) {
    if (c->inflight.load() == 0) return FFS_OK;
    return refuse(c->err, FFS_ERR_INVALID, std::string(who) + ": a batch of this context is in flight (ffs_wait for it first)" + why);
}
// A per-pixel table of the context on the device: H rows of pitch_px entries, addressed like the pixel rows, the entries beyond W are `fill`.
// *d_table is allocated at the first set, extra_bytes_per_entry behind the rows, and kept; `rows` is left holding what was copied.
template <typename T>
static int upload_pixel_table(ffs_ctx* c, const char* who, const char* what, const T* host, T fill, size_t extra_bytes_per_entry, T** d_table, std::vector<T>& rows) {
    const Layout& L = c->L;
    rows.assign((size_t)L.pitch_px * L.H, fill);
    for (int y = 0; y < L.H; ++y) std::memcpy(rows.data() + (size_t)y * L.pitch_px, host + (size_t)y * L.W, (size_t)L.W * sizeof(T));
    HIP_TRY(c, hipSetDevice(c->device));
    if (!*d_table && hipMalloc(reinterpret_cast<void**>(d_table), rows.size() * (sizeof(T) + extra_bytes_per_entry)) != hipSuccess) {
        (void)hipGetLastError();
        *d_table = nullptr;
        return refuse(c->err, FFS_ERR_NOMEM, std::string(who) + ": hipMalloc(" + what + ") failed");
    }
    HIP_TRY(c, hipMemcpy(*d_table, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice));
    return FFS_OK;
}

// ---- lifecycle: which handles are alive ---------------------------------------------------------------------
// Every handle the ABI has given out is in a process-wide registry until it is destroyed -- by its own destroy call, or by the
// ffs_ctx_destroy of its context, which closes a context's streams and stacks before the context itself.  A destroy call on a handle
// that is not (or no longer) in the registry does nothing, so the ORDER in which a caller (a binding's finalisers, a C++ driver's
// unwinding, a test that leaks) lets go of contexts, streams and stacks cannot reach freed memory.  When the process exits with
// handles alive, the library's own exit handler -- registered after the HIP runtime has initialised, so it runs BEFORE the runtime's
// handlers -- joins the helper threads and waits for the work in flight (kernels that write into pinned host memory); every destroy
// call after that is a no-op and the runtime's own teardown takes the memory.  DESIGN.md section 10c.
enum HandleKind { kHandleCtx = 0, kHandleStream = 1, kHandleStack = 2 };
void handle_add(HandleKind kind, const void* h);
bool handle_take(HandleKind kind, const void* h);   // removes h; false: not a live handle (destroyed already, or the process is exiting)
bool handle_live(HandleKind kind, const void* h);
bool process_exiting();
// A stream handle that its context's ffs_ctx_destroy (or an earlier ffs_stream_destroy) has closed is refused by submit and wait
// with FFS_ERR_INVALID and a text in ffs_last_error(NULL), instead of being followed into freed memory.
static inline bool stream_handle_ok(const ffs_stream* s) {
    if (handle_live(kHandleStream, s)) return true;
    g_create_error = "stale ffs_stream handle: the stream was destroyed (with its context, or by ffs_stream_destroy)";
    return false;
}
void stream_destroy_internal(ffs_stream* s);         // what ffs_stream_destroy does once the handle is out of the registry

// ---- functions one unit calls in another ----------------------------------------------------------------------
// ffs_context.hip
int stream_create_sized(ffs_ctx* c, uint32_t max_batch, uint32_t cap, uint32_t max_comp, ffs_stream** out);
int ensure_host_staging(ffs_stream* s, size_t bytes);   // pinned staging of at least `bytes` (contents are not kept when it grows)
size_t default_staging_bytes(const ffs_stream* s);      // max_batch raw frames (+ the slack incompressible chunks need)
// ffs_submit.hip
bool chain_prepare_device();   // asks for k_frame_chain's dynamic LDS on the current device; false: use the four kernels
StreamGeometry batch_stream_geometry(const ffs_stream* s, size_t fstride, uint32_t n_frames);   // launch_geometry.hpp's, for a batch of this stream
ThresholdRoute batch_route(const ffs_stream* s, const Rerun& how);   // threshold_route.hpp's, for the stream's batch (s->batch) and what a re-run overrides
ThresholdArgs make_threshold_args(ffs_stream* s, const void* img, size_t pitch, size_t fstride, uint32_t n_frames, const StreamGeometry& g,
                                  const ThresholdRoute& route);
int check_layout(ffs_stream* s, size_t pitch, size_t fstride, uint32_t n_frames);
int ensure_extended_buffers(ffs_stream* s);
int enqueue_batch(ffs_stream* s, const void* d_img, size_t pitch, size_t fstride, uint32_t n, const ParamSnapshot* snapshot = nullptr,
                  const Rerun& how = Rerun{});
extern std::atomic<int> g_live_stacks;   // 3D stacks alive in the process (ffs_stack3d.hip)
bool wave_logs_for(ffs_stream* s, ThresholdArgs& a, const StreamGeometry& g, const Rerun& how);
// The threshold stage where all of it runs in s->st, in its two steps: the dense kernel, with HIP events on the dispatch itself (either
// may be null), and the kernels that follow it (k_bright_fix / k_exact; extended: erosion + final pass; none behind the general-window
// kernel or with wave logs).  What enqueue_batch launches for such a batch, and what ffs_bench_threshold times.
void launch_dense_kernel(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, const StreamGeometry& g, uint32_t n_frames, hipEvent_t start,
                         hipEvent_t stop, bool plane_clean = false, bool counts_clean = false);
void launch_dense_rest(ffs_stream* s, const ThresholdRoute& route, const ThresholdArgs& a, uint32_t n_frames);
// ffs_products.hip
// The radial profile: ensure makes room for the profiles of this stream's batches under a map of `bins` bins (no batch of the stream in flight);
// launch puts the two kernels into `st` for frames that are in place there (start / stop: events on the two dispatches, either may be null).
// launch_radial_dense / _stage: the batch's two places for it, behind the threshold stage's kernels or behind the sparse launch; publish is ffs_wait's side.
int radial_ensure_buffers(ffs_stream* s, uint32_t bins);
int radial_launch(ffs_stream* s, const void* d_img, size_t pitch, size_t fstride, uint32_t n_frames, hipStream_t st, hipEvent_t start, hipEvent_t stop);
int launch_radial_dense(ffs_stream* s, uint32_t n);
int launch_radial_stage(ffs_stream* s, uint32_t n);
void radial_publish(ffs_stream* s);
void radial_free(ffs_stream* s);
// The radial-profile threshold (ThresholdStage::kRadial): ensure makes the stream's buffers and asks the device for the histogram's LDS (first
// use); hist and rest (the cut and strong kernels) launch into s->st from the threshold stage's arguments; publish is ffs_wait's side.
int radthr_ensure_buffers(ffs_stream* s);
void launch_radthr_hist(ffs_stream* s, const ThresholdArgs& t, uint32_t n_frames, hipEvent_t start, hipEvent_t stop);
void launch_radthr_rest(ffs_stream* s, const ThresholdArgs& t, uint32_t n_frames, hipEvent_t stop);
void radthr_publish(ffs_stream* s);
void radthr_free(ffs_stream* s);
// The per-pixel statistics: ensure makes the accumulators and the context's stream on first use; launch puts the kernel over n_frames frames that
// are in place in `st` (the caller keeps two launches apart).  launch_pixel_stats does that for a batch, once; join_pixel_stats makes its sparse stream wait.
int pixstats_ensure(ffs_ctx* c);
int pixstats_launch(ffs_ctx* c, const void* d_img, size_t pitch, size_t fstride, uint32_t n_frames, long long max_valid, hipStream_t st, hipEvent_t start,
                    hipEvent_t stop);
int launch_pixel_stats(ffs_stream* s, uint32_t n);
int join_pixel_stats(ffs_stream* s);
// ffs_encoded.hip
const char* encoded_corruption(uint32_t overflow);   // the text for a status word in which a decode kernel flagged a corrupt chunk, else null
void encoded_free(ffs_stream* s);
void jfped_free_stream(ffs_stream* s);   // the stream's fold events, if it ever folded
void jfped_free_ctx(ffs_ctx* c);         // the accumulators and the context's fold stream (context destroy; every stream is closed)
// ffs_wait.hip
int ffs_wait_impl(ffs_stream* s, const ffs_frame_result** results, uint32_t* n_results);
void ahead_register(ffs_stream* s);   // the batch just enqueued may be assembled ahead of its ffs_wait
int ahead_take(ffs_stream* s);        // waits for the AheadThread to be done with the stream's batch; its verdict (0, 2 or 3), state reset
void ahead_stop(ffs_ctx* c, bool destroy);   // the thread leaves and is joined (context destroy, process exit)
// ffs_spotbg.hip
void spotbg_free(ffs_stream* s);   // the stream's own HIP stream, events and buffers of ffs_stream_spot_backgrounds, if it was ever called
// ffs_shoebox.hip
void shoebox_free_ctx(ffs_ctx* c);   // the open job, if any (context destroy; every stream is closed)
// ffs_predict.hip
void predict_free_ctx(ffs_ctx* c);   // what ffs_ctx_predict kept (context destroy)
// ffs_index.hip
void index_free_ctx(ffs_ctx* c);     // what the index calls kept (context destroy)
// ffs_assign.hip
void assign_free_ctx(ffs_ctx* c);    // what ffs_ctx_index_assign kept (context destroy)
// ffs_stack3d.hip
void stack3d_free(ffs_stack3d* st);
// ffs_multi.hip
void gather_scratch_free(ffs_stream* s);   // what ffs_multi_gather_rows allocated for the stream, if anything
// A batch's two packed arrays (s->d_pack_k / _i, `packed` entries, packed in s->st2) from the stream's device into dst_k / dst_i on the device
// of `home`, ordered on home_st: RCCL send / recv in one group, or a peer (one GPU: device) copy behind s->ev_pack that leaves s->ev_sent
int multi_move_packed(ffs_stream* s, ffs_ctx* home, hipStream_t home_st, uint32_t* dst_k, uint32_t* dst_i, uint64_t packed);
