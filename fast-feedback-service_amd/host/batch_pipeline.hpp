// batch_pipeline.hpp -- GPU batches assembled from several reader threads.
//
// The reference gives every worker thread one frame at a time: read, decompress, copy, kernel, copy back, connected
// components, in sequence (spotfinder.cc:751-1008).  Rounds 2-3 gave every worker batches of its own -- four frames, an
// eighth of what the kernels are tuned for, and sixteen small submissions in flight.  Now a GPU batch is an ASSEMBLY that all
// the GPU's reader threads fill together: global batch b holds images b B .. b B + B - 1, goes to GPU b mod n_dev, and sits
// in assembly (b / n_dev) mod K of that GPU (an ffs_stream with its pinned staging area cut into B slots).  A reader takes
// the next slot number from the GPU's counter, reads that image's chunk into its slot, and whoever fills a batch's last
// slot submits it.  One collector thread per GPU waits for the batches in order, hands each to the driver's callback
// and frees the assembly for batch b + K n_dev.  Readers never wait for the GPU unless all K assemblies are in flight.
//
// Depends on ffs_hip.h (streams, submit, wait, ffs_last_error -- nothing of contexts, the 3D stack or the exchange between
// GPUs), reader.hpp, codecs.hpp and the standard library: tests/pipeline_cpu links it against a fake of those calls.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <sched.h>
#include <set>
#include <span>
#include <vector>

#include "ffs_hip.h"
#include "reader.hpp"

namespace ffshost {

struct PipelineGpu {
    ffs_ctx* ctx = nullptr;
    ffs_ctx* vctx = nullptr;         // --validate: every batch also goes through this context
    int device = 0;                  // (for the -v lines)
    std::optional<cpu_set_t> cpus;   // the GPU's NUMA node: its readers and its collector are kept there
};

struct PipelineConfig {
    uint32_t batch = 1;        // B: frames per GPU batch
    uint32_t assemblies = 1;   // K: batches in flight per GPU
    uint32_t readers = 1;      // reader threads, dealt round-robin to the GPUs
    bool gpu_decode = false;   // chunks go to the GPU as they are (ffs_submit_encoded with `codec`)
    int codec = FFS_CODEC_BSLZ4;
    // --jungfrau-calibration: the six planes (6 x width x height float32), null: the frames are photon counts.  The source's frames are raw
    // 16-bit words and bytes_per_pixel, the contexts', is 4; a frame the CPU decodes is converted by codecs.hpp's jungfrau_convert
    const float* jungfrau_planes = nullptr;
    bool read_only = false, verbose = false;
    float timeout = 30.0f;     // seconds without a new image after which the readers stop
    float slot_margin = 2.0f;  // per cent of head room per chunk slot
    uint32_t start_index = 0, num_images = 0, width = 0, height = 0;
    size_t bytes_per_pixel = 2;
    std::vector<PipelineGpu> gpus;
    std::chrono::steady_clock::time_point start;   // "... ms after the start" of the -v lines
};

// One collected batch, as the collector hands it to the driver.  Pointers hold until the callback returns.
struct BatchView {
    const ffs_frame_result* results = nullptr;
    const ffs_frame_result* validation = nullptr;   // the validation context's results, or nullptr
    uint32_t count = 0;
    const uint8_t* staging = nullptr;   // the assembly's staging area: decoded frames lie `slot_bytes` apart
    size_t slot_bytes = 0;
    float timings[5] = {0};             // ffs_stream_timings
    uint32_t submitted_by = 0;          // the reader thread that submitted the batch
    uint32_t gpu = 0;                   // index into PipelineConfig::gpus
    uint64_t q = 0;                     // the GPU-local batch number
    ffs_stream* stream = nullptr;
};
// false fails the run (the callback has printed why)
using BatchCallback = std::function<bool(const BatchView&)>;

class BatchPipeline {
  public:
    BatchPipeline(const PipelineConfig& cfg, Reader& reader, std::atomic<bool>& stop);
    ~BatchPipeline();
    // starts collectors, readers and the stop watcher, joins them; true: nothing failed
    bool run(const BatchCallback& on_batch);

    uint32_t images_completed() const { return completed_.load(); }
    double seconds_waiting_for_images() const { return time_waiting_.load(); }
    const std::vector<ffs_stream*>& streams_to_retire() const { return retired_streams_; }   // destroyed after the summary
    uint64_t total_batches() const { return total_batches_; }
    // no further batch may come: a failure, the readers have ended, or a stop was asked for (what a callback that waits
    // for other GPUs' batches has to poll -- these are announced on the GPUs' condition variables, not on its own)
    bool winding_down() const { return failed_.load() || readers_done_.load() || stop_.load(); }
    bool readers_have_ended() const { return readers_done_.load(); }   // every reader has joined, half-filled batches are flushed
    std::mutex& print_mutex() { return print_mutex_; }   // whole lines to stdout, the pipeline's -v lines among them

  private:
    struct Assembly;
    struct Gpu;
    struct ReaderState;
    void wake_all();
    void fail();
    void fail(const char* what, ffs_ctx* cx);
    void pin_to(uint32_t di);
    bool ensure_assembly(Gpu& G, Assembly& A, uint32_t index, int thread_id);
    bool submit_batch(Gpu& G, Assembly& A, uint32_t n, uint32_t first, int thread_id);
    bool read_chunk(ReaderState& R, uint32_t image_num, std::span<uint8_t> dst, std::span<uint8_t>& chunk);
    bool claim_assembly(ReaderState& R, Gpu& G, Assembly& A, uint64_t q, uint64_t b, uint32_t n_in_batch);
    bool place_chunk(ReaderState& R, Assembly& A, uint32_t k, uint32_t image_num, std::span<uint8_t>& chunk, bool have_chunk);
    bool decode_into_slot(ReaderState& R, uint8_t* slot, uint32_t image_num);
    void reader_loop(int thread_id);
    void collector_loop(uint32_t di, const BatchCallback& on_batch);
    void flush_half_filled();

    const PipelineConfig cfg_;
    Reader& reader_;
    std::atomic<bool>& stop_;
    const uint32_t n_dev_, K_;
    const size_t frame_bytes_;
    const uint64_t total_batches_;
    const bool byte_offset_;
    std::vector<std::unique_ptr<Gpu>> gpus_;
    std::mutex reader_mutex_, print_mutex_;
    std::mutex awaited_mutex_;            // guards awaited_
    std::multiset<uint32_t> awaited_;     // the images the readers are reading or waiting for right now (read_chunk): a time-out names the lowest
    std::atomic<bool> readers_done_{false};   // no batch will be submitted any more: collectors stop at the first one that is missing
    std::atomic<size_t> chunk_estimate_{0};   // staging bytes per compressed chunk, from the first chunk anybody reads
    std::atomic<int> failed_{0};
    std::atomic<uint32_t> completed_{0};
    std::atomic<double> time_waiting_{0.0};
    std::vector<ffs_stream*> retired_streams_;
};

}  // namespace ffshost
