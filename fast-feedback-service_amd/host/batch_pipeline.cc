// batch_pipeline.cc -- see batch_pipeline.hpp: assemblies, readers, collectors, the stop watcher and the flush of half-filled batches.
#include "batch_pipeline.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <pthread.h>
#include <thread>

#include "codecs.hpp"

using namespace std::chrono_literals;

namespace ffshost {

static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
static double secs(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

struct BatchPipeline::Assembly {
    ffs_stream* s = nullptr;
    ffs_stream* v = nullptr;       // --validate: the same batch on the validation context
    uint8_t* host = nullptr;       // the stream's pinned staging area (allocated when the assembly is first claimed)
    size_t host_bytes = 0, slot_bytes = 0;
    size_t over_at = 0, over_used = 0;   // overflow area behind the slots
    std::unique_ptr<std::mutex> over_mu = std::make_unique<std::mutex>();
    std::vector<const void*> chunk_ptr;
    std::vector<size_t> chunk_len;
    std::vector<std::vector<uint8_t>> spill;   // chunks that did not fit their slot (their whole batch then goes up from here)
    std::vector<uint8_t> slot_filled;          // (under the GPU's mutex) which slots of the batch hold their image
    // state, under the GPU's mutex
    int64_t batch = -1;            // the global batch this assembly holds, -1: free
    uint64_t next_q = 0;           // the GPU-local batch number it serves next (claims happen in order)
    uint32_t n = 0, filled = 0;
    bool ready = false;            // staging area in place: slots may be filled
    bool creating = false;         // somebody is making the stream and pinning the staging area
    bool submitted = false, skipped = false;
    int submitted_by = 0;
};

struct BatchPipeline::Gpu {
    ffs_ctx* ctx = nullptr;
    ffs_ctx* vctx = nullptr;
    uint32_t index = 0;
    std::vector<Assembly> as;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<uint64_t> next_slot{0};
};

// what one reader thread carries from image to image
struct BatchPipeline::ReaderState {
    int thread_id = 0;
    // scratch: a chunk whose size nobody knows yet; chunks the CPU decodes.  NOT value-initialised: a vector of this size
    // zero-fills 72 MB (10 ms of page faults on the clock, for a chunk of 7 MB)
    size_t raw_bytes = 0;
    std::unique_ptr<uint8_t[]> raw;
    std::span<uint8_t> scratch() {
        if (!raw) raw.reset(new uint8_t[raw_bytes]);
        return {raw.get(), raw_bytes};
    }
    double t_read = 0, t_chunk = 0, t_submit = 0, t_blocked = 0;
    uint32_t n_read = 0, n_submitted = 0;
    std::chrono::steady_clock::time_point last_received;
};

BatchPipeline::BatchPipeline(const PipelineConfig& cfg, Reader& reader, std::atomic<bool>& stop)
    : cfg_(cfg), reader_(reader), stop_(stop), n_dev_((uint32_t)cfg.gpus.size()), K_(cfg.assemblies),
      frame_bytes_((size_t)cfg.width * cfg.height * cfg.bytes_per_pixel),
      total_batches_(((uint64_t)cfg.num_images + cfg.batch - 1) / cfg.batch),
      byte_offset_(reader.get_raw_chunk_compression() == Reader::BYTE_OFFSET_32) {
    for (uint32_t di = 0; di < n_dev_; ++di) {
        auto g = std::make_unique<Gpu>();
        g->ctx = cfg_.gpus[di].ctx;
        g->vctx = cfg_.gpus[di].vctx;
        g->index = di;
        g->as.resize(K_);
        for (uint32_t k = 0; k < K_; ++k) {
            Assembly& A = g->as[k];
            A.next_q = k;
            A.chunk_ptr.resize(cfg_.batch);
            A.chunk_len.resize(cfg_.batch);
            A.spill.resize(cfg_.batch);
            A.slot_filled.assign(cfg_.batch, 0);
        }
        gpus_.push_back(std::move(g));
    }
}

BatchPipeline::~BatchPipeline() = default;

void BatchPipeline::wake_all() {
    for (auto& g : gpus_) { std::lock_guard<std::mutex> lock(g->mu); g->cv.notify_all(); }
}

void BatchPipeline::fail() {
    failed_ = 1;
    wake_all();
}

void BatchPipeline::fail(const char* what, ffs_ctx* cx) {
    std::printf("Error: %s%s\n", what, cx ? ffs_last_error(cx) : "");
    fail();
}

void BatchPipeline::pin_to(uint32_t di) {
    if (cfg_.gpus[di].cpus) (void)pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), &*cfg_.gpus[di].cpus);
}

// ---- the collector of one GPU: results of its batches, in order (the reference's post-processing of an image, :901-1087) ----
void BatchPipeline::collector_loop(uint32_t di, const BatchCallback& on_batch) {
    Gpu& G = *gpus_[di];
    pin_to(di);
    double t_wait = 0, t_emit = 0;
    uint32_t n_batches = 0;
    for (uint64_t q = 0;; ++q) {
        const uint64_t b = q * n_dev_ + di;
        if (b >= total_batches_) break;
        Assembly& A = G.as[q % K_];
        {
            std::unique_lock<std::mutex> lock(G.mu);
            // (an interrupt or a time-out stops the READERS; what has been submitted -- and, below, every image that was read --
            // still comes out, as the reference's workers finish the image they hold: spotfinder.cc:770-790)
            G.cv.wait(lock, [&] { return (A.batch == (int64_t)b && A.submitted) || readers_done_.load() || failed_.load(); });
            if (failed_.load() || !(A.batch == (int64_t)b && A.submitted)) break;
        }
        BatchView view;
        if (!A.skipped) {
            uint32_t nres = 0;
            const auto t_w0 = now();
            const int wrc = ffs_wait(A.s, &view.results, &nres);
            t_wait += secs(t_w0, now());
            const auto t_e0 = now();
            if (wrc != FFS_OK) { fail("", G.ctx); break; }
            ffs_stream_timings(A.s, view.timings);
            if (A.v) {
                uint32_t nv = 0;
                if (ffs_wait(A.v, &view.validation, &nv) != FFS_OK || nv != nres) { fail("validation pass: ", G.vctx); break; }
            }
            view.count = nres;
            view.staging = A.host;
            view.slot_bytes = A.slot_bytes;
            view.submitted_by = (uint32_t)A.submitted_by;
            view.gpu = di;
            view.q = q;
            view.stream = A.s;
            if (!on_batch(view)) { fail(); break; }
            completed_ += nres;
            t_emit += secs(t_e0, now());
        } else {
            completed_ += A.n;   // --read-only: nothing was submitted
        }
        ++n_batches;
        if (cfg_.verbose && n_batches <= 5 && !A.skipped) {
            const float* tm = view.timings;
            std::lock_guard<std::mutex> lock(print_mutex_);
            std::printf("GPU %d collector: batch %u out %.1f ms after the start (device: copy+decode %.2f, threshold %.2f, sparse %.2f, total %.2f ms)\n",
                        cfg_.gpus[di].device, n_batches - 1, secs(cfg_.start, now()) * 1e3, tm[0], tm[1], tm[2], tm[4]);
        }
        {
            std::lock_guard<std::mutex> lock(G.mu);
            A.batch = -1;
            A.next_q += K_;
            A.submitted = false;
            G.cv.notify_all();
        }
    }
    if (cfg_.verbose) {
        std::lock_guard<std::mutex> lock(print_mutex_);
        std::printf("GPU %d collector: %u batches; waiting for the GPU %.0f ms, results out %.0f ms, done %.0f ms after the start\n",
                    cfg_.gpus[di].device, n_batches, t_wait * 1e3, t_emit * 1e3, secs(cfg_.start, now()) * 1e3);
    }
}

// the first n frames of an assembly's batch go to the GPU (n = all of them, or what had been read when the readers stopped)
bool BatchPipeline::submit_batch(Gpu& G, Assembly& A, uint32_t n, uint32_t first, int thread_id) {
    if (cfg_.read_only) {
        A.skipped = true;
    } else {
        const bool gpu_decode = cfg_.gpu_decode;
        bool spilled = false;
        for (uint32_t i = 0; i < n; ++i) spilled = spilled || !A.spill[i].empty();
        if (gpu_decode && spilled)   // (all chunks of a batch lie in the staging area or none: the others go through the heap too)
            for (uint32_t i = 0; i < n; ++i)
                if (A.spill[i].empty()) {
                    const uint8_t* p = static_cast<const uint8_t*>(A.chunk_ptr[i]);
                    A.spill[i].assign(p, p + A.chunk_len[i]);
                    A.chunk_ptr[i] = A.spill[i].data();
                }
        const int sub = gpu_decode ? ffs_submit_encoded(A.s, cfg_.codec, A.chunk_ptr.data(), A.chunk_len.data(), n, first)
                                   : ffs_submit(A.s, A.host, n, first);
        if (sub != FFS_OK) { fail("", G.ctx); return false; }
        if (A.v) {   // the same input through the validation context
            const int vsub = gpu_decode ? ffs_submit_encoded(A.v, cfg_.codec, A.chunk_ptr.data(), A.chunk_len.data(), n, first)
                                        : ffs_submit(A.v, A.host, n, first);
            if (vsub != FFS_OK) { fail("validation pass: ", G.vctx); return false; }
        }
    }
    std::lock_guard<std::mutex> lock(G.mu);
    A.n = n;
    A.submitted_by = thread_id;
    A.submitted = true;
    G.cv.notify_all();
    return true;
}

// An assembly's stream(s) and pinned staging area, made by whoever asks first (the others wait).  The first K readers of a GPU
// each make one assembly as soon as the size of a chunk is known, side by side: made one after the other, each when its first
// batch was claimed, the first four batches of a run went through at one per 10 ms (a 150 MB staging area takes 6 ms to pin).
bool BatchPipeline::ensure_assembly(Gpu& G, Assembly& A, uint32_t index, int thread_id) {
    std::unique_lock<std::mutex> lock(G.mu);
    if (A.ready) return true;
    if (A.creating) {
        G.cv.wait(lock, [&] { return A.ready || stop_.load() || failed_.load(); });
        return A.ready;
    }
    A.creating = true;
    lock.unlock();
    const auto t_c0 = now();
    bool ok = ffs_stream_create(G.ctx, &A.s) == FFS_OK && (!G.vctx || ffs_stream_create(G.vctx, &A.v) == FFS_OK);
    const auto t_c1 = now();
    // chunks: B tight slots (the first chunk's size + 2 %: what lies in consecutive slots crosses PCIe as ONE copy --
    // a copy per chunk cost 5 % of the frame rate) and behind them an overflow area for the chunks that do not fit theirs
    const size_t batch = cfg_.batch;
    A.slot_bytes = cfg_.gpu_decode ? chunk_estimate_.load() : frame_bytes_;
    A.over_at = batch * A.slot_bytes;
    const size_t over = cfg_.gpu_decode ? std::max(batch * A.slot_bytes / 4, std::min(3 * A.slot_bytes, frame_bytes_ + 4096)) : 0;
    void* v = nullptr;
    ok = ok && ffs_stream_reserve_host(A.s, A.over_at + over) == FFS_OK && ffs_stream_host_buffer(A.s, &v, &A.host_bytes) == FFS_OK;
    A.host = static_cast<uint8_t*>(v);
    if (!ok) { fail("", G.ctx); return false; }
    lock.lock();
    A.ready = true;
    G.cv.notify_all();
    lock.unlock();
    if (cfg_.verbose) {
        std::lock_guard<std::mutex> pl(print_mutex_);
        std::printf("Thread %2d: assembly %u of GPU %d ready (stream %.1f ms, %.0f MB of staging %.1f ms) %.0f ms after the start\n", thread_id,
                    index, cfg_.gpus[G.index].device, secs(t_c0, t_c1) * 1e3, A.host_bytes / 1e6, secs(t_c1, now()) * 1e3, secs(cfg_.start, now()) * 1e3);
    }
    return true;
}

// image `image_num`'s chunk into dst, once the frame source has it.  false: stopped
bool BatchPipeline::read_chunk(ReaderState& R, uint32_t image_num, std::span<uint8_t> dst, std::span<uint8_t>& chunk) {
    const uint32_t offset_image_num = image_num + cfg_.start_index;  // :756
    // The images the readers are after right now, this one among them from here to the return (a reader parked at the reader mutex below
    // included): the time-out names the LOWEST of them, the first image the source did not deliver, whichever reader's patience ran out
    // first -- which of them that is depends on when each received its last image, not on the data.
    struct Awaited {
        BatchPipeline& p;
        const uint32_t image;
        Awaited(BatchPipeline& p_, uint32_t image_) : p(p_), image(image_) {
            std::lock_guard<std::mutex> l(p.awaited_mutex_);
            p.awaited_.insert(image);
        }
        ~Awaited() {
            std::lock_guard<std::mutex> l(p.awaited_mutex_);
            p.awaited_.erase(p.awaited_.find(image));
        }
        uint32_t lowest() const {
            std::lock_guard<std::mutex> l(p.awaited_mutex_);
            return *p.awaited_.begin();
        }
    } awaited(*this, offset_image_num);
    // readers are not thread-safe in general (:763-765); those that say they are skip the lock
    std::unique_lock<std::mutex> lock(reader_mutex_, std::defer_lock);
    if (!reader_.reentrant()) lock.lock();
    const auto w0 = now();
    while (!reader_.is_image_available(offset_image_num) && !stop_.load()) {
        if (secs(R.last_received, now()) > cfg_.timeout) {  // :776-787
            std::printf("Timeout waiting for image %u\n", awaited.lowest());
            stop_.store(true);
            wake_all();
            break;
        }
        std::this_thread::sleep_for(100ms);
    }
    if (stop_.load()) return false;
    R.last_received = now();
    time_waiting_.fetch_add(secs(w0, R.last_received));
    for (;;) {  // zero-length reads on /dev/shm: retry (:805-821)
        const auto c0 = now();
        chunk = reader_.get_raw_chunk(offset_image_num, dst);
        R.t_chunk += secs(c0, now());
        if (chunk.size() != 0) break;
        std::printf("\033[1mRace Condition?!?? Got buffer size 0 for image %u. Sleeping.\033[0m\n", image_num);
        std::this_thread::sleep_for(100ms);
        if (stop_.load() || failed_.load()) return false;
    }
    return true;
}

// batch b's assembly: claimed by the first of its readers to get here (in order: batch q - K must have been collected).
// false: stopped or failed
bool BatchPipeline::claim_assembly(ReaderState& R, Gpu& G, Assembly& A, uint64_t q, uint64_t b, uint32_t n_in_batch) {
    const auto t_b0 = now();
    std::unique_lock<std::mutex> lock(G.mu);
    G.cv.wait(lock, [&] { return A.batch == (int64_t)b || (A.batch == -1 && A.next_q == q) || stop_.load() || failed_.load(); });
    if (stop_.load() || failed_.load()) return false;
    if (A.batch == -1) {
        A.batch = (int64_t)b;
        A.n = n_in_batch;
        A.filled = 0;
        A.submitted = false;
        A.skipped = false;
        std::fill(A.slot_filled.begin(), A.slot_filled.end(), (uint8_t)0);
        A.over_used = 0;   // (before the lock is dropped below: the batch's other readers take the overflow area as soon as they see `ready`)
        if (!A.ready) {   // first use (usually made ahead, in reader_loop): the stream(s) and the pinned staging area, outside the lock
            lock.unlock();
            if (!ensure_assembly(G, A, (uint32_t)(q % K_), R.thread_id)) return false;
            lock.lock();
        }
        else {   // (a batch that went up through the heap may have made the library grow -- and move -- the staging area)
            void* v = nullptr;
            (void)ffs_stream_host_buffer(A.s, &v, &A.host_bytes);
            A.host = static_cast<uint8_t*>(v);
        }
    } else if (!A.ready) {
        G.cv.wait(lock, [&] { return A.ready || stop_.load() || failed_.load(); });
        if (!A.ready) return false;
    }
    R.t_blocked += secs(t_b0, now());
    return true;
}

// a chunk the GPU decodes: into slot k of the staging area, the overflow area behind the slots, or the heap.  `chunk` is what
// has been read already (have_chunk: into the reader's scratch) and comes back as where the chunk lies.  false: stopped
bool BatchPipeline::place_chunk(ReaderState& R, Assembly& A, uint32_t k, uint32_t image_num, std::span<uint8_t>& chunk, bool have_chunk) {
    uint8_t* slot = A.host + (size_t)k * A.slot_bytes;
    if (have_chunk && chunk.size() <= A.slot_bytes) {
        std::memcpy(slot, chunk.data(), chunk.size());
        chunk = {slot, chunk.size()};
    } else if (!have_chunk) {
        if (!read_chunk(R, image_num, {slot, A.slot_bytes}, chunk)) return false;
    }
    if (chunk.data() != slot || chunk.size() >= A.slot_bytes) {
        // larger than its slot (the read may have been cut): into the overflow area of the same staging buffer, one such
        // chunk at a time (its size is only known once it has been read: the area's free end is its buffer) ...
        bool placed = false;
        {
            std::lock_guard<std::mutex> over_lock(*A.over_mu);
            const size_t at = A.over_at + A.over_used;
            const size_t room = at < A.host_bytes ? A.host_bytes - at : 0;
            if (room >= 2 * A.slot_bytes) {
                if (!read_chunk(R, image_num, {A.host + at, room}, chunk)) return false;
                if (chunk.size() < room) {
                    placed = true;
                    A.over_used += (chunk.size() + 63) & ~(size_t)63;
                }
            }
        }
        if (!placed) {   // ... or, when that is full too, through the heap -- and so will its batch
            A.spill[k].resize(R.raw_bytes);
            if (!read_chunk(R, image_num, A.spill[k], chunk)) return false;
            A.spill[k].resize(chunk.size());
            chunk = {A.spill[k].data(), chunk.size()};
        }
    }
    A.chunk_ptr[k] = chunk.data();
    A.chunk_len[k] = chunk.size();
    return true;
}

// a frame the CPU decodes: the chunk into the reader's scratch, its pixels into the slot.  false: stopped
bool BatchPipeline::decode_into_slot(ReaderState& R, uint8_t* slot, uint32_t image_num) {
    std::span<uint8_t> chunk;
    if (!read_chunk(R, image_num, R.scratch(), chunk)) return false;
    const size_t n_px = (size_t)cfg_.width * cfg_.height;
    switch (reader_.get_raw_chunk_compression()) {  // decode outside the lock (:823-842)
    case Reader::BITSHUFFLE_LZ4:
        if (chunk.size() < 12 || bshuf_decompress_lz4(chunk.data() + 12, chunk.size() - 12, slot, n_px, cfg_.bytes_per_pixel) < 0) {
            std::printf("Error: corrupt bitshuffle-LZ4 chunk for image %u\n", image_num);
            fail();
        }
        break;
    case Reader::BYTE_OFFSET_32:
        if (cfg_.bytes_per_pixel == 2) byte_offset_decompress(chunk.data(), chunk.size(), reinterpret_cast<uint16_t*>(slot), n_px);
        else byte_offset_decompress(chunk.data(), chunk.size(), reinterpret_cast<uint32_t*>(slot), n_px);
        break;
    case Reader::NONE:
        if (cfg_.jungfrau_planes) {   // raw Jungfrau words: the rule the GPU kernel compiles (csrc/jungfrau_model.hpp), on this thread
            if (chunk.size() != n_px * 2) {
                std::printf("Error: image %u is %zu bytes, a frame of raw Jungfrau words is %zu\n", image_num, chunk.size(), n_px * 2);
                fail();
                break;
            }
            jungfrau_convert(reinterpret_cast<const uint16_t*>(chunk.data()), n_px, cfg_.jungfrau_planes, reinterpret_cast<uint32_t*>(slot));
            break;
        }
        std::memcpy(slot, chunk.data(), std::min(chunk.size(), frame_bytes_));
        break;
    }
    return true;
}

// ---- a reader: chunks from the frame source into the slots of its GPU's assemblies ----------------------------------------
void BatchPipeline::reader_loop(int thread_id) {
    const uint32_t di = (uint32_t)thread_id % n_dev_;
    const uint32_t batch = cfg_.batch;
    Gpu& G = *gpus_[di];
    pin_to(di);
    ReaderState R;
    R.thread_id = thread_id;
    // (a byte-offset section: seven bytes per pixel at the most -- what a read cuts off behind that is never parsed)
    R.raw_bytes = byte_offset_ ? (size_t)7 * cfg_.width * cfg_.height + 4096 : frame_bytes_ * (cfg_.bytes_per_pixel == 2 ? 2 : 1) + 4096;
    R.last_received = now();
    bool made_mine = false;
    while (!stop_.load() && !failed_.load()) {
        const uint64_t j = G.next_slot.fetch_add(1);
        const uint64_t q = j / batch, b = q * n_dev_ + di;
        const uint32_t k = (uint32_t)(j % batch);
        if (b >= total_batches_) break;
        const uint32_t first = (uint32_t)(b * batch);
        const uint32_t n_in_batch = std::min<uint32_t>(batch, cfg_.num_images - first);
        if (k >= n_in_batch) continue;   // (the last batch is short)
        const uint32_t image_num = first + k;
        Assembly& A = G.as[q % K_];

        // the first chunk anybody reads sizes the staging areas (chunks that the GPU decodes: B slots of that size + --slot-margin,
        // 2 %, + 16 KiB; the overflow area behind them is another 25 %: see ensure_assembly)
        std::span<uint8_t> chunk;
        bool have_chunk = false;
        const auto t_fill = now();
        if (cfg_.gpu_decode && chunk_estimate_.load() == 0) {
            if (!read_chunk(R, image_num, R.scratch(), chunk)) break;
            have_chunk = true;
            size_t expect = 0;
            chunk_estimate_.compare_exchange_strong(expect, ((chunk.size() + (size_t)(chunk.size() * (double)cfg_.slot_margin / 100.0) + 16384) + 63) & ~(size_t)63);
        }

        if (!made_mine) {   // the GPU's first K readers make one assembly each, side by side (see ensure_assembly)
            made_mine = true;
            const uint32_t local = (uint32_t)thread_id / n_dev_;
            if (local < K_ && !ensure_assembly(G, G.as[local], local, thread_id)) break;
        }
        if (!claim_assembly(R, G, A, q, b, n_in_batch)) break;

        A.spill[k].clear();
        if (cfg_.gpu_decode) {
            if (!place_chunk(R, A, k, image_num, chunk, have_chunk)) break;
        } else {
            if (!decode_into_slot(R, A.host + (size_t)k * A.slot_bytes, image_num)) break;
        }
        if (failed_.load()) break;
        ++R.n_read;
        R.t_read += secs(t_fill, now());

        bool last = false;
        {
            std::lock_guard<std::mutex> lock(G.mu);
            A.slot_filled[k] = 1;
            last = ++A.filled == A.n;
        }
        if (!last) continue;
        // the batch is complete: whoever filled its last slot sends it off
        const auto t_s0 = now();
        if (!submit_batch(G, A, A.n, first, thread_id)) break;
        ++R.n_submitted;
        R.t_submit += secs(t_s0, now());
        if (cfg_.verbose && b < 5) {
            std::lock_guard<std::mutex> lock(print_mutex_);
            std::printf("Thread %2d: batch %llu submitted %.1f ms after the start (the call took %.2f ms)\n", thread_id, (unsigned long long)b,
                        secs(cfg_.start, now()) * 1e3, secs(t_s0, now()) * 1e3);
        }
    }
    if (cfg_.verbose) {
        std::lock_guard<std::mutex> lock(print_mutex_);
        std::printf("Thread %2d: %u chunks read in %.0f ms (%.0f ms of it in get_raw_chunk), waiting for a free assembly %.0f ms, %u batches submitted (%.0f ms), "
                    "done %.0f ms after the start\n", thread_id, R.n_read, R.t_read * 1e3, R.t_chunk * 1e3, R.t_blocked * 1e3, R.n_submitted, R.t_submit * 1e3,
                    secs(cfg_.start, now()) * 1e3);
    }
}

// Readers that stopped early (a time-out: the data set ended before --images; an interrupt) leave batches half filled.  The
// reference's workers finish the image they hold, so every image that WAS read still goes through: the leading filled
// slots of such a batch are submitted as a shorter batch (images arrive in order; one behind a missing image is dropped).
void BatchPipeline::flush_half_filled() {
    for (uint32_t di = 0; di < n_dev_; ++di) {
        Gpu& G = *gpus_[di];
        for (Assembly& A : G.as) {
            uint32_t prefix = 0, first = 0;
            {
                std::lock_guard<std::mutex> lock(G.mu);
                if (A.batch < 0 || A.submitted || !A.ready) continue;
                while (prefix < A.n && A.slot_filled[prefix]) ++prefix;
                first = (uint32_t)((uint64_t)A.batch * cfg_.batch);
            }
            if (prefix > 0) (void)submit_batch(G, A, prefix, first, 0);
        }
    }
}

bool BatchPipeline::run(const BatchCallback& on_batch) {
    std::vector<std::thread> threads;
    for (uint32_t di = 0; di < n_dev_; ++di) threads.emplace_back([this, di, &on_batch] { collector_loop(di, on_batch); });
    for (uint32_t t = 0; t < cfg_.readers; ++t) threads.emplace_back([this, t] { reader_loop((int)t); });
    // A signal handler can only set the stop flag (nothing else is safe there), so somebody has to tell the threads parked on a GPU's
    // condition variable: readers waiting for a free assembly are woken by the collector only when a batch COMPLETES, and after an
    // interrupt none may -- the readers that hold its slots return without filling them.  (The reference's workers poll: :770-790.)
    std::atomic<bool> watch_over{false};
    std::thread stop_watcher([this, &watch_over] {
        bool told = false;
        while (!watch_over.load()) {
            if (!told && (stop_.load() || failed_.load())) {
                wake_all();
                told = true;
            }
            std::this_thread::sleep_for(20ms);
        }
    });
    for (size_t t = n_dev_; t < threads.size(); ++t) threads[t].join();   // the readers
    watch_over.store(true);
    stop_watcher.join();
    if (!failed_.load()) flush_half_filled();
    readers_done_.store(true);
    wake_all();                                                          // (collectors waiting for a batch nobody will submit)
    for (uint32_t di = 0; di < n_dev_; ++di) threads[di].join();
    // every result is out: the streams' buffers are released after the totals are printed, not on the clock
    for (auto& g : gpus_)
        for (Assembly& A : g->as) {
            if (A.s) retired_streams_.push_back(A.s);
            if (A.v) retired_streams_.push_back(A.v);
        }
    return !failed_.load();
}

}  // namespace ffshost
