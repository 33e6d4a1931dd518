// pipeline_check.cc -- host/batch_pipeline.cc against fake_ffs.cc and a frame source whose image i is a function of i: no GPU,
// no libffs_hip.so.  Built twice by tests/test_batch_pipeline_cpu.py (ThreadSanitizer; AddressSanitizer + UBSan).  Every case
// checks: each expected image reported exactly once, with the checksum of the bytes the reader produced for it; per GPU the
// batches come out in ascending order; global batch b went to GPU b mod n_dev; never more than K batches of a GPU in flight.
// Prints "FAIL ..." per broken expectation and ends with "OK" and exit code 0 when there was none.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>

#include "batch_pipeline.hpp"
#include "fake_ffs.hpp"

using namespace ffshost;
using namespace std::chrono_literals;

static std::atomic<int> g_failures{0};
static std::string g_case;
#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            ++g_failures;                                           \
            std::printf("FAIL [%s] %s: ", g_case.c_str(), #cond);   \
            std::printf(__VA_ARGS__);                               \
            std::printf("\n");                                      \
        }                                                           \
    } while (0)

// image i: `length(i)` bytes (raw frames: one frame's worth), byte p of it a function of (i, p); images >= available never come
class FakeReader : public Reader {
  public:
    uint32_t width = 8, height = 8, n_images = 0, available = 0;
    h5read_dtype dtype = H5READ_DTYPE_UINT16;
    ChunkCompression compression = NONE;
    bool is_reentrant = false;
    std::function<size_t(size_t)> length;
    std::atomic<int> inside{0}, overlaps{0};   // calls running at once: none may when the reader is not reentrant

    static uint8_t byte_of(size_t i, size_t p) { return (uint8_t)(i * 131 + p * 7 + (p >> 8) + (i >> 3)); }
    uint32_t checksum_of(size_t i) const {
        std::vector<uint8_t> b(length(i));
        for (size_t p = 0; p < b.size(); ++p) b[p] = byte_of(i, p);
        return fake::checksum(b.data(), b.size());
    }
    struct Call {
        FakeReader& r;
        explicit Call(FakeReader& r_) : r(r_) { if (r.inside.fetch_add(1) != 0 && !r.is_reentrant) r.overlaps += 1; }
        ~Call() { r.inside.fetch_sub(1); }
    };
    bool is_image_available(size_t index) override { Call c(*this); return index < available; }
    std::span<uint8_t> get_raw_chunk(size_t index, std::span<uint8_t> dst) override {
        Call c(*this);
        const size_t n = std::min(length(index), dst.size());   // (a read into too small a destination is cut, as the real readers' are)
        for (size_t p = 0; p < n; ++p) dst[p] = byte_of(index, p);
        return dst.first(n);
    }
    ChunkCompression get_raw_chunk_compression() override { return compression; }
    size_t get_number_of_images() const override { return n_images; }
    h5read_dtype get_dtype() const override { return dtype; }
    std::array<int64_t, 2> get_trusted_range() const override { return {0, 65535}; }
    std::array<size_t, 2> image_shape() const override { return {height, width}; }
    std::optional<std::span<const uint8_t>> get_mask() const override { return std::nullopt; }
    std::optional<float> get_wavelength() const override { return 1.0f; }
    std::optional<std::array<float, 2>> get_pixel_size() const override { return std::nullopt; }
    std::optional<std::array<float, 2>> get_beam_center() const override { return std::nullopt; }
    std::optional<float> get_detector_distance() const override { return std::nullopt; }
    std::array<float, 2> get_oscillation() const override { return {0.f, 0.f}; }
    bool reentrant() const override { return is_reentrant; }
};

struct Case {
    std::string name;
    uint32_t readers = 1, batch = 1, K = 1, gpus = 1, images = 23, available = 23, side = 8;
    size_t bytes_per_pixel = 2;
    bool reentrant = false, gpu_decode = false, read_only = false, validate = false;
    float timeout = 30.0f;
    std::function<size_t(size_t)> chunk_length;   // gpu_decode
    // what happens beside run(): called on the main thread while run() is on another; gets the stop flag and the pipeline
    std::function<void(std::atomic<bool>&, const BatchPipeline&)> beside;
    bool expect_ok = true;
    // images expected: exactly once each (exact), or at most once each and none else (!exact)
    uint32_t expect_images = 23;
    bool exact = true;
};

struct Outcome {
    std::vector<fake::Submit> submits;
    uint32_t completed = 0;
    bool ok = false, stop_was_set = false;
};

static Outcome run_case(const Case& c) {
    g_case = c.name;
    const size_t frame_bytes = (size_t)c.side * c.side * c.bytes_per_pixel;
    FakeReader reader;
    reader.width = reader.height = c.side;
    reader.n_images = c.images;
    reader.available = c.available;
    reader.dtype = c.bytes_per_pixel == 2 ? H5READ_DTYPE_UINT16 : H5READ_DTYPE_UINT32;
    reader.compression = c.gpu_decode ? Reader::BITSHUFFLE_LZ4 : Reader::NONE;
    reader.is_reentrant = c.reentrant;
    reader.length = c.gpu_decode ? c.chunk_length : [frame_bytes](size_t) { return frame_bytes; };

    PipelineConfig cfg;
    cfg.batch = c.batch;
    cfg.assemblies = c.K;
    cfg.readers = std::max(c.readers, c.gpus);   // (reader t serves GPU t mod n_dev: the driver starts at least one per GPU)
    cfg.gpu_decode = c.gpu_decode;
    cfg.read_only = c.read_only;
    cfg.timeout = c.timeout;
    cfg.num_images = c.images;
    cfg.width = cfg.height = c.side;
    cfg.bytes_per_pixel = c.bytes_per_pixel;
    cfg.start = std::chrono::steady_clock::now();
    for (uint32_t g = 0; g < c.gpus; ++g)   // context ids: GPU g -> g, its validation context -> 100 + g
        cfg.gpus.push_back({fake::make_ctx((int)g, frame_bytes), c.validate ? fake::make_ctx(100 + (int)g, frame_bytes) : nullptr, (int)g, std::nullopt});

    std::mutex mu;
    std::map<uint32_t, int> seen;            // image -> times reported
    std::vector<int64_t> last_q(c.gpus, -1);
    auto on_batch = [&mu, &seen, &last_q, &reader, &c](const BatchView& v) {
        std::lock_guard<std::mutex> lock(mu);
        CHECK(v.gpu < c.gpus && (int64_t)v.q > last_q[v.gpu], "GPU %u: batch %llu after %lld", v.gpu, (unsigned long long)v.q, (long long)last_q[v.gpu]);
        last_q[v.gpu] = (int64_t)v.q;
        const uint64_t b = v.q * c.gpus + v.gpu;   // global batch b is local batch b / n_dev of GPU b mod n_dev
        CHECK(v.count >= 1 && v.count <= c.batch && v.stream != nullptr && v.timings[4] == 5.0f, "count %u", v.count);
        CHECK((v.validation != nullptr) == c.validate, "validation results");
        for (uint32_t i = 0; i < v.count; ++i) {
            const uint32_t image = (uint32_t)v.results[i].frame_id;
            CHECK(image == b * c.batch + i, "image %u at place %u of batch %llu", image, i, (unsigned long long)b);
            CHECK(v.results[i].num_strong_pixels == reader.checksum_of(image), "image %u: not the bytes the reader produced", image);
            if (v.validation)
                CHECK(v.validation[i].frame_id == v.results[i].frame_id && v.validation[i].num_strong_pixels == v.results[i].num_strong_pixels,
                      "image %u: the validation context got another input", image);
            seen[image] += 1;
        }
        return true;
    };

    Outcome out;
    std::atomic<bool> stop{false};
    {
        BatchPipeline pipeline(cfg, reader, stop);
        if (c.beside) {
            std::thread runner([&pipeline, &on_batch, &out] { out.ok = pipeline.run(on_batch); });
            c.beside(stop, pipeline);
            runner.join();
        } else {
            out.ok = pipeline.run(on_batch);
        }
        out.completed = pipeline.images_completed();
        CHECK(pipeline.seconds_waiting_for_images() >= 0.0, "time waiting");
        CHECK(pipeline.streams_to_retire().size() <= (size_t)c.K * c.gpus * (c.validate ? 2 : 1), "%zu streams", pipeline.streams_to_retire().size());
        for (ffs_stream* s : pipeline.streams_to_retire()) ffs_stream_destroy(s);
    }
    out.stop_was_set = stop.load();
    out.submits = fake::submits();

    CHECK(out.ok == c.expect_ok, "run() returned %d", (int)out.ok);
    for (const auto& [image, times] : seen) CHECK(times == 1 && image < c.expect_images, "image %u reported %d times", image, times);
    if (c.exact) {
        CHECK(seen.size() == (c.read_only ? 0 : c.expect_images), "%zu images reported, %u expected", seen.size(), c.expect_images);
        CHECK(out.completed == c.expect_images, "%u images completed, %u expected", out.completed, c.expect_images);
    }
    for (const fake::Submit& s : out.submits) {
        const uint32_t b = s.first / c.batch;
        CHECK(s.first % c.batch == 0 && s.ctx % 100 == (int)(b % c.gpus), "batch %u (first image %u) went to context %d", b, s.first, s.ctx);
    }
    for (uint32_t g = 0; g < c.gpus; ++g) {
        CHECK(fake::max_in_flight((int)g) <= (int)c.K, "GPU %u: %d batches in flight, K = %u", g, fake::max_in_flight((int)g), c.K);
        CHECK(fake::streams_made((int)g) <= (int)c.K, "GPU %u: %d streams, K = %u", g, fake::streams_made((int)g), c.K);
    }
    CHECK(fake::protocol_errors() == 0, "%d protocol errors (a stream submitted again before its wait, ...)", fake::protocol_errors());
    CHECK(reader.overlaps.load() == 0, "%d overlapping calls into a reader that is not reentrant", reader.overlaps.load());
    return out;
}

template <typename Pred>
static bool poll_until(Pred p) {   // up to 20 s; the cases need milliseconds
    for (int i = 0; i < 20000 && !p(); ++i) std::this_thread::sleep_for(1ms);
    return p();
}

// ---- raw frames: readers x batch x K x GPUs over 23 images (no multiple of a batch size above 1: a short last batch) ----
static void raw_cases() {
    int n = 0;
    for (uint32_t readers : {1u, 3u, 8u})
        for (uint32_t batch : {1u, 4u, 6u})
            for (uint32_t K : {1u, 2u, 4u})
                for (uint32_t gpus : {1u, 2u}) {
                    Case c;
                    c.name = "raw readers=" + std::to_string(readers) + " batch=" + std::to_string(batch) + " K=" + std::to_string(K) + " gpus=" + std::to_string(gpus);
                    c.readers = readers; c.batch = batch; c.K = K; c.gpus = gpus;
                    c.reentrant = n % 2 == 0;
                    c.side = n % 3 == 0 ? 16 : 8;
                    c.bytes_per_pixel = n % 5 == 0 ? 4 : 2;
                    c.validate = n % 7 == 0;
                    ++n;
                    const Outcome o = run_case(c);
                    uint32_t submitted = 0;
                    for (const auto& s : o.submits) if (s.ctx < 100) submitted += s.n;
                    CHECK(submitted == 23 && !o.stop_was_set, "%u images submitted", submitted);
                    fake::reset();
                }
}

// ---- chunks the GPU decodes: slot, overflow area, heap --------------------------------------------------------------------
// 64 x 64 pixels of 16 bits, not smaller: a slot is the first chunk + 2 % + 16 KiB, and no chunk is longer than a reader's scratch
// (4 W H + 4096 bytes), so below 56 x 56 no chunk can outgrow its slot.  Small chunks are 300 bytes: slots of 16704 bytes, B = 8
// of them and an overflow area of max(8 * 16704 / 4, min(3 * 16704, 8192 + 4096)) = 33408 bytes = two slots -- room for ONE chunk
// of 18000 bytes (the area takes a chunk only while two slots' worth are free).  Batch 1 has one such chunk (image 10: overflow
// area), batch 2 two (images 17, 19: one in the overflow area, one in the heap -- and with it the whole batch), batch 4 one.
static void chunk_cases() {
    const size_t slot = 16704;
    for (uint32_t readers : {1u, 3u})
        for (bool move : {false, true}) {
            Case c;
            c.name = std::string("chunks readers=") + std::to_string(readers) + (move ? " buffer moves" : "");
            c.readers = readers; c.batch = 8; c.K = 2; c.gpus = 1; c.images = c.available = c.expect_images = 40;
            c.side = 64;
            c.gpu_decode = true;
            c.reentrant = readers == 3;
            c.chunk_length = [](size_t i) -> size_t { return (i == 10 || i == 17 || i == 19 || i == 33) ? 18000 : 300 + i % 7; };
            fake::move_buffer_after_heap_batch(move);
            const Outcome o = run_case(c);
            int in_slot = 0, in_overflow = 0, in_heap = 0;
            for (const auto& s : o.submits) {
                int outside = 0;
                for (uint32_t i = 0; i < s.n; ++i) {
                    const long long at = s.offset[i];
                    if (at < 0) { ++outside; ++in_heap; }
                    else if (at == (long long)(i * slot)) ++in_slot;
                    else if (at >= (long long)(c.batch * slot)) ++in_overflow;
                    else CHECK(false, "image %u lies at %lld: neither its slot nor the overflow area", s.first + i, at);
                }
                CHECK(outside == 0 || outside == (int)s.n, "batch of image %u: %d of %u chunks from the heap", s.first, outside, s.n);
                CHECK((outside != 0) == (s.first == 16), "batch of image %u: %d chunks from the heap", s.first, outside);
            }
            // 40 chunks: batch 2's eight from the heap; of the others, images 10 and 33 in the overflow area
            CHECK(in_slot == 30 && in_overflow == 2 && in_heap == 8, "placements: %d slot, %d overflow, %d heap", in_slot, in_overflow, in_heap);
            CHECK(fake::buffer_moves() == (move ? 1 : 0), "%d moves of a staging area", fake::buffer_moves());
            fake::reset();
        }
}

// ---- the source ends early: images >= 14 never come, the readers give up after 0.3 s ---------------------------------------
// With a reentrant reader every image below 14 is read at once and comes out.  A reader that is not reentrant is polled UNDER the
// reader mutex (as the reference does, :763-790), and the mutex is not fair: while the thread that waits for image 14 holds it,
// the (at most two) other threads return without having read the images they claimed.  Then batches 0 and 1 are complete (image 14
// is read into batch 3's assembly, which batch 1 had to leave first), and of batches 2 and 3 the leading run of what was read
// is submitted -- each image once at the most.  (When image 8 is among the unread, batch 2 is not submitted at all and the
// collector, which stops at the first batch that is missing, leaves a submitted run of batch 3 uncollected.)  So the variant
// with a reader that is not reentrant DELIBERATELY asserts less than "every image below 14 exactly once": making that hold means
// polling outside the reader mutex and collecting past a missing batch, a change of the protocol ("Known
// gap"), not of where its code lives.
static void early_end_cases() {
    for (uint32_t variant = 0; variant < 3; ++variant) {
        const bool reentrant = variant < 2;
        Case c;
        c.gpus = variant == 1 ? 2 : 1;
        c.name = "source ends early gpus=" + std::to_string(c.gpus) + (reentrant ? "" : " reader not reentrant");
        c.readers = 3; c.batch = 4; c.K = 2; c.available = c.expect_images = 14;
        c.reentrant = reentrant;
        c.exact = reentrant;
        c.timeout = 0.3f;
        const Outcome o = run_case(c);
        CHECK(o.stop_was_set, "the time-out sets the stop flag");
        uint32_t of_batch_3 = 0, submitted = 0;   // batch 3 = images 12..15: its leading filled slots, 12 and 13
        for (const auto& s : o.submits) {
            submitted += s.n;
            if (s.first == 12) of_batch_3 = s.n;
        }
        if (reentrant) CHECK(of_batch_3 == 2 && o.submits.size() == 4 && o.completed == submitted, "the half-filled batch goes up as its two leading slots (%zu submits)", o.submits.size());
        else CHECK(o.completed >= 8 && o.completed <= submitted && submitted <= 14 && of_batch_3 <= 2, "%u images completed, %u submitted, %u of batch 3", o.completed, submitted, of_batch_3);
        fake::reset();
    }
}

// ---- stop while parked: ffs_wait blocks, all K assemblies of both GPUs are in flight, the readers wait for a free one ---------
static void stop_while_parked() {
    Case c;
    c.name = "stop while parked";
    c.readers = 8; c.batch = 2; c.K = 2; c.gpus = 2; c.images = c.available = 200;
    c.reentrant = true;
    c.expect_images = 8;   // K batches of two images on each of two GPUs: what was submitted comes out, nothing else
    fake::block_waits();
    c.beside = [](std::atomic<bool>& stop, const BatchPipeline& pipeline) {
        const bool all_in_flight = poll_until([] { return fake::submits_so_far() == 4; });
        CHECK(all_in_flight, "%d batches submitted", fake::submits_so_far());
        std::this_thread::sleep_for(50ms);   // (nothing shows a reader arriving at the condition variable: this lets them)
        stop.store(true);
        // The collectors sit in ffs_wait, so no batch completes and nobody but the stop watcher can wake the parked readers:
        // they must all have left -- run() has joined them -- BEFORE the fake lets a wait return.
        bool readers_left = false;
        for (int i = 0; i < 5000 && !(readers_left = pipeline.readers_have_ended()); ++i) std::this_thread::sleep_for(1ms);
        CHECK(readers_left, "the readers are still parked 5 s after the stop flag was set: nobody told them");
        fake::release_waits();
    };
    const Outcome o = run_case(c);
    CHECK(o.submits.size() == 4, "%zu submits", o.submits.size());
    fake::reset();
}

// ---- a submit fails while other readers are parked: K = 3, the third submit fails, five readers wait for assembly 0 -------------
static void failing_submit() {
    Case c;
    c.name = "failing submit";
    c.readers = 8; c.batch = 2; c.K = 3; c.gpus = 1; c.images = c.available = 200;
    c.expect_ok = false;
    c.exact = false;
    c.expect_images = 6;   // (two of the batches 0, 1, 2 went through; a collector that sees the failure stops)
    fake::block_waits();
    fake::fail_submit(3);
    c.beside = [](std::atomic<bool>&, const BatchPipeline&) {
        CHECK(poll_until([] { return fake::submit_has_failed(); }), "the third submit");
        std::this_thread::sleep_for(50ms);
        fake::release_waits();
    };
    const Outcome o = run_case(c);
    CHECK(o.submits.size() == 2 && !o.stop_was_set, "%zu submits went through", o.submits.size());
    fake::reset();
}

static void read_only() {
    Case c;
    c.name = "read only";
    c.readers = 3; c.batch = 4; c.K = 2; c.gpus = 2;
    c.read_only = true;
    const Outcome o = run_case(c);
    CHECK(o.submits.empty(), "%zu submits", o.submits.size());
    fake::reset();
}

int main() {
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    raw_cases();
    chunk_cases();
    early_end_cases();
    stop_while_parked();
    failing_submit();
    read_only();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures.load());
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
