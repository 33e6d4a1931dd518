// fake_ffs.cc -- the ffs_* functions host/batch_pipeline.cc references, on the CPU: staging areas are malloc'ed, a submit
// checksums every frame's bytes as it received them (the slot contents for ffs_submit, the chunk pointer / length pairs for
// ffs_submit_encoded) and ffs_wait returns them as results: frame_id = first + i, the checksum in num_strong_pixels.
// The bytes are read BEFORE the fake takes its own lock: what orders the readers' writes into the staging area before the
// submit has to be the pipeline's own synchronisation, not the fake's.
#include "fake_ffs.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <map>
#include <mutex>

struct ffs_ctx {
    int id = 0;
    size_t frame_bytes = 0;
};

struct ffs_stream {
    ffs_ctx* ctx = nullptr;
    uint8_t* buf = nullptr;
    size_t bytes = 0;
    bool outstanding = false;
    std::vector<ffs_frame_result> results;
};

namespace {
struct State {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<ffs_ctx*> ctxs;
    std::vector<fake::Submit> submits;
    std::map<int, int> in_flight, max_in_flight, streams_made;
    int n_submit_calls = 0, fail_nth = 0, moves = 0, protocol_errors = 0, live_streams = 0;
    bool blocked = false, failed = false, move_after_heap = false;
} g;

// the common part of both submits, after the frames' checksums have been taken
int record_submit(ffs_stream* s, fake::Submit&& rec, const std::vector<uint32_t>& sums, bool from_heap) {
    std::lock_guard<std::mutex> lock(g.mu);
    if (++g.n_submit_calls == g.fail_nth) {
        g.failed = true;
        return FFS_ERR_DEVICE;
    }
    if (s->outstanding) ++g.protocol_errors;
    s->outstanding = true;
    s->results.assign(rec.n, ffs_frame_result{});
    for (uint32_t i = 0; i < rec.n; ++i) {
        s->results[i].frame_id = (int64_t)rec.first + i;
        s->results[i].num_strong_pixels = sums[i];
    }
    if (from_heap && g.move_after_heap) {   // (the library copies such a batch into a staging area made large enough for it)
        std::free(s->buf);
        s->bytes *= 2;
        s->buf = static_cast<uint8_t*>(std::malloc(s->bytes));
        ++g.moves;
    }
    const int id = s->ctx->id;
    g.max_in_flight[id] = std::max(g.max_in_flight[id], ++g.in_flight[id]);
    g.submits.push_back(std::move(rec));
    return FFS_OK;
}
}  // namespace

extern "C" {

int ffs_stream_create(ffs_ctx* ctx, ffs_stream** out) {
    auto* s = new ffs_stream;
    s->ctx = ctx;
    std::lock_guard<std::mutex> lock(g.mu);
    ++g.streams_made[ctx->id];
    ++g.live_streams;
    *out = s;
    return FFS_OK;
}

void ffs_stream_destroy(ffs_stream* s) {
    std::free(s->buf);
    delete s;
    std::lock_guard<std::mutex> lock(g.mu);
    --g.live_streams;
}

int ffs_stream_reserve_host(ffs_stream* s, size_t bytes) {
    if (bytes > s->bytes) {
        std::free(s->buf);
        s->buf = static_cast<uint8_t*>(std::malloc(bytes));
        s->bytes = bytes;
    }
    return s->buf ? FFS_OK : FFS_ERR_NOMEM;
}

int ffs_stream_host_buffer(ffs_stream* s, void** ptr, size_t* bytes) {
    *ptr = s->buf;
    *bytes = s->bytes;
    return FFS_OK;
}

int ffs_submit(ffs_stream* s, const void* host_pixels, uint32_t n_frames, int64_t first_frame_id) {
    const size_t frame_bytes = s->ctx->frame_bytes;
    const uint8_t* px = static_cast<const uint8_t*>(host_pixels);
    std::vector<uint32_t> sums(n_frames);
    for (uint32_t i = 0; i < n_frames; ++i) sums[i] = fake::checksum(px + (size_t)i * frame_bytes, frame_bytes);
    fake::Submit rec;
    rec.ctx = s->ctx->id;
    rec.first = (uint32_t)first_frame_id;
    rec.n = n_frames;
    rec.buffer_bytes = s->bytes;
    if (s->buf && (px != s->buf || (size_t)n_frames * frame_bytes > s->bytes)) {   // (a validation stream has no staging area of its own)
        std::lock_guard<std::mutex> lock(g.mu);
        ++g.protocol_errors;
    }
    return record_submit(s, std::move(rec), sums, false);
}

int ffs_submit_encoded(ffs_stream* s, int, const void* const* chunks, const size_t* chunk_bytes, uint32_t n_frames, int64_t first_frame_id) {
    std::vector<uint32_t> sums(n_frames);
    fake::Submit rec;
    rec.ctx = s->ctx->id;
    rec.first = (uint32_t)first_frame_id;
    rec.n = n_frames;
    rec.encoded = true;
    rec.buffer_bytes = s->bytes;
    bool from_heap = false;
    for (uint32_t i = 0; i < n_frames; ++i) {
        const uint8_t* p = static_cast<const uint8_t*>(chunks[i]);
        sums[i] = fake::checksum(p, chunk_bytes[i]);
        const bool inside = p >= s->buf && p + chunk_bytes[i] <= s->buf + s->bytes;
        rec.offset.push_back(inside ? (long long)(p - s->buf) : -1);
        from_heap = from_heap || !inside;
    }
    return record_submit(s, std::move(rec), sums, from_heap);
}

int ffs_wait(ffs_stream* s, const ffs_frame_result** results, uint32_t* n_results) {
    std::unique_lock<std::mutex> lock(g.mu);
    g.cv.wait(lock, [] { return !g.blocked; });
    if (!s->outstanding) ++g.protocol_errors;
    s->outstanding = false;
    --g.in_flight[s->ctx->id];
    *results = s->results.data();
    *n_results = (uint32_t)s->results.size();
    return FFS_OK;
}

int ffs_stream_timings(ffs_stream*, float ms[5]) {
    for (int i = 0; i < 5; ++i) ms[i] = 1.0f + i;
    return FFS_OK;
}

const char* ffs_last_error(const ffs_ctx*) { return "injected device error"; }

}  // extern "C"

namespace fake {

uint32_t checksum(const uint8_t* p, size_t n) {
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

ffs_ctx* make_ctx(int id, size_t frame_bytes) {
    auto* c = new ffs_ctx{id, frame_bytes};
    std::lock_guard<std::mutex> lock(g.mu);
    g.ctxs.push_back(c);
    return c;
}

void reset() {
    std::lock_guard<std::mutex> lock(g.mu);
    if (g.live_streams != 0) std::abort();
    for (ffs_ctx* c : g.ctxs) delete c;
    g.ctxs.clear();
    g.submits.clear();
    g.in_flight.clear();
    g.max_in_flight.clear();
    g.streams_made.clear();
    g.n_submit_calls = g.fail_nth = g.moves = g.protocol_errors = 0;
    g.blocked = g.failed = g.move_after_heap = false;
}

void block_waits() { std::lock_guard<std::mutex> lock(g.mu); g.blocked = true; }
void release_waits() { std::lock_guard<std::mutex> lock(g.mu); g.blocked = false; g.cv.notify_all(); }
void fail_submit(int nth) { std::lock_guard<std::mutex> lock(g.mu); g.fail_nth = nth; }
void move_buffer_after_heap_batch(bool on) { std::lock_guard<std::mutex> lock(g.mu); g.move_after_heap = on; }

std::vector<Submit> submits() { std::lock_guard<std::mutex> lock(g.mu); return g.submits; }
int submits_so_far() { std::lock_guard<std::mutex> lock(g.mu); return (int)g.submits.size(); }
bool submit_has_failed() { std::lock_guard<std::mutex> lock(g.mu); return g.failed; }
int max_in_flight(int ctx) { std::lock_guard<std::mutex> lock(g.mu); return g.max_in_flight[ctx]; }
int streams_made(int ctx) { std::lock_guard<std::mutex> lock(g.mu); return g.streams_made[ctx]; }
int buffer_moves() { std::lock_guard<std::mutex> lock(g.mu); return g.moves; }
int protocol_errors() { std::lock_guard<std::mutex> lock(g.mu); return g.protocol_errors; }

}  // namespace fake
