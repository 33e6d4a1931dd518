// ffs_encoded.hip -- encoded input from entry point to teardown: bitshuffle-LZ4 chunks (kernels_decode.hpp), CBF byte-offset chunks
// (kernels_byteoffset.hpp) and raw Jungfrau words (kernels_jungfrau.hpp) cross PCIe as they lie in the file and are decoded into the stream's
// pitched device image, which enqueue_batch (ffs_submit.hip) then takes like any other.  The decoders' kernels are included here and nowhere
// else.  What is decided about a batch -- may a chunk be a frame, where do the chunks lie, which bytes are copied, the tables the kernels
// read -- is encoded_plan.hpp's, without HIP; this unit allocates, copies, records and launches.  The codec is looked at by prepare and
// launch (and the chunk check) only.  The dark-frame fold of raw Jungfrau words (kernels_jfped.hpp; at the end of this file, from begin to
// end) reuses the chunk placement and the upload.
#include "ffs_internal.hpp"
#include "kernels_decode.hpp"
#include "kernels_byteoffset.hpp"
#include "kernels_jungfrau.hpp"
#include "kernels_jfped.hpp"

static_assert(sizeof(BlockEntry) == sizeof(uint2), "DecodeArgs::table reads the block table as uint2");

const char* encoded_corruption(uint32_t overflow) {
    if (overflow & kOvfCorruptLz4) return "corrupt bitshuffle-LZ4 chunk: an LZ4 block did not decode to its block size";
    if (overflow & kOvfCorruptByteOffset) return "corrupt byte-offset chunk: it holds fewer elements than the frame has pixels";
    return nullptr;
}

void encoded_free(ffs_stream* s) {
    EncodedState& E = s->enc;
    for (void* p : {(void*)E.d_comp, (void*)E.d_tab, (void*)E.d_bo_frames, (void*)E.d_bo_lane, (void*)E.d_bo_map, (void*)E.d_bo_state}) (void)hipFree(p);
    for (void* p : {(void*)E.h_tab, (void*)E.h_bo_frames}) (void)hipHostFree(p);
    E = EncodedState{};
}

// a table of max_batch rows the host writes and a kernel reads: its device and pinned host copies, made on first use
template <typename T>
static bool ensure_table(T** dev, T** host, size_t bytes) {
    if (*dev) return true;
    if (dmalloc(dev, bytes) == hipSuccess && hipHostMalloc(reinterpret_cast<void**>(host), bytes, hipHostMallocDefault) == hipSuccess) return true;
    (void)hipGetLastError();
    (void)hipFree(*dev);   // (both or neither: the next batch tries again)
    *dev = nullptr;
    return false;
}

// A batch whose chunks are on their way to the device: what prepare leaves for launch
struct EncodedBatch {
    int codec = FFS_CODEC_BSLZ4;
    std::vector<size_t> base, sizes;   // per chunk: its offset in the staging buffer and in d_comp, its bytes
    uint32_t bo_max_tiles = 0;         // byte-offset: tiles of the longest chunk, the launches' grid
};

// byte-offset chunks need no index: the frame table is written and the summary tables are sized here, on the caller's thread
static int prepare_byte_offset(ffs_stream* s, EncodedBatch& b) {
    ffs_ctx* c = s->ctx;
    EncodedState& E = s->enc;
    if (!ensure_table(&E.d_bo_frames, &E.h_bo_frames, (size_t)s->max_batch * sizeof(BoFrame)))
        return refuse(c->err, FFS_ERR_NOMEM, "allocation of the byte-offset frame table failed");
    const BoTiles t = bo_frame_table(b.base.data(), b.sizes.data(), (uint32_t)b.base.size(), (uint64_t)c->L.W * c->L.H, E.h_bo_frames);
    b.bo_max_tiles = t.max_tiles;
    if (t.sum <= E.bo_tiles_cap) return FFS_OK;
    // (the stream is idle, but its last decode may still read the tables on a decode-only path: they are freed behind both streams)
    if (E.d_bo_lane) {
        HIP_TRY(c, hipStreamSynchronize(s->st_up));
        HIP_TRY(c, hipStreamSynchronize(s->st));
    }
    (void)hipFree(E.d_bo_lane); (void)hipFree(E.d_bo_map); (void)hipFree(E.d_bo_state);
    E.d_bo_lane = nullptr; E.d_bo_map = nullptr; E.d_bo_state = nullptr;
    E.bo_tiles_cap = 0;
    const size_t want = t.sum + t.sum / 4 + 16;
    if (dmalloc(&E.d_bo_lane, want * 7 * 64 * sizeof(uint2)) != hipSuccess || dmalloc(&E.d_bo_map, want * 7 * sizeof(uint2)) != hipSuccess
        || dmalloc(&E.d_bo_state, want * sizeof(uint4)) != hipSuccess) {
        (void)hipGetLastError();
        return refuse(c->err, FFS_ERR_NOMEM, "allocation of the byte-offset summary tables failed");
    }
    E.bo_tiles_cap = want;
    return FFS_OK;
}

// Caller's thread: checks the chunks, places them in the pinned staging buffer (unless they already are there), starts their copy to the
// device and records ev[6] behind it.  A failure leaves no copy reading memory the caller gets back.
// fold: the caller is the dark-frame fold (its name, for the texts), which converts nothing and needs no calibration; else null.
static int prepare(ffs_stream* s, int codec, const void* const* chunks, const size_t* chunk_bytes, uint32_t n, EncodedBatch& b, const char* fold = nullptr) {
    ffs_ctx* c = s->ctx;
    EncodedState& E = s->enc;
    const size_t W = (size_t)c->L.W, H = (size_t)c->L.H, es = (size_t)c->settings.pixel_bytes;
    const bool byte_offset = codec == FFS_CODEC_BYTE_OFFSET, jungfrau = codec == FFS_CODEC_JUNGFRAU_RAW;
    b.codec = codec;
    if (!byte_offset && !jungfrau && !E.d_tab) {
        E.blocking = bshuf_blocking(W * H, es);
        if (!ensure_table(&E.d_tab, &E.h_tab, (size_t)s->max_batch * (E.blocking.blocks + 1) * sizeof(BlockEntry)))
            return refuse(c->err, FFS_ERR_NOMEM, "allocation of the compressed-chunk buffers failed");
    }
    std::string why;
    for (uint32_t f = 0; f < n; ++f)
        if (!chunk_ok(codec, chunks[f], chunk_bytes[f], W, H, es, why)) return refuse(c->err, FFS_ERR_INVALID, why);
    Placement pl;
    if (!place_chunks(chunks, chunk_bytes, n, s->h_img, s->h_img_bytes, b.base, pl))
        return refuse(c->err, FFS_ERR_INVALID, "ffs_submit_compressed: either all chunks lie in the stream's host buffer or none");
    if (jungfrau) {   // (no table: the conversion reads the context's calibration and the chunks where they lie)
        if (!fold && !c->settings.jungfrau_calibration)
            return refuse(c->err, FFS_ERR_INVALID, "ffs_submit_encoded: raw Jungfrau words need a calibration and the context has none (ffs_ctx_set_jungfrau_calibration)");
        if (const uint32_t f = first_unaligned_base(b.base.data(), n); f < n)
            return refuse(c->err, FFS_ERR_INVALID, std::string(fold ? fold : "ffs_submit_encoded") + ": raw Jungfrau chunk " + std::to_string(f) + " lies in the stream's host buffer at offset "
                                                       + std::to_string(b.base[f]) + ", which is not a multiple of 16");
    }
    if (!pl.in_place) {
        FFS_TRY(ensure_host_staging(s, pl.staging));   // (grows with headroom; kept from then on)
        for (uint32_t f = 0; f < n; ++f) std::memcpy(s->h_img + b.base[f], chunks[f], chunk_bytes[f]);
    }
    if (pl.hi > kMaxStagedBytes) return refuse(c->err, FFS_ERR_INVALID, "ffs_submit_compressed: more than 4 GiB of chunks in one batch");
    if (E.d_comp_bytes < pl.hi + 64) {   // the device side of the staging area follows its size (hipMalloc is cheap)
        if (E.d_comp) HIP_TRY(c, hipStreamSynchronize(s->st_up));
        (void)hipFree(E.d_comp);
        E.d_comp = nullptr;
        E.d_comp_bytes = 0;
        const size_t want = std::max(pl.hi + pl.hi / 4 + 4096, s->h_img_bytes) + 64;
        if (dmalloc(&E.d_comp, want) != hipSuccess) {
            (void)hipGetLastError();
            return refuse(c->err, FFS_ERR_NOMEM, "allocation of the device buffer for compressed chunks failed");
        }
        E.d_comp_bytes = want;
    }
    if (pl.in_place) {
        std::vector<std::pair<size_t, size_t>> ranges;   // (each copy costs ~10 us of the caller's time)
        copy_ranges(b.base.data(), chunk_bytes, n, ranges);
        for (const auto& [begin, end] : ranges) HIP_TRY(c, hipMemcpyAsync(E.d_comp + begin, s->h_img + begin, end - begin, hipMemcpyHostToDevice, s->st_up));
    } else {
        HIP_TRY(c, hipMemcpyAsync(E.d_comp + pl.lo, s->h_img + pl.lo, pl.hi - pl.lo, hipMemcpyHostToDevice, s->st_up));
    }
    // "this batch's chunks are on the device", recorded HERE: the upload stream is shared by the context's streams, and an event
    // recorded later (by the helper thread, after the block index) would also wait for every other batch's chunks queued meanwhile
    HIP_TRY(c, hipEventRecord(s->ev[6], s->st_up));
    b.sizes.assign(chunk_bytes, chunk_bytes + n);
    if (!byte_offset) return FFS_OK;
    const int rc = prepare_byte_offset(s, b);
    if (rc != FFS_OK) (void)hipStreamSynchronize(s->st_up);   // (the chunks' copy reads the staging buffer the caller gets back)
    return rc;
}

// bitshuffle-LZ4 (may run on the stream's helper thread while the chunks cross PCIe): indexes the blocks -- a pointer chase of ~2 ms for 32
// Eiger frames, on up to four threads -- and enqueues the table's copy.  Errors go to `err`, not to the context (another thread may own
// that string).
static int index_blocks(ffs_stream* s, const EncodedBatch& b, hipStream_t st, std::string& err) {
    EncodedState& E = s->enc;
    const uint32_t n = (uint32_t)b.base.size(), nb = E.blocking.blocks;
    const size_t tail = (size_t)E.blocking.tail_elems * s->ctx->settings.pixel_bytes;
    std::vector<size_t> pos(n, 12);
    std::atomic<bool> ok{true};
    static const bool trace = std::getenv("FFS_TRACE_SUBMIT") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto walk = [&](uint32_t f0, uint32_t f1) {
        if (!walk_block_chains(s->h_img, b.base.data(), b.sizes.data(), pos.data(), f0, f1, nb, tail, E.h_tab)) ok = false;
    };
    const uint32_t n_thr = (uint64_t)n * nb >= 32768 ? std::min<uint32_t>(4, n) : 1;
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < n_thr; ++t) th.emplace_back(walk, n * t / n_thr, n * (t + 1) / n_thr);
    walk(0, n / n_thr);
    for (auto& t : th) t.join();
    if (trace)
        std::fprintf(stderr, "[ffs] indexed %u blocks in %.3f ms (%u threads)\n", n * nb,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), n_thr);
    if (!ok) return refuse(err, FFS_ERR_INVALID, "ffs_submit_compressed: block lengths run past the end of a chunk");
    // (the table goes up in the stream the decode kernel runs in: half a megabyte that must not queue behind other batches' chunks)
    const hipError_t e = hipMemcpyAsync(E.d_tab, E.h_tab, (size_t)n * (nb + 1) * sizeof(BlockEntry), hipMemcpyHostToDevice, st);
    return e == hipSuccess ? FFS_OK : refuse(err, FFS_ERR_DEVICE, std::string("hipMemcpyAsync(block table): ") + hipGetErrorString(e));
}

// Puts a prepared batch's decode into `st`: the table its kernels read (with_table: the block index or the frame table, copied in `st`) and
// the kernels (with_decode: one launch, byte-offset: summarise, compose, emit).  after: an event `st` waits for ahead of the kernels, or
// null -- the block table does not wait for it, it is indexed from the host's copy while the chunks still travel; done: an event recorded
// in `st` behind the kernels, or null.  Errors go to `err`.
static int launch(ffs_stream* s, const EncodedBatch& b, hipStream_t st, bool with_table, bool with_decode, hipEvent_t after, hipEvent_t done, std::string& err) {
    ffs_ctx* c = s->ctx;
    EncodedState& E = s->enc;
    const Layout& L = c->L;
    const bool byte_offset = b.codec == FFS_CODEC_BYTE_OFFSET, jungfrau = b.codec == FFS_CODEC_JUNGFRAU_RAW;
    const uint32_t n = (uint32_t)b.base.size();
    if (with_table && !byte_offset && !jungfrau) FFS_TRY(index_blocks(s, b, st, err));
    if (with_table) (void)hipGetLastError();
    hipError_t e = after ? hipStreamWaitEvent(st, after, 0) : hipSuccess;
    if (e == hipSuccess && with_table && byte_offset) e = hipMemcpyAsync(E.d_bo_frames, E.h_bo_frames, (size_t)n * sizeof(BoFrame), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && with_decode && byte_offset) {
        const BoArgs a{.comp = E.d_comp, .frames = E.d_bo_frames, .lane_pre = E.d_bo_lane, .tile_map = E.d_bo_map, .tile_state = E.d_bo_state,
                       .image = s->d_img, .frame_stride = L.frame_stride, .pitch = L.pitch, .W = (uint32_t)L.W, .H = (uint32_t)L.H, .error = s->d_overflow};
        const dim3 grid(b.bo_max_tiles, n);
        hipLaunchKernelGGL(k_bo_summarise, grid, dim3(64), 0, st, a);
        hipLaunchKernelGGL(k_bo_compose, dim3(n), dim3(64), 0, st, a);
        if (c->settings.pixel_bytes == 2) hipLaunchKernelGGL(k_bo_emit<uint16_t>, grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL(k_bo_emit<uint32_t>, grid, dim3(64), 0, st, a);
    } else if (e == hipSuccess && with_decode && jungfrau) {
        // one launch for up to kJfMaxFrames frames, whose bases travel in its arguments; a lane per group of eight pixels of the flat frame
        const uint32_t n_px = (uint32_t)L.W * (uint32_t)L.H, groups = (n_px + kJfLanePixels - 1) / kJfLanePixels;
        const dim3 grid((groups + kJfBlock - 1) / kJfBlock);
        for (uint32_t f0 = 0; f0 < n; f0 += kJfMaxFrames) {
            JfArgs a{.comp = E.d_comp, .planes = c->d_jf_cal, .plane_stride = c->jf_plane_stride, .image = s->d_img + (uint64_t)f0 * L.frame_stride,
                     .frame_stride = L.frame_stride, .pitch = L.pitch, .W = (uint32_t)L.W, .n_px = n_px, .n_frames = std::min(n - f0, kJfMaxFrames), .base = {}};
            for (uint32_t f = 0; f < a.n_frames; ++f) a.base[f] = (uint32_t)b.base[f0 + f];
            if (L.W % kJfLanePixels == 0) hipLaunchKernelGGL(k_jungfrau_raw<true>, grid, dim3(kJfBlock), 0, st, a);
            else hipLaunchKernelGGL(k_jungfrau_raw<false>, grid, dim3(kJfBlock), 0, st, a);
        }
    } else if (e == hipSuccess && with_decode) {
        const BshufBlocking& k = E.blocking;
        const DecodeArgs da{.comp = E.d_comp, .table = reinterpret_cast<const uint2*>(E.d_tab), .image = s->d_img, .frame_stride = L.frame_stride,
                            .pitch = L.pitch, .W = L.W, .H = L.H, .elem_bytes = c->settings.pixel_bytes, .blocks_per_frame = k.blocks, .block_elems = k.block_elems,
                            .last_block_elems = k.last_elems, .tail_elems = k.tail_elems, .error = s->d_overflow};
        const dim3 grid(k.blocks + 1, n);
        if (c->settings.pixel_bytes == 2) hipLaunchKernelGGL(k_bshuf_lz4_decode<2>, grid, dim3(64), 0, st, da);
        else hipLaunchKernelGGL(k_bshuf_lz4_decode<4>, grid, dim3(64), 0, st, da);
    }
    if (e == hipSuccess && with_decode) e = hipGetLastError();
    if (e == hipSuccess && done) e = hipEventRecord(done, st);
    return e == hipSuccess ? FFS_OK : refuse(err, FFS_ERR_DEVICE, std::string("decode launch: ") + hipGetErrorString(e));
}

static bool codec_known(ffs_ctx* c, int codec, const char* who) {
    if (codec == FFS_CODEC_BSLZ4 || codec == FFS_CODEC_BYTE_OFFSET || codec == FFS_CODEC_JUNGFRAU_RAW) return true;
    c->err = std::string(who) + ": unknown codec " + std::to_string(codec);
    return false;
}

static int ffs_submit_encoded_impl(ffs_stream* s, int codec, const void* const* chunks, const size_t* chunk_bytes, uint32_t n_frames, int64_t first_frame_id) {
    if (!s || !chunks || !chunk_bytes) return FFS_ERR_INVALID;
    ffs_ctx* c = s->ctx;
    if (s->busy) return refuse(c->err, FFS_ERR_INVALID, "stream already has a batch in flight: call ffs_wait() first");
    if (n_frames == 0 || n_frames > s->max_batch) return refuse(c->err, FFS_ERR_INVALID, "n_frames must be in 1..max_batch");
    if (!codec_known(c, codec, "ffs_submit_encoded")) return FFS_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    s->radial_todo = true;
    s->stats_todo = true;
    s->dev_input = false;
    HIP_TRY(c, hipEventRecord(s->ev[0], s->st_up));
    EncodedBatch b;
    FFS_TRY(prepare(s, codec, chunks, chunk_bytes, n_frames, b));
    // The rest -- block index, table copy, decode kernel and the hot path's launches -- is enqueued by a
    // helper thread, so that the caller gets its thread back while the index is built; ffs_wait joins it.
    s->first_id = first_frame_id;
    s->reruns = 0;
    // (s->n_frames stays the PREVIOUS batch's until enqueue_batch has planned this one: plan_batch reads that batch's counts with it)
    mark_busy(s);
    s->job_rc = FFS_OK;
    s->job_err.clear();
    const ParamSnapshot snap = snapshot_of(c->settings);
    s->job = std::thread([s, c, snap, n_frames, b = std::move(b)]() {
        if (hipSetDevice(c->device) != hipSuccess) {
            s->job_rc = refuse(s->job_err, FFS_ERR_DEVICE, "hipSetDevice failed on the stream's helper thread");
            return;
        }
        // the decode kernel runs with the dense kernels (in their order), behind the copies of its input
        hipStream_t dst = c->tune.decode_in_dense_stream ? s->st : s->st_up;
        int r = launch(s, b, dst, true, true, dst != s->st_up ? s->ev[6] : nullptr, s->ev[1], s->job_err);
        if (r == FFS_OK) {
            r = enqueue_batch(s, s->d_img, c->L.pitch, c->L.frame_stride, n_frames, &snap);
            if (r != FFS_OK) s->job_err = c->err;
        }
        s->job_rc = r;
        if (r == FFS_OK) ahead_register(s);
    });
    return FFS_OK;
}

extern "C" int ffs_decode_only_encoded(ffs_stream* s, int codec, const void* const* chunks, const size_t* chunk_bytes, uint32_t n_frames,
                                       uint32_t iters, float* ms_decode, void* host_out) {
    if (!s || !chunks || !chunk_bytes || iters == 0) return FFS_ERR_INVALID;
    ffs_ctx* c = s->ctx;
    if (s->busy || n_frames == 0 || n_frames > s->max_batch) return refuse(c->err, FFS_ERR_INVALID, "ffs_decode_only: stream busy or n_frames out of range");
    if (!codec_known(c, codec, "ffs_decode_only_encoded")) return FFS_ERR_INVALID;
    const Layout& L = c->L;
    HIP_TRY(c, hipSetDevice(c->device));
    s->waited_ok = false;   // (the decoded frames replace the last batch's in the stream's image buffer: ffs_stream_spot_backgrounds has nothing to read)
    EncodedBatch b;
    std::string err;
    int rc = prepare(s, codec, chunks, chunk_bytes, n_frames, b);
    if (rc == FFS_OK && (rc = launch(s, b, s->st_up, true, false, nullptr, nullptr, err)) != FFS_OK) c->err = err;
    if (rc != FFS_OK) {
        (void)hipStreamSynchronize(s->st_up);
        return rc;
    }
    HIP_TRY(c, hipEventRecord(s->ev[0], s->st_up));
    for (uint32_t i = 0; i < iters; ++i)
        if ((rc = launch(s, b, s->st_up, false, true, nullptr, nullptr, err)) != FFS_OK) return refuse(c->err, rc, err);
    HIP_TRY(c, hipEventRecord(s->ev[1], s->st_up));
    uint32_t flag = 0;
    HIP_TRY(c, hipMemcpyAsync(&flag, s->d_overflow, 4, hipMemcpyDeviceToHost, s->st_up));
    HIP_TRY(c, hipStreamSynchronize(s->st_up));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    if (ms_decode) *ms_decode = ms / iters;
    if (host_out) {
        const size_t row = (size_t)L.W * c->settings.pixel_bytes;
        HIP_TRY(c, hipMemcpy2D(host_out, row, s->d_img, L.pitch, row, (size_t)L.H * n_frames, hipMemcpyDeviceToHost));
    }
    if (const char* text = encoded_corruption(flag)) {
        HIP_TRY(c, hipMemset(s->d_overflow, 0, 4));
        return refuse(c->err, FFS_ERR_INVALID, text);
    }
    return FFS_OK;
}
extern "C" int ffs_decode_only(ffs_stream* s, const void* const* chunks, const size_t* chunk_bytes, uint32_t n_frames, uint32_t iters, float* ms_decode, void* host_out) {
    return ffs_decode_only_encoded(s, FFS_CODEC_BSLZ4, chunks, chunk_bytes, n_frames, iters, ms_decode, host_out);
}

extern "C" int ffs_submit_compressed(ffs_stream* s, const void* const* chunks, const size_t* chunk_bytes, uint32_t n_frames, int64_t first_frame_id) {
    if (!s || !stream_handle_ok(s)) return FFS_ERR_INVALID;
    return guarded(s->ctx, [&] { return ffs_submit_encoded_impl(s, FFS_CODEC_BSLZ4, chunks, chunk_bytes, n_frames, first_frame_id); });
}
extern "C" int ffs_submit_encoded(ffs_stream* s, int codec, const void* const* chunks, const size_t* chunk_bytes, uint32_t n_frames, int64_t first_frame_id) {
    if (!s || !stream_handle_ok(s)) return FFS_ERR_INVALID;
    return guarded(s->ctx, [&] { return ffs_submit_encoded_impl(s, codec, chunks, chunk_bytes, n_frames, first_frame_id); });
}

// ---- Jungfrau pedestals: dark frames folded into the context's accumulators (kernels_jfped.hpp) ------------------------
// The accumulators are one allocation of nine dense planes: count[3] (uint32), then sum[3], then sum_sq[3] (uint64), jfped_stride entries each.
static size_t jfped_bytes(size_t stride) { return stride * 3 * (sizeof(uint32_t) + 2 * sizeof(uint64_t)); }
static uint32_t* jfped_count(const ffs_ctx* c) { return reinterpret_cast<uint32_t*>(c->d_jfped); }
static uint64_t* jfped_sum(const ffs_ctx* c) { return reinterpret_cast<uint64_t*>(c->d_jfped + c->jfped_stride * 3 * sizeof(uint32_t)); }
static uint64_t* jfped_sum_sq(const ffs_ctx* c) { return jfped_sum(c) + c->jfped_stride * 3; }

void jfped_free_stream(ffs_stream* s) {
    for (hipEvent_t& e : s->jfped_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}
void jfped_free_ctx(ffs_ctx* c) {
    if (c->jfped_st) {
        (void)hipStreamSynchronize(c->jfped_st);
        (void)hipStreamDestroy(c->jfped_st);
        c->jfped_st = nullptr;
    }
    if (c->d_jfped) (void)hipFree(c->d_jfped);
    c->d_jfped = nullptr;
}

static int jfped_begin_impl(ffs_ctx* c) {
    if (c->settings.pixel_bytes != 4)
        return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_jungfrau_pedestal_begin: raw Jungfrau words belong to contexts of 32-bit photon counts: the context must have pixel_bytes 4");
    if (c->inflight.load() > 0)
        return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_jungfrau_pedestal_begin: a batch or a fold of this context is in flight (wait for it first): a begin zeroes the accumulators");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->jfped_st) HIP_TRY(c, hipStreamCreateWithFlags(&c->jfped_st, hipStreamNonBlocking));
    if (!c->d_jfped) {
        const size_t stride = ((size_t)c->L.W * c->L.H + kJfPedLanePixels - 1) / kJfPedLanePixels * kJfPedLanePixels;
        uint8_t* d = nullptr;
        if (dmalloc(&d, jfped_bytes(stride)) != hipSuccess) {
            (void)hipGetLastError();
            return refuse(c->err, FFS_ERR_NOMEM, "ffs_ctx_jungfrau_pedestal_begin: hipMalloc(accumulators, " + std::to_string(jfped_bytes(stride) >> 20) + " MB) failed");
        }
        c->d_jfped = d;
        c->jfped_stride = stride;
    }
    HIP_TRY(c, hipMemsetAsync(c->d_jfped, 0, jfped_bytes(c->jfped_stride), c->jfped_st));
    HIP_TRY(c, hipStreamSynchronize(c->jfped_st));
    std::lock_guard<std::mutex> lock(c->jfped_mu);
    c->jfped_frames = 0;
    return FFS_OK;
}
extern "C" int ffs_ctx_jungfrau_pedestal_begin(ffs_ctx* c) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return jfped_begin_impl(c); });
}

extern "C" int ffs_ctx_jungfrau_pedestal_end(ffs_ctx* c) {
    if (!c) return FFS_ERR_INVALID;
    if (!c->d_jfped) return FFS_OK;
    if (c->inflight.load() > 0)
        return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_jungfrau_pedestal_end: a batch or a fold of this context is in flight (wait for it first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->jfped_st));
    (void)hipFree(c->d_jfped);
    c->d_jfped = nullptr;
    return FFS_OK;
}

// A fold counts among the context's batches in flight from its first device call to its return -- begin, get, end and a calibration change see
// it there -- on every way out.  The stream itself is not marked busy: the fold is synchronous on the thread that drives the stream, and its
// host buffer may still grow for the chunks (ensure_host_staging).
namespace {
struct FoldInFlight {
    ffs_ctx* c;
    explicit FoldInFlight(ffs_ctx* c_) : c(c_) { ++c->inflight; }
    ~FoldInFlight() { --c->inflight; }
};
}  // namespace

static int jfped_fold_impl(ffs_stream* s, const void* const* chunks, const size_t* chunk_bytes, uint32_t n, float* ms_fold) {
    static const char* const who = "ffs_stream_jungfrau_pedestal_fold";
    ffs_ctx* c = s->ctx;
    if (!chunks || !chunk_bytes) return refuse(c->err, FFS_ERR_INVALID, std::string(who) + ": chunks or chunk_bytes is NULL");
    if (!c->d_jfped)
        return refuse(c->err, FFS_ERR_INVALID, std::string(who) + ": the context has no accumulators (ffs_ctx_jungfrau_pedestal_begin first; ffs_ctx_jungfrau_pedestal_end frees them)");
    if (s->busy) return refuse(c->err, FFS_ERR_INVALID, std::string(who) + ": the stream has a batch in flight: call ffs_wait() first");
    if (n == 0 || n > s->max_batch) return refuse(c->err, FFS_ERR_INVALID, std::string(who) + ": n_frames must be in 1..max_batch (" + std::to_string(s->max_batch) + "), got " + std::to_string(n));
    const size_t frame_bytes = (size_t)c->L.W * c->L.H * 2;
    for (uint32_t f = 0; f < n; ++f)
        if (!chunks[f] || chunk_bytes[f] != frame_bytes)
            return refuse(c->err, FFS_ERR_INVALID, std::string(who) + ": chunk " + std::to_string(f) + (chunks[f] ? " of " + std::to_string(chunk_bytes[f]) + " bytes" : std::string(" (NULL)"))
                                                       + " is not a dark frame of " + std::to_string((size_t)c->L.W * c->L.H) + " 16-bit words (" + std::to_string(frame_bytes) + " bytes)");
    auto too_many = [&] {
        return refuse(c->err, FFS_ERR_INVALID, std::string(who) + ": " + std::to_string(n) + " more frames would take n_frames past 2^32 - 1 (the counts are 32 bits)");
    };
    {
        std::lock_guard<std::mutex> lock(c->jfped_mu);
        if (!jf_pedestal_frames_fit(c->jfped_frames, n)) return too_many();
    }
    HIP_TRY(c, hipSetDevice(c->device));
    for (hipEvent_t& e : s->jfped_ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    FoldInFlight in_flight(c);
    EncodedBatch b;
    FFS_TRY(prepare(s, FFS_CODEC_JUNGFRAU_RAW, chunks, chunk_bytes, n, b, who));
    // from here on the chunks' copy reads memory the caller gets back: every way out waits for it
    const uint32_t n_px = (uint32_t)c->L.W * (uint32_t)c->L.H, groups = (n_px + kJfPedLanePixels - 1) / kJfPedLanePixels;
    const dim3 grid((groups + kJfPedBlock - 1) / kJfPedBlock);
    hipError_t e = hipSuccess;
    bool fits = true;
    {
        std::lock_guard<std::mutex> lock(c->jfped_mu);
        fits = jf_pedestal_frames_fit(c->jfped_frames, n);   // (another stream's fold may have come in between)
        if (fits) e = hipStreamWaitEvent(c->jfped_st, s->ev[6], 0);
        for (uint32_t f0 = 0; fits && e == hipSuccess && f0 < n; f0 += kJfPedMaxLaunch) {
            JfPedArgs a{.comp = s->enc.d_comp, .count = jfped_count(c), .sum = jfped_sum(c), .sum_sq = jfped_sum_sq(c), .plane_stride = c->jfped_stride,
                        .n_px = n_px, .n_frames = std::min(n - f0, kJfPedMaxLaunch), .base = {}};
            for (uint32_t f = 0; f < a.n_frames; ++f) a.base[f] = (uint32_t)b.base[f0 + f];
            const bool first = f0 == 0, last = n - f0 <= kJfPedMaxLaunch;
            hipExtLaunchKernelGGL(k_jungfrau_pedestal_fold, grid, dim3(kJfPedBlock), 0, c->jfped_st, first ? s->jfped_ev[0] : nullptr, last ? s->jfped_ev[1] : nullptr, 0, a);
            e = hipGetLastError();
        }
        // (a launch that failed half way through a long batch leaves the accumulators undefined, like a failed ffs_wait the pixel statistics)
        if (fits && e == hipSuccess) c->jfped_frames += n;
    }
    if (!fits || e != hipSuccess) {
        (void)hipStreamSynchronize(s->st_up);
        (void)hipStreamSynchronize(c->jfped_st);
        if (!fits) return too_many();
        return refuse(c->err, FFS_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    HIP_TRY(c, hipEventSynchronize(s->jfped_ev[1]));   // (the launch waited for the chunks: the host buffer is free as well)
    if (ms_fold) HIP_TRY(c, hipEventElapsedTime(ms_fold, s->jfped_ev[0], s->jfped_ev[1]));
    return FFS_OK;
}
extern "C" int ffs_stream_jungfrau_pedestal_fold(ffs_stream* s, const void* const* chunks, const size_t* chunk_bytes, uint32_t n_frames, float* ms_fold) {
    if (!s || !stream_handle_ok(s)) return FFS_ERR_INVALID;
    return guarded(s->ctx, [&] { return jfped_fold_impl(s, chunks, chunk_bytes, n_frames, ms_fold); });
}

// Everything is checked before anything is copied; the planes are dense on the device as the caller reads them: nine plain copies.
static int jfped_get_impl(ffs_ctx* c, ffs_jungfrau_pedestal_stats* out) {
    if (!c->d_jfped)
        return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_get_jungfrau_pedestal: the context has no accumulators (ffs_ctx_jungfrau_pedestal_begin first; ffs_ctx_jungfrau_pedestal_end frees them)");
    if (c->inflight.load() > 0)
        return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_get_jungfrau_pedestal: a batch or a fold of this context is in flight (wait for it first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->jfped_st));
    const size_t n = (size_t)c->L.W * c->L.H, stride = c->jfped_stride;
    for (size_t st = 0; st < 3; ++st) {
        if (out->count[st]) HIP_TRY(c, hipMemcpy(out->count[st], jfped_count(c) + st * stride, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (out->sum[st]) HIP_TRY(c, hipMemcpy(out->sum[st], jfped_sum(c) + st * stride, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out->sum_sq[st]) HIP_TRY(c, hipMemcpy(out->sum_sq[st], jfped_sum_sq(c) + st * stride, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    std::lock_guard<std::mutex> lock(c->jfped_mu);
    out->n_frames = c->jfped_frames;
    return FFS_OK;
}
extern "C" int ffs_ctx_get_jungfrau_pedestal(ffs_ctx* c, ffs_jungfrau_pedestal_stats* out) {
    if (!c) return FFS_ERR_INVALID;
    if (!out) return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_get_jungfrau_pedestal: out is NULL");
    return guarded(c, [&] { return jfped_get_impl(c, out); });
}

// The planes rule on the host (jungfrau_pedestal_model.hpp): no context, no GPU; its texts go where ffs_last_error(NULL) reads them
extern "C" int ffs_jungfrau_pedestal_planes(const ffs_jungfrau_pedestal_stats* stats, size_t n_px, uint32_t min_frames, float max_rms, float* const pedestal[3],
                                            float* const rms[3], uint8_t* const ok[3]) {
    static const char* const who = "ffs_jungfrau_pedestal_planes: ";
    if (!stats || !pedestal || !rms || !ok) return refuse(g_create_error, FFS_ERR_INVALID, std::string(who) + "stats, pedestal, rms or ok is NULL");
    for (int st = 0; st < 3; ++st)
        if (!stats->count[st] || !stats->sum[st] || !stats->sum_sq[st])
            return refuse(g_create_error, FFS_ERR_INVALID, std::string(who) + "a count, sum or sum_sq plane of stage " + std::to_string(st) + " is NULL");
    if (min_frames == 0) return refuse(g_create_error, FFS_ERR_INVALID, std::string(who) + "min_frames must be at least 1");
    if (!jf_pedestal_args_ok(min_frames, max_rms))
        return refuse(g_create_error, FFS_ERR_INVALID, std::string(who) + "max_rms must be finite and >= 0 (0: no noise test), got " + std::to_string(max_rms));
    for (int st = 0; st < 3; ++st)
        jf_pedestal_plane(stats->count[st], stats->sum[st], stats->sum_sq[st], n_px, min_frames, max_rms, pedestal[st], rms[st], ok[st]);
    return FFS_OK;
}
