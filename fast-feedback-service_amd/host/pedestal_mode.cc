// pedestal_mode.cc -- spotfinder --jungfrau-pedestal (pedestal_mode.hpp).  One context.  On the GPU every worker thread has an ffs_stream of
// its own: it reads a batch of frames straight into the stream's pinned buffer, at slots that are multiples of 64 bytes, and folds them; the
// library keeps the threads' launches on the accumulators apart.  With --cpu-decode the threads read a batch's frames side by side and then
// each folds ITS slice of the pixels over all of them, so no two threads touch one accumulator entry.  Integers throughout: the files are the
// same, byte for byte, either way and with any number of threads.
#include "pedestal_mode.hpp"

#include <atomic>
#include <barrier>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <thread>

#include "codecs.hpp"
#include "ffs_hip.h"

namespace ffshost {

namespace {

struct Source {
    Reader& reader;
    size_t frame_bytes;
    float timeout;
    std::mutex mu;   // around every call of a reader that is not reentrant (spotfinder.cc:763-765)
    std::atomic<bool> failed{false};

    // frame `index` into dst; false (and `failed`): it did not appear in time, or came short
    bool read(size_t index, uint8_t* dst) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            {
                std::unique_lock<std::mutex> lock(mu, std::defer_lock);
                if (!reader.reentrant()) lock.lock();
                if (reader.is_image_available(index)) {
                    if (reader.get_raw_chunk(index, {dst, frame_bytes}).size() == frame_bytes) return true;
                    std::printf("Error: image %zu is not a frame of %zu bytes of raw Jungfrau words\n", index, frame_bytes);
                    failed = true;
                    return false;
                }
            }
            if (failed.load()) return false;
            if (std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count() > timeout) {
                std::printf("Error: timed out waiting for image %zu\n", index);
                failed = true;
                return false;
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
    }
};

bool write_file(const std::string& name, const void* data, size_t bytes) {
    std::ofstream f(name, std::ios::binary | std::ios::trunc);
    if (f && f.write(static_cast<const char*>(data), (std::streamsize)bytes) && f.flush()) return true;
    std::printf("Error: --jungfrau-pedestal: cannot write %s\n", name.c_str());
    return false;
}

}  // namespace

int run_jungfrau_pedestal(const Args& args, Reader& reader, const std::vector<float>& old_calibration) {
    if (reader.get_raw_chunk_compression() != Reader::NONE || reader.get_element_size() != 2)
        arg_error("--jungfrau-pedestal: dark frames of raw Jungfrau words are uncompressed 16-bit frames; this frame source hands over "
                  + std::string(reader.get_raw_chunk_compression() == Reader::NONE ? "uncompressed" : "compressed") + " frames of "
                  + std::to_string(reader.get_element_size() * 8) + " bits");
    const uint32_t width = (uint32_t)reader.image_shape()[1], height = (uint32_t)reader.image_shape()[0];
    const size_t n_px = (size_t)width * height, frame_bytes = n_px * 2;
    const uint32_t num_images = args.images_set ? args.images : (uint32_t)reader.get_number_of_images();
    const uint32_t batch = std::max<uint32_t>(1, std::min<uint32_t>(args.batch ? args.batch : 8, std::max<uint32_t>(1, num_images)));
    const uint32_t n_batches = (num_images + batch - 1) / batch;
    const uint32_t threads = std::max<uint32_t>(1, args.threads);
    const bool on_gpu = !args.cpu_decode;
    std::printf("Image:       %4u x %4u = %zu px\n", width, height, n_px);
    std::printf("Dark run:    %u frames of raw Jungfrau words, folded %s, %u frames per fold, %u threads\n", num_images, on_gpu ? "on the GPU" : "on the worker threads", batch, threads);
    Source source{reader, frame_bytes, args.timeout};
    std::vector<uint32_t> count(3 * n_px, 0u);
    std::vector<uint64_t> sum(3 * n_px, 0ull), sum_sq(3 * n_px, 0ull);
    uint64_t frames = 0;
    const auto t_start = std::chrono::steady_clock::now();

    if (on_gpu) {
        ffs_ctx* ctx = nullptr;
        if (ffs_ctx_create(args.devices.empty() ? args.device : args.devices[0], width, height, 4, batch, 0, &ctx) != FFS_OK) {
            std::printf("Error: %s\n", ffs_last_error(nullptr));
            return 1;
        }
        if (ffs_ctx_jungfrau_pedestal_begin(ctx) != FFS_OK) {
            std::printf("Error: %s\n", ffs_last_error(ctx));
            return 1;
        }
        const size_t slot = (frame_bytes + 63) / 64 * 64;
        // (a worker owns a stream and with it device and pinned memory for a batch: at most eight, as when the GPU decodes data)
        const uint32_t workers = std::min({threads, 8u, n_batches ? n_batches : 1u});
        std::atomic<uint32_t> next{0};
        std::mutex print_mu;
        auto work = [&] {
            ffs_stream* s = nullptr;
            void* v = nullptr;
            size_t host_bytes = 0;
            if (ffs_stream_create(ctx, &s) != FFS_OK || ffs_stream_reserve_host(s, (size_t)batch * slot) != FFS_OK || ffs_stream_host_buffer(s, &v, &host_bytes) != FFS_OK
                || host_bytes < (size_t)batch * slot) {
                std::lock_guard<std::mutex> lock(print_mu);
                std::printf("Error: %s\n", ffs_last_error(ctx));
                source.failed = true;
                return;
            }
            uint8_t* host = static_cast<uint8_t*>(v);
            std::vector<const void*> chunks(batch);
            std::vector<size_t> sizes(batch, frame_bytes);
            for (uint32_t b = next++; b < n_batches && !source.failed.load(); b = next++) {
                const uint32_t first = b * batch, n = std::min(batch, num_images - first);
                for (uint32_t k = 0; k < n; ++k) {
                    if (!source.read(first + k, host + (size_t)k * slot)) return;
                    chunks[k] = host + (size_t)k * slot;
                }
                if (ffs_stream_jungfrau_pedestal_fold(s, chunks.data(), sizes.data(), n, nullptr) != FFS_OK) {
                    std::lock_guard<std::mutex> lock(print_mu);
                    std::printf("Error: %s\n", ffs_last_error(ctx));
                    source.failed = true;
                    return;
                }
            }
        };
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < workers; ++t) pool.emplace_back(work);
        work();
        for (std::thread& t : pool) t.join();
        if (source.failed.load()) return 1;
        ffs_jungfrau_pedestal_stats st{};
        for (size_t s = 0; s < 3; ++s) {
            st.count[s] = count.data() + s * n_px;
            st.sum[s] = sum.data() + s * n_px;
            st.sum_sq[s] = sum_sq.data() + s * n_px;
        }
        if (ffs_ctx_get_jungfrau_pedestal(ctx, &st) != FFS_OK || ffs_ctx_jungfrau_pedestal_end(ctx) != FFS_OK) {
            std::printf("Error: %s\n", ffs_last_error(ctx));
            return 1;
        }
        frames = st.n_frames;
        ffs_ctx_destroy(ctx);
    } else {
        std::vector<uint8_t> staged((size_t)batch * frame_bytes);
        std::barrier sync((std::ptrdiff_t)threads);
        auto work = [&](uint32_t t) {
            const size_t lo = n_px * t / threads, hi = n_px * (t + 1) / threads;
            for (uint32_t b = 0; b < n_batches; ++b) {
                const uint32_t first = b * batch, n = std::min(batch, num_images - first);
                for (uint32_t k = t; k < n; k += threads) (void)source.read(first + k, staged.data() + (size_t)k * frame_bytes);
                sync.arrive_and_wait();   // the batch's frames are read (or the run has failed: every thread sees that here)
                if (source.failed.load()) return;
                // (a tile of pixels over all frames of the batch, then the next: the tile's 60 B a pixel of accumulators stay in the cache)
                constexpr size_t kTile = 4096;
                for (size_t a = lo; a < hi; a += kTile)
                    for (uint32_t k = 0; k < n; ++k)
                        jungfrau_pedestal_fold_slice(reinterpret_cast<const uint16_t*>(staged.data() + (size_t)k * frame_bytes), n_px, a, std::min(hi, a + kTile), count.data(),
                                                     sum.data(), sum_sq.data());
                sync.arrive_and_wait();   // ... and folded: the staging area is free
            }
        };
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work, t);
        work(0);
        for (std::thread& t : pool) t.join();
        if (source.failed.load()) return 1;
        frames = num_images;
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();

    std::vector<float> pedestal(3 * n_px), rms(3 * n_px);
    std::vector<uint8_t> ok(3 * n_px);
    jungfrau_pedestal_planes(count.data(), sum.data(), sum_sq.data(), n_px, args.pedestal_min_frames, args.pedestal_max_rms, pedestal.data(), rms.data(), ok.data());
    const std::string& prefix = args.jungfrau_pedestal;
    if (!write_file(prefix + ".count.u32", count.data(), count.size() * 4) || !write_file(prefix + ".sum.u64", sum.data(), sum.size() * 8)
        || !write_file(prefix + ".sum_sq.u64", sum_sq.data(), sum_sq.size() * 8) || !write_file(prefix + ".pedestal.f32", pedestal.data(), pedestal.size() * 4)
        || !write_file(prefix + ".rms.f32", rms.data(), rms.size() * 4) || !write_file(prefix + ".ok.u8", ok.data(), ok.size()))
        return 1;
    if (!old_calibration.empty()) {
        std::vector<float> out(6 * n_px);
        jungfrau_repedestal(old_calibration.data(), n_px, pedestal.data(), ok.data(), out.data());
        if (!write_file(prefix + ".calibration.f32", out.data(), out.size() * 4)) return 1;
    }
    uint64_t words[3] = {0, 0, 0}, usable[3] = {0, 0, 0};
    for (size_t s = 0; s < 3; ++s)
        for (size_t k = 0; k < n_px; ++k) {
            words[s] += count[s * n_px + k];
            usable[s] += ok[s * n_px + k];
        }
    const uint64_t invalid = frames * n_px - words[0] - words[1] - words[2];
    std::printf("Jungfrau pedestals: %llu frames, words counted G0 %llu G1 %llu G2 %llu, invalid words %llu; usable pixels G0 %llu G1 %llu G2 %llu of %zu "
                "(min frames %u, max rms %g); %.1f frames/s -> %s.{count.u32,sum.u64,sum_sq.u64,pedestal.f32,rms.f32,ok.u8%s}\n",
                (unsigned long long)frames, (unsigned long long)words[0], (unsigned long long)words[1], (unsigned long long)words[2], (unsigned long long)invalid,
                (unsigned long long)usable[0], (unsigned long long)usable[1], (unsigned long long)usable[2], n_px, args.pedestal_min_frames, (double)args.pedestal_max_rms,
                seconds > 0 ? frames / seconds : 0.0, prefix.c_str(), old_calibration.empty() ? "" : ",calibration.f32");
    return 0;
}

}  // namespace ffshost
