// spotfinder.cc -- the `spotfinder` driver for libffs_hip.so: same command line, stdout phrases,
// --pipe_fd JSON lines, output files and exit codes as the reference's spotfinder/spotfinder.cc
// (flags :291-398, JSON :997-1008, per-image lines :1055-1087, 3D stage :1101-1148, summary
// :1308-1329), rebuilt around batches that all reader threads of a GPU fill together
// (batch_pipeline.hpp).  This file: set-up, what is done with a collected batch, the stages after
// the run.  All device work goes through include/ffs_hip.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <map>
#include <condition_variable>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <sys/resource.h>
#include <sched.h>
#include <unistd.h>
#include <vector>

#include "batch_pipeline.hpp"
#include "cli_args.hpp"
#include "ffs_hip.h"
#include "minijson.hpp"
#include "pedestal_mode.hpp"
#include "radial_bins.hpp"
#include "kabsch_space.hpp"
#include "png_writer.hpp"
#include "reader.hpp"
#include "shoebox_geometry.hpp"
#include "predict_geometry.hpp"
#include "index_basis.hpp"
#include "index_assign.hpp"
#include "../csrc/predict_plan.hpp"
#include "../csrc/shoebox_model.hpp"
#include "../csrc/sweep_plan.hpp"

using namespace ffshost;
using namespace std::chrono_literals;
namespace fs = std::filesystem;

static std::atomic<bool> g_stop{false};
extern "C" void stop_processing(int) {  // spotfinder.cc:43-54
    if (g_stop.load()) std::_Exit(1);
    static const char msg[] = "Running interrupted by user request\n";
    (void)!write(STDOUT_FILENO, msg, sizeof msg - 1);
    g_stop.store(true);
}

struct DetectorGeometry {  // spotfinder/kernels/masking.cuh:16-80
    float pixel_size_x = 0, pixel_size_y = 0, beam_center_x = 0, beam_center_y = 0, distance = 0;
};

static DetectorGeometry detector_from_json(const std::string& text) {
    const JsonValue j = JsonParser(text).parse();
    for (const char* k : {"pixel_size_x", "pixel_size_y", "beam_center_x", "beam_center_y", "distance"})
        (void)j.at(k);  // throws "Key ... is missing from the input JSON"
    DetectorGeometry d;
    d.pixel_size_x = (float)j.at("pixel_size_x").number() / 1000.0f;  // mm -> m
    d.pixel_size_y = (float)j.at("pixel_size_y").number() / 1000.0f;
    d.beam_center_x = (float)j.at("beam_center_x").number() / (d.pixel_size_x * 1000);  // mm -> px
    d.beam_center_y = (float)j.at("beam_center_y").number() / (d.pixel_size_y * 1000);
    d.distance = (float)j.at("distance").number() / 1000.0f;
    return d;
}

// thread-safe writer of JSON lines to the inherited pipe (PipeHandler, spotfinder.cc:208-255)
class PipeHandler {
    int fd_;
    std::mutex m_;
  public:
    explicit PipeHandler(int fd) : fd_(fd) { std::printf("PipeHandler initialized with pipe_fd: %d\n", fd); }
    ~PipeHandler() { close(fd_); }
    void send(const std::string& line) { send_lines(line + "\n"); }
    // whole lines, each ending in a newline: one write for a batch's worth (a write per line was 7 000 system calls a second on
    // the one thread that also frees the GPU's staging areas)
    void send_lines(const std::string& s) {
        std::lock_guard<std::mutex> lock(m_);
        size_t at = 0;
        while (at < s.size()) {
            const ssize_t w = write(fd_, s.c_str() + at, s.size() - at);
            if (w == -1) { if (errno == EINTR) continue; std::cerr << "Error writing to pipe: " << std::strerror(errno) << std::endl; return; }
            at += (size_t)w;
        }
    }
};

template <typename T>
static std::string fmt_num(T v) { std::ostringstream o; o << v; return o.str(); }  // iostream default, :1138-1147

#define FFS_CHECK(ctx, expr)                                                       \
    do {                                                                           \
        if ((expr) != FFS_OK) {                                                    \
            std::printf("Error: %s\n", ffs_last_error(ctx));                       \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

using Clock = std::chrono::steady_clock;
static double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// -v: where the process's wall time goes outside the timed loop (the service starts one process per request, service.py:497,
// so start-up and tear-down are what a short request sees): "[+ ms since main] step (ms it took)"
class Stamps {
    const Clock::time_point process_start_;
    Clock::time_point prev_;
  public:
    bool verbose = false;
    explicit Stamps(Clock::time_point process_start) : process_start_(process_start), prev_(process_start) {}
    Clock::time_point process_start() const { return process_start_; }
    void operator()(const char* what) {
        if (!verbose) return;
        const auto t = Clock::now();
        std::printf("[%7.1f ms] %s (%.1f ms)\n", ms_between(process_start_, t), what, ms_between(prev_, t));
        prev_ = t;
    }
};

struct JoinedThread {   // (an early `return` must not meet a joinable std::thread)
    std::thread th;
    ~JoinedThread() { if (th.joinable()) th.join(); }
};

struct FrameShape {
    uint32_t width = 0, height = 0;
    size_t bytes_per_pixel = 2;
    size_t pixels() const { return (size_t)width * height; }
    size_t frame_bytes() const { return pixels() * bytes_per_pixel; }
};

// ---- set-up steps -------------------------------------------------------------------------------------------------------------

// wait_for_ready_for_read, :137-175 (give_up: no GPU after all -- stop waiting for files and say nothing more)
template <typename Checker>
static void wait_ready(const std::string& path, Checker checker, float timeout, const std::atomic<bool>& give_up) {
    const auto t0 = Clock::now();
    bool waited = false;
    while (!checker(path)) {
        if (give_up.load()) return;
        const double w = std::chrono::duration<double>(Clock::now() - t0).count();
        std::printf("\rWaiting for \033[1;35m%s\033[0m to be ready for read [%4.1f s] ", path.c_str(), w);
        std::fflush(stdout);
        waited = true;
        if (w > timeout) {
            std::printf("\nError: Waited too long for read availability\n");
            std::exit(1);
        }
        std::this_thread::sleep_for(80ms);
    }
    if (waited) std::printf("\n");
}

// choose the reader (spotfinder.cc:438-466).  -> 0, or the process's exit code
static int open_reader(const Args& args, const std::atomic<bool>& give_up, std::unique_ptr<Reader>& out) {
    const std::string& file = args.file;
    try {
        if (args.sample || file.rfind("synth:", 0) == 0) {
            out = make_synth_reader(args.sample ? "synth:eiger16m:6" : file);
        } else {
            if (!fs::exists(file) && file.find('#') == std::string::npos)
                wait_ready(file, [](const std::string& s) { return fs::exists(s); }, args.timeout, give_up);
            if (fs::is_directory(file)) {
                wait_ready(file, is_ready_for_read<SHMRead>, args.timeout, give_up);
                out = make_shm_reader(file);
            } else if (file.size() > 4 && file.compare(file.size() - 4, 4, ".cbf") == 0) {
                if (!args.images_set) {
                    std::printf("Error: CBF reading must specify --images\n");
                    return 1;
                }
                out = make_cbf_reader(file, args.images, args.start_index);
            } else {
                wait_ready(file, is_ready_for_read<H5Read>, args.timeout, give_up);
                out = make_h5_reader(file);
            }
        }
    } catch (const std::exception& e) {
        if (!give_up.load()) std::printf("Error: %s\n", e.what());
        return 1;
    }
    return 0;
}

// The frame source is opened (header, the 72 MB pixel mask of an Eiger-16M stream directory: 35 ms) on a helper thread WHILE this
// one initialises the HIP runtime (70-160 ms): nothing in it needs the GPU, and a request's latency is the wall time of the process
// (DESIGN.md section 5b).  It prints only when it has to wait for its files or fails.  -> 0, or the process's exit code
// --gain-map FILE: exactly width x height float32 values, little-endian (the byte order of every host this driver is built for), row-major;
// every value inside what ffs_ctx_set_gain_map accepts.  Anything else is a usage error.  Empty: no map was asked for.
static std::vector<float> read_gain_map(const Args& args, uint32_t width, uint32_t height) {
    std::vector<float> map;
    if (args.gain_map.empty()) return map;
    const size_t n = (size_t)width * height;
    std::ifstream f(args.gain_map, std::ios::binary | std::ios::ate);
    if (!f) arg_error("--gain-map: cannot open " + args.gain_map);
    const std::streamoff bytes = f.tellg();
    if (bytes < 0 || (uint64_t)bytes != (uint64_t)n * sizeof(float))
        arg_error("--gain-map: " + args.gain_map + " holds " + std::to_string((long long)bytes) + " bytes, the " + std::to_string(width) + " x "
                  + std::to_string(height) + " float32 values of this detector are " + std::to_string(n * sizeof(float)));
    map.resize(n);
    f.seekg(0);
    if (!f.read(reinterpret_cast<char*>(map.data()), bytes)) arg_error("--gain-map: cannot read " + args.gain_map);
    for (size_t i = 0; i < n; ++i)
        if (!(map[i] >= 0x1p-60f && map[i] <= 0x1p60f))   // (false for a NaN)
            arg_error("--gain-map: value " + std::to_string(i) + " of " + args.gain_map + " is " + std::to_string(map[i])
                      + ": every value must be finite and in [2^-60, 2^60]");
    return map;
}

// --jungfrau-calibration FILE: exactly 6 x width x height float32 values, little-endian, row-major -- pedestal G0, G1, G2, then factor G0, G1,
// G2 -- for a source of uncompressed 16-bit frames.  The ranges are the library's to check (ffs_ctx_set_jungfrau_calibration names plane and
// entry).  Anything else is a usage error.  Empty: the flag was not given.
static std::vector<float> read_jungfrau_calibration(const Args& args, Reader& reader) {
    std::vector<float> planes;
    if (args.jungfrau_calibration.empty()) return planes;
    const std::string& file = args.jungfrau_calibration;
    if (reader.get_raw_chunk_compression() != Reader::NONE || reader.get_element_size() != 2)
        arg_error("--jungfrau-calibration: raw Jungfrau words are uncompressed 16-bit frames; this frame source hands over "
                  + std::string(reader.get_raw_chunk_compression() == Reader::NONE ? "uncompressed" : "compressed") + " frames of "
                  + std::to_string(reader.get_element_size() * 8) + " bits (compressed raw frames are not supported)");
    const uint32_t width = (uint32_t)reader.image_shape()[1], height = (uint32_t)reader.image_shape()[0];
    const size_t n = (size_t)6 * width * height;
    std::ifstream f(file, std::ios::binary | std::ios::ate);
    if (!f) arg_error("--jungfrau-calibration: cannot open " + file);
    const std::streamoff bytes = f.tellg();
    if (bytes < 0 || (uint64_t)bytes != (uint64_t)n * sizeof(float))
        arg_error("--jungfrau-calibration: " + file + " holds " + std::to_string((long long)bytes) + " bytes, the 6 x " + std::to_string(width) + " x "
                  + std::to_string(height) + " float32 values of this detector are " + std::to_string(n * sizeof(float)));
    planes.resize(n);
    f.seekg(0);
    if (!f.read(reinterpret_cast<char*>(planes.data()), bytes)) arg_error("--jungfrau-calibration: cannot read " + file);
    return planes;
}
static int set_jungfrau_calibration(ffs_ctx* cx, const std::vector<float>& planes, size_t n_px) {
    ffs_jungfrau_calibration cal{};
    for (int s = 0; s < 3; ++s) {
        cal.pedestal[s] = planes.data() + (size_t)s * n_px;
        cal.factor[s] = planes.data() + (size_t)(3 + s) * n_px;
    }
    return ffs_ctx_set_jungfrau_calibration(cx, &cal);
}

// --pixel-stats PREFIX, after the last wait: the contexts' statistics merged on the host -- counts and sums add (the sums of squares modulo
// 2^64, as each context's own), the maximum is the largest -- and written as four raw little-endian files of width x height values.
static bool write_pixel_stats(const std::string& prefix, const std::vector<ffs_ctx*>& ctxs, uint32_t width, uint32_t height) {
    const size_t n = (size_t)width * height;
    std::vector<uint32_t> count(n, 0), max(n, 0), c1, m1;
    std::vector<uint64_t> sum(n, 0), sum_sq(n, 0), s1, q1;
    uint64_t frames = 0;
    for (size_t k = 0; k < ctxs.size(); ++k) {
        ffs_pixel_stats st{};
        if (k == 0) {
            st.count = count.data(); st.sum = sum.data(); st.sum_sq = sum_sq.data(); st.max = max.data();
        } else {
            c1.resize(n); m1.resize(n); s1.resize(n); q1.resize(n);
            st.count = c1.data(); st.sum = s1.data(); st.sum_sq = q1.data(); st.max = m1.data();
        }
        FFS_CHECK(ctxs[k], ffs_ctx_get_pixel_stats(ctxs[k], &st));
        frames += st.n_frames;
        if (k == 0) continue;
        for (size_t i = 0; i < n; ++i) {
            count[i] += c1[i];
            sum[i] += s1[i];
            sum_sq[i] += q1[i];
            max[i] = std::max(max[i], m1[i]);
        }
    }
    auto write = [&](const char* suffix, const void* data, size_t bytes) {
        const std::string name = prefix + suffix;
        std::ofstream f(name, std::ios::binary | std::ios::trunc);
        if (!f || !f.write(static_cast<const char*>(data), (std::streamsize)bytes) || !f.flush()) {
            std::printf("Error: --pixel-stats: cannot write %s\n", name.c_str());
            return false;
        }
        return true;
    };
    if (!write(".count.u32", count.data(), n * 4) || !write(".sum.u64", sum.data(), n * 8) || !write(".sum_sq.u64", sum_sq.data(), n * 8)
        || !write(".max.u32", max.data(), n * 4))
        return false;
    std::printf("Pixel statistics: %llu frames -> %s.{count.u32,sum.u64,sum_sq.u64,max.u32}\n", (unsigned long long)frames, prefix.c_str());
    return true;
}

// (--gain-map: the file is held against the frame source's shape as soon as the source is open, ahead of the verdict on the devices -- a
// usage error is reported as one wherever the driver runs)
static int open_source_beside_runtime(const Args& args, Stamps& stamp, std::unique_ptr<Reader>& reader, std::vector<float>& gain_map,
                                      std::vector<float>& jungfrau_planes) {
    int reader_rc = 0;
    std::atomic<bool> give_up{false};
    JoinedThread reader_holder;
    reader_holder.th = std::thread([&args, &give_up, &reader, &reader_rc] { reader_rc = open_reader(args, give_up, reader); });
    stamp("arguments parsed");
    const int n_devices = ffs_device_count();
    if (!args.gain_map.empty()) {
        reader_holder.th.join();
        if (reader_rc != 0) return reader_rc;
        gain_map = read_gain_map(args, (uint32_t)reader->image_shape()[1], (uint32_t)reader->image_shape()[0]);
    }
    if (!args.jungfrau_calibration.empty()) {   // (likewise)
        if (reader_holder.th.joinable()) reader_holder.th.join();
        if (reader_rc != 0) return reader_rc;
        jungfrau_planes = read_jungfrau_calibration(args, *reader);
    }
    if (args.radial_bins) {   // (--radial-bins needs the geometry --dmin needs: without it a usage error, like a bad --gain-map, wherever the driver runs)
        if (reader_holder.th.joinable()) reader_holder.th.join();
        if (reader_rc != 0) return reader_rc;
        const bool detector = args.detector_set || (reader->get_beam_center() && reader->get_pixel_size() && reader->get_detector_distance());
        const bool wavelength = args.wavelength_set || reader->get_wavelength();
        if (!detector) arg_error("--radial-bins needs the detector geometry (distance, beam centre, pixel size): the frame source has none, pass --detector");
        if (!wavelength) arg_error("--radial-bins needs the wavelength: the frame source has none, pass --wavelength");
    }
    if (n_devices < 1) {  // cuda_arg_parser.cc:56-61
        give_up.store(true);
        std::printf("\033[1;31mError: Could not select GPU device\033[0m\n");
        return 1;
    }
    stamp("HIP runtime initialised (first device query)");
    char name[256];
    if (ffs_device_name(args.device, name, sizeof name) != FFS_OK) {
        give_up.store(true);
        std::printf("\033[1;31mError: Could not select GPU device\033[0m\n");
        return 1;
    }
    std::printf("Using %s\n", name);
    if (reader_holder.th.joinable()) reader_holder.th.join();
    if (reader_rc != 0) return reader_rc;
    stamp("frame source opened (beside the runtime's initialisation)");
    return 0;
}

// The reference builds one binary per pixel width and exits with the data's bit depth on a
// mismatch (spotfinder.cc:468-476) so that the service relaunches spotfinder32
// (service.py:503-507).  This binary handles both widths; --strict-dtype (or being invoked
// as spotfinder / spotfinder32 with FFS_STRICT_DTYPE set) restores the exit-code protocol.  -> 0, or the exit code
static int check_dtype(const Args& args, const char* argv0, size_t bytes_per_pixel) {
    const std::string self = fs::path(argv0).filename().string();
    const size_t expect = self == "spotfinder32" ? 4 : 2;
    if ((args.strict_dtype || std::getenv("FFS_STRICT_DTYPE")) && bytes_per_pixel != expect) {
        std::printf("Error: Data type mismatch; This executable only accepts %zu bit != %zu\n", expect * 8,
                    bytes_per_pixel * 8);
        return (int)(bytes_per_pixel * 8);
    }
    return 0;
}

// The reference hands the frame source's trusted maximum to every launch (spotfinder.cc:482,868,879) and its kernels
// refuse centre pixels above it (kernels/thresholding.cu:208-215).  Here: --max-valid trusted (default) does the same
// whenever that maximum says something, i.e. lies below the pixel type's own maximum (the reference narrows the int64 to
// pixel_t, spotfinder.cu:155,167 -- a cut-off above 65535 on 16-bit data wraps there; here it means "no pixel is above it").
// < 0: no test
static int64_t max_valid_pixel(const std::string& arg, const Reader& reader, size_t bytes_per_pixel) {
    const int64_t trusted_px_max = reader.get_trusted_range()[1];
    const int64_t type_max = bytes_per_pixel == 2 ? 65535ll : 4294967295ll;
    if (arg == "trusted") return (trusted_px_max >= 0 && trusted_px_max < type_max) ? trusted_px_max : -1;
    if (arg != "none") return std::stoll(arg);
    return -1;
}

struct Experiment {
    DetectorGeometry detector;
    float wavelength = 0, oscillation_start = 0, oscillation_width = 0;
};

// detector geometry / wavelength (spotfinder.cc:484-587), from the command line or the frame source.  -> 0, or the exit code
static int read_experiment(const Args& args, const Reader& reader, Experiment& ex) {
    DetectorGeometry& detector = ex.detector;
    if (args.detector_set) {
        try {
            detector = detector_from_json(args.detector_json);
        } catch (const std::exception& e) {
            std::printf("Error: %s\n", e.what());
            return 1;
        }
    } else {
        const auto bc = reader.get_beam_center();
        const auto ps = reader.get_pixel_size();
        const auto dd = reader.get_detector_distance();
        if (!bc) { std::printf("Error: No beam center available from file. Please pass detector metadata with --distance.\n"); return 1; }
        if (!ps) { std::printf("Error: No pixel size available from file. Please pass detector metadata with --distance.\n"); return 1; }
        if (!dd) { std::printf("Error: No detector distance available from file. Please pass metadata with --distance.\n"); return 1; }
        detector.distance = *dd;
        detector.beam_center_x = (*bc)[1];
        detector.beam_center_y = (*bc)[0];
        detector.pixel_size_x = (*ps)[1];
        detector.pixel_size_y = (*ps)[0];
    }
    if (args.wavelength_set) {
        ex.wavelength = args.wavelength;
    } else {
        const auto w = reader.get_wavelength();
        if (!w) {
            std::printf("Error: No wavelength provided. Please pass wavelength using: --wavelength\n");
            return 1;
        }
        ex.wavelength = *w;
        std::printf("Got wavelength from file: %f \xc3\x85\n", ex.wavelength);
    }
    std::printf("Detector geometry:\n    Distance:    %.1f mm\n    Beam Center: %.1f px %.1f px\nBeam Wavelength: %.2f \xc3\x85\n",
                detector.distance * 1000, detector.beam_center_x, detector.beam_center_y, ex.wavelength);
    const auto osc = reader.get_oscillation();
    ex.oscillation_start = osc[0];
    ex.oscillation_width = osc[1];
    if (ex.oscillation_width > 0)
        std::printf("Oscillation:  Start: %.2f\xc2\xb0  Width: %.2f\xc2\xb0\n", ex.oscillation_start, ex.oscillation_width);
    return 0;
}

// --integrate FILE, ahead of the run: the flat single-panel geometry of kabsch_space.hpp and the file's records as a shoebox table
// (shoebox_geometry.hpp), a job opened on every context.  The geometry is printed as the key=value words `ffs_hosttool shoebox` takes, every
// number as %.17g (it parses back to the same float64).  -> 0, or the exit code
static int open_integration(const Args& args, const Experiment& ex, bool rotation, const std::vector<ffs_ctx*>& ctxs, size_t& n_boxes) {
    if (!rotation) {
        std::printf("Error: --integrate needs a rotation source (an oscillation width above 0)\n");
        return 1;
    }
    const DetectorGeometry& d = ex.detector;
    const KabschGeometry kg{d.distance * 1000.0, d.beam_center_x, d.beam_center_y, d.pixel_size_x * 1000.0, d.pixel_size_y * 1000.0, ex.wavelength,
                            ex.oscillation_start, ex.oscillation_width};
    std::vector<ffs_shoebox> table;
    try {
        for (const ShoeboxRecord& r : read_shoebox_file(args.integrate)) table.push_back(shoebox_from_record(kg, r));
    } catch (const std::exception& e) {
        std::printf("Error: --integrate: %s\n", e.what());
        return 1;
    }
    if (table.size() > 0xFFFFFFFFull) {
        std::printf("Error: --integrate: more than 2^32 - 1 reflections\n");
        return 1;
    }
    const ffs_scan_geometry g = shoebox_flat_geometry(kg);
    const double delta_b = shoebox_delta(args.integrate_n_sigma, args.sigma_b), delta_m = shoebox_delta(args.integrate_n_sigma, args.sigma_m);
    for (ffs_ctx* cx : ctxs)
        FFS_CHECK(cx, ffs_ctx_shoebox_begin(cx, &g, table.data(), (uint32_t)table.size(), args.integrate_algorithm, delta_b, delta_m));
    n_boxes = table.size();
    std::printf("Integration: %zu reflections from %s, %s foreground of %.17g x sigma_b %.17g and sigma_m %.17g degrees, %s background\n", n_boxes, args.integrate.c_str(),
                args.integrate_algorithm == FFS_SHOEBOX_DIALS ? "dials" : "ellipsoid", args.integrate_n_sigma, args.sigma_b, args.sigma_m,
                args.integrate_background ? "glm" : "tukey");
    std::printf("Integration geometry: distance=%.17g beam_x=%.17g beam_y=%.17g pixel_x=%.17g pixel_y=%.17g wavelength=%.17g osc_start=%.17g osc_width=%.17g\n",
                kg.distance_mm, kg.beam_center_x_px, kg.beam_center_y_px, kg.pixel_size_x_mm, kg.pixel_size_y_mm, kg.wavelength, kg.oscillation_start, kg.oscillation_width);
    return 0;
}

// --predict CRYSTAL, ahead of the run: the reflections of the source's geometry and image count predicted on the first context
// (ffs_ctx_predict), the records into PREFIX.predictions, one summary line, and a shoebox job opened on every context with the boxes not flagged
// FFS_PREDICT_BOX_REFUSED; from there on the run is --integrate's.  The candidate count of the line is csrc/predict_plan.hpp's.  -> 0, or the
// exit code
static int open_prediction(const Args& args, const Experiment& ex, bool rotation, uint32_t num_images, int W, int H, const std::vector<ffs_ctx*>& ctxs, size_t& n_boxes) {
    if (!rotation) {
        std::printf("Error: --predict needs a rotation source (an oscillation width above 0)\n");
        return 1;
    }
    const DetectorGeometry& d = ex.detector;
    const KabschGeometry kg{d.distance * 1000.0, d.beam_center_x, d.beam_center_y, d.pixel_size_x * 1000.0, d.pixel_size_y * 1000.0, ex.wavelength,
                            ex.oscillation_start, ex.oscillation_width};
    ffs_crystal crystal{};
    try {
        crystal = read_crystal_file(args.predict, args.predict_centring);
    } catch (const std::exception& e) {
        std::printf("Error: --predict: %s\n", e.what());
        return 1;
    }
    const ffs_scan_geometry g = shoebox_flat_geometry(kg);
    const double delta_b = shoebox_delta(args.integrate_n_sigma, args.sigma_b), delta_m = shoebox_delta(args.integrate_n_sigma, args.sigma_m);
    ffs_ctx* cx0 = ctxs[0];
    uint32_t n = 0;
    float ms = 0.0f;
    int rc = ffs_ctx_predict(cx0, &g, &crystal, num_images, args.predict_dmin, delta_b, delta_m, nullptr, 0, &n, nullptr);
    if (rc != FFS_OK && rc != FFS_ERR_OVERFLOW) FFS_CHECK(cx0, rc);
    std::vector<ffs_prediction> records(n);
    if (n) FFS_CHECK(cx0, ffs_ctx_predict(cx0, &g, &crystal, num_images, args.predict_dmin, delta_b, delta_m, records.data(), n, &n, &ms));
    ffsamd::ShoeboxGeometry mg;
    ffsamd::PredictCrystal mx;
    ffsamd::PredictSetup setup{};
    std::memcpy(&mg, &g, sizeof mg);
    std::memcpy(&mx, &crystal, sizeof mx);
    (void)ffsamd::predict_refusal(mg, mx, num_images, args.predict_dmin, delta_b, delta_m, W, H, setup);   // (the library has taken the call)
    const std::string name = args.integrate_out + ".predictions";
    std::ofstream f(name, std::ios::binary | std::ios::trunc);
    if (!f || !f.write(reinterpret_cast<const char*>(records.data()), (std::streamsize)(records.size() * sizeof(ffs_prediction))) || !f.flush()) {
        std::printf("Error: --integrate-out: cannot write %s\n", name.c_str());
        return 1;
    }
    std::printf("Prediction: %s -> %s (dmin %.17g, centring %c, %.3f ms on the GPU)\n", predict_summary_line(setup.n_candidates, records).c_str(), name.c_str(),
                args.predict_dmin, "PIFABCR"[args.predict_centring], (double)ms);
    const std::vector<ffs_shoebox> table = boxes_of_predictions(records);
    for (ffs_ctx* cx : ctxs)
        FFS_CHECK(cx, ffs_ctx_shoebox_begin(cx, &g, table.data(), (uint32_t)table.size(), args.integrate_algorithm, delta_b, delta_m));
    n_boxes = table.size();
    std::printf("Integration: %zu reflections from the prediction, %s foreground of %.17g x sigma_b %.17g and sigma_m %.17g degrees, %s background\n", n_boxes,
                args.integrate_algorithm == FFS_SHOEBOX_DIALS ? "dials" : "ellipsoid", args.integrate_n_sigma, args.sigma_b, args.sigma_m,
                args.integrate_background ? "glm" : "tukey");
    std::printf("Integration geometry: distance=%.17g beam_x=%.17g beam_y=%.17g pixel_x=%.17g pixel_y=%.17g wavelength=%.17g osc_start=%.17g osc_width=%.17g\n",
                kg.distance_mm, kg.beam_center_x_px, kg.beam_center_y_px, kg.pixel_size_x_mm, kg.pixel_size_y_mm, kg.wavelength, kg.oscillation_start, kg.oscillation_width);
    std::printf("Prediction scan: width=%d height=%d n_images=%u\n", W, H, num_images);
    return 0;
}

// --integrate, after the last wait: the records into PREFIX.shoebox_sums and the summary line.  One context hands out its records; with
// several, their integer accumulators and histograms are added on the host (as --pixel-stats adds its planes) and the records are made from
// the sums by the function the library calls (csrc/shoebox_model.hpp).
static bool write_integration(const Args& args, const std::vector<ffs_ctx*>& ctxs, size_t n_boxes) {
    std::vector<ffs_shoebox_sum> sums(n_boxes);
    uint32_t n = 0;
    if (ctxs.size() == 1) {
        FFS_CHECK(ctxs[0], ffs_ctx_get_shoebox_sums(ctxs[0], args.integrate_background, sums.data(), (uint32_t)n_boxes, &n));
    } else {
        std::vector<ffsamd::ShoeboxAcc> acc(n_boxes, ffsamd::ShoeboxAcc{});
        std::vector<uint32_t> hist(n_boxes * (size_t)ffsamd::kSpotBgBins, 0u), bins((size_t)ffsamd::kSpotBgBins);
        std::vector<ffs_shoebox_sum> part(n_boxes);
        for (ffs_ctx* cx : ctxs) {
            FFS_CHECK(cx, ffs_ctx_get_shoebox_sums(cx, args.integrate_background, part.data(), (uint32_t)n_boxes, &n));
            for (size_t i = 0; i < n_boxes; ++i) {
                acc[i].fg_sum += part[i].fg_sum, acc[i].m_x += part[i].m_x, acc[i].m_y += part[i].m_y, acc[i].m_z += part[i].m_z;
                acc[i].fg_count += part[i].fg_count, acc[i].n_overflow += part[i].n_overflow, acc[i].flags |= part[i].flags;
                FFS_CHECK(cx, ffs_ctx_get_shoebox_histogram(cx, (uint32_t)i, bins.data()));
                for (size_t v = 0; v < bins.size(); ++v) hist[i * bins.size() + v] += bins[v];
            }
        }
        for (size_t i = 0; i < n_boxes; ++i) {
            const ffsamd::ShoeboxSum r = ffsamd::shoebox_sum(acc[i], hist.data() + i * (size_t)ffsamd::kSpotBgBins, args.integrate_background);
            static_assert(sizeof r == sizeof sums[i], "the model's record is ffs_shoebox_sum");
            std::memcpy(&sums[i], &r, sizeof r);
        }
    }
    const std::string name = args.integrate_out + ".shoebox_sums";
    std::ofstream f(name, std::ios::binary | std::ios::trunc);
    if (!f || !f.write(reinterpret_cast<const char*>(sums.data()), (std::streamsize)(sums.size() * sizeof(ffs_shoebox_sum))) || !f.flush()) {
        std::printf("Error: --integrate-out: cannot write %s\n", name.c_str());
        return false;
    }
    std::printf("Integration: %s -> %s\n", shoebox_summary_line(sums.data(), sums.size()).c_str(), name.c_str());
    return true;
}

// frames per GPU batch.  Chunks: 16 for long runs (120 MB of staging per batch for Eiger-16M: the threshold kernels are tuned
// for 16-32 frames and PCIe, not the GPU, is the limit), 8 for runs below 2048 images per GPU -- a stream's device buffers
// (37 MB per frame of the batch) are prepared by the driver on FIRST USE at ~60 GB/s, so four assemblies of 16 frames cost a
// run its first 40 ms, of 8 frames 20 ms (1000 frames: 6.0 k frames/s against 5.2-5.5 k).  Decoded frames are five times
// larger: 4.  Never more than half the data set per GPU.
static uint32_t default_batch(bool gpu_decode, uint32_t num_images, uint32_t n_dev) {
    const uint32_t batch_dflt = !gpu_decode ? 4u : (num_images >= 2048u * n_dev ? 16u : 8u);
    return std::max<uint32_t>(1, std::min<uint32_t>(batch_dflt, num_images / (2 * n_dev)));
}

// The exchange between GPUs (RCCL communicators: 2-5 s to load the library and initialise, measured in round 5 -- it was what two
// contexts cost a 1000-image request) serves rotation sweeps only -- every frame's strong-pixel list has to reach the GPU that owns
// the 3D stack -- so stills never pay it, and a sweep initialises it on a helper thread beside the contexts and the first batches
// (joined before the first batch is added to the stack).
class Exchange {
    JoinedThread holder_;
    std::once_flag joined_;
  public:
    // (--gather rccl names the transport: contexts that share a GPU then send to their own rank, which a one-GPU box can rehearse)
    void start(const std::vector<int>& devices, bool gather_rccl) {
        holder_.th = std::thread([&devices, gather_rccl] { (void)ffs_multi_init(devices.data(), (int)devices.size(), gather_rccl ? "rccl" : nullptr); });
    }
    void join() { std::call_once(joined_, [this] { if (holder_.th.joinable()) holder_.th.join(); }); }
};

static bool create_context(int device, const FrameShape& shape, uint32_t batch, ffs_ctx** out) {
    if (ffs_ctx_create(device, shape.width, shape.height, (int)shape.bytes_per_pixel, batch, 0, out) == FFS_OK) return true;
    std::printf("Error: %s\n", ffs_last_error(nullptr));
    return false;
}

// the pixel mask and the resolution filter into every context (upload_mask, spotfinder.cc:61-108; :648-683)
static void upload_masks(const std::vector<ffs_ctx*>& ctxs, const Reader& reader, const Args& args, const Experiment& ex, const FrameShape& shape) {
    const uint32_t width = shape.width, height = shape.height;
    {
        size_t valid = 0;
        const auto t0 = Clock::now();
        const auto mask = reader.get_mask();
        if (mask) for (uint8_t v : *mask) valid += v != 0;
        else valid = shape.pixels();
        for (ffs_ctx* cx : ctxs) FFS_CHECK(cx, ffs_ctx_set_mask(cx, mask ? mask->data() : nullptr));
        const double ms = ms_between(t0, Clock::now());
        std::printf("Uploaded mask (%.2f Mpx) in %.2f ms (%.1f GBps)\n", valid / 1e6, ms,
                    (double)width * height * ctxs.size() / (ms * 1e-3) / 1e9);
    }
    if (const auto mask = reader.get_mask(); args.writeout && mask) write_mask_png("mask_source.png", mask->data(), width, height);
    if (args.dmin > 0 || args.dmax > 0) {
        const DetectorGeometry& detector = ex.detector;
        for (ffs_ctx* cx : ctxs)
            FFS_CHECK(cx, ffs_ctx_apply_resolution_mask(cx, ex.wavelength, detector.distance, detector.beam_center_x,
                                                        detector.beam_center_y, detector.pixel_size_x,
                                                        detector.pixel_size_y, args.dmin, args.dmax));
        if (args.writeout) {
            std::vector<uint8_t> m(shape.pixels());
            FFS_CHECK(ctxs[0], ffs_ctx_get_mask(ctxs[0], m.data()));
            write_mask_png("mask_calculated.png", m.data(), width, height);
        }
    }
}

static ffs_params make_params(const Args& args, bool rotation, int64_t max_valid) {
    ffs_params prm;
    ffs_default_params(&prm);
    prm.min_spot_size = args.min_spot_size;
    prm.min_spot_size_3d = args.min_spot_size_3d;
    prm.max_peak_centroid_separation = args.max_sep;
    prm.want_reflections = (!rotation && (args.save_h5 || args.output_for_index)) ? 1 : 0;
    if (args.spot_background) prm.want_reflections = 1;   // (the spots whose backgrounds are measured are the reflections left after both filters)
    prm.want_strong_mask = args.writeout ? 1 : 0;
    prm.algorithm = args.algo;
    prm.max_valid = max_valid;
    prm.min_count = (int32_t)args.min_count;
    prm.kernel_half_x = args.kernel_half_x;
    prm.kernel_half_y = args.kernel_half_y;
    if (args.validate) prm.want_strong_mask = 1;   // the masks are what --validate compares (spotfinder.cc:1012-1053)
    return prm;
}

// --validate (spotfinder.cc:1012-1053 compares every image with the CPU baseline, which is test infrastructure here and
// not linked into the product): every batch also goes through a second context per GPU whose threshold stage shares
// nothing with the hot path's but the predicate -- no streaming kernel, no screen, no queue: the window of EVERY valid
// pixel is gathered from memory (tuning "threshold_path" = 2; the extended algorithm: its plain one-pixel-per-lane first
// pass and the grid-wide sparse kernels) -- and the two strong-pixel masks are compared image by image.
static bool create_validation_contexts(const std::vector<int>& devices, const std::vector<ffs_ctx*>& ctxs, const FrameShape& shape, uint32_t batch,
                                       const ffs_params& prm, int max_valid_scope, double gain, const std::vector<float>& gain_map,
                                       std::vector<ffs_ctx*>& vctxs) {
    for (size_t di = 0; di < devices.size(); ++di) {
        if (!create_context(devices[di], shape, batch, &vctxs[di])) return false;
        ffs_ctx* v = vctxs[di];
        FFS_CHECK(v, ffs_ctx_set_tuning(v, "threshold_path", 2));
        FFS_CHECK(v, ffs_ctx_set_tuning(v, "ext_first_pass", 0));
        FFS_CHECK(v, ffs_ctx_set_tuning(v, "sparse_stage", 1));
        FFS_CHECK(v, ffs_ctx_set_tuning(v, "strong_log", 0));
        std::vector<uint8_t> m(shape.pixels());   // the mask as the first context holds it (resolution filter included)
        FFS_CHECK(ctxs[di], ffs_ctx_get_mask(ctxs[di], m.data()));
        FFS_CHECK(v, ffs_ctx_set_mask(v, m.data()));
        FFS_CHECK(v, ffs_ctx_set_params(v, &prm));
        FFS_CHECK(v, ffs_ctx_set_max_valid_scope(v, max_valid_scope));
        FFS_CHECK(v, ffs_ctx_set_gain(v, gain));
        if (!gain_map.empty()) FFS_CHECK(v, ffs_ctx_set_gain_map(v, gain_map.data()));
    }
    std::printf("Validation: every image is also decided by the gather path (every valid pixel's window summed from memory)\n");
    return true;
}

// Workers are dealt round-robin to the GPUs; each is kept on the CPUs of its GPU's NUMA node (where the node is known
// and leaves it CPUs of this process's affinity set), so that the frames it reads, its pinned staging buffer -- first
// touched by hipHostMalloc on this thread -- and the GPU's PCIe root sit on one socket.  --no-numa-pinning turns it off.
static std::vector<std::optional<cpu_set_t>> numa_cpu_sets(const std::vector<int>& devices, bool verbose) {
    std::vector<std::optional<cpu_set_t>> node_cpus(devices.size());
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    sched_getaffinity(0, sizeof allowed, &allowed);
    for (size_t di = 0; di < devices.size(); ++di) {
        const int node = ffs_device_numa_node(devices[di]);
        if (node < 0) continue;
        std::ifstream f("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist");
        std::string list;
        if (!std::getline(f, list)) continue;
        cpu_set_t set;
        CPU_ZERO(&set);
        std::stringstream ss(list);
        std::string tok;
        int n_set = 0;
        while (std::getline(ss, tok, ',')) {
            const size_t dash = tok.find('-');
            const int lo = std::atoi(tok.c_str()), hi = dash == std::string::npos ? lo : std::atoi(tok.c_str() + dash + 1);
            for (int cpu = lo; cpu <= hi && cpu < CPU_SETSIZE; ++cpu)
                if (CPU_ISSET(cpu, &allowed)) { CPU_SET(cpu, &set); ++n_set; }
        }
        if (n_set > 0) node_cpus[di] = set;
    }
    if (verbose)
        for (size_t di = 0; di < devices.size(); ++di)
            std::printf("GPU %d: NUMA node %d%s\n", devices[di], ffs_device_numa_node(devices[di]),
                        node_cpus[di] ? ", workers pinned to its CPUs" : " (workers not pinned)");
    return node_cpus;
}

// How many of the -n threads read.  The reference needs one thread per frame in flight because its threads decompress
// (service.py passes --threads 40); here a reader only moves chunks from the frame source into pinned memory, and eight
// per GPU saturate PCIe (tools/cli_profile.sh) -- beyond that they contend for the page cache's locks.  Threads that
// decompress on the host (--cpu-decode, --writeout) are all used.
static uint32_t reader_count(const Args& args, bool gpu_decode, uint32_t n_dev) {
    uint32_t n_workers = args.threads;
    if (gpu_decode && !args.all_threads) n_workers = std::min<uint32_t>(n_workers, 8 * n_dev);
    n_workers = std::max(n_workers, n_dev);
    if (args.verbose && n_workers != args.threads) std::printf("Workers: %u of the %u threads read for the GPU(s)\n", n_workers, args.threads);
    return n_workers;
}

// ---- --gather rccl: the spot centres of one ROUND of batches (local batch q of every GPU) through ffs_multi_gather_rows ----------
// The collectors meet once per round; the last to arrive runs the collective for all (counts by ncclAllGather, rows by ncclSend /
// ncclRecv to the first GPU, one copy to the host) and everybody takes its own batch's rows from the gathered table.  A round
// that cannot fill up (the data set ends, an interrupt) is served from the host arrays, as `--gather host` serves all of them.
class GatherRound {
    static constexpr uint32_t kCap = 1u << 20;
    const BatchPipeline& pipeline_;
    Exchange& exchange_;
    const uint32_t n_dev_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<ffs_stream*> streams_;
    std::vector<uint64_t> n_rows_, row_at_;   // per GPU: rows of its batch, where they start in `rows_`
    std::vector<float> rows_;
    const std::vector<int> devices_, comm_devices_;   // per GPU; and the communicator's, as ffs_multi_init made it from them
    uint32_t arrived_ = 0;
    uint64_t round_ = 0;                      // rounds served so far
    bool ok_ = false;                         // the round just served went through RCCL
  public:
    std::atomic<uint64_t> rccl_rounds{0}, host_rounds{0};
    GatherRound(const std::vector<int>& devices, const BatchPipeline& pipeline, Exchange& exchange)
        : pipeline_(pipeline), exchange_(exchange), n_dev_((uint32_t)devices.size()), streams_(n_dev_, nullptr), n_rows_(n_dev_, 0),
          row_at_(n_dev_, 0), rows_((size_t)kCap * 4), devices_(devices), comm_devices_(ffsamd::distinct_devices(devices)) {}
    // -> pointer to this GPU's rows (frame id bits, x, y, z) of the round, or nullptr: read them from the host arrays
    const float* rows_of(uint32_t di, uint64_t q, ffs_stream* st, uint32_t my_rows) {
        const bool full_round = (q + 1) * n_dev_ <= pipeline_.total_batches();   // every GPU has a local batch q
        if (!full_round) { host_rounds += 1; return nullptr; }
        std::unique_lock<std::mutex> lock(mu_);
        // (waits in slices: a failure or the end of the readers is announced on the GPUs' condition variables, not on this one)
        while (!(round_ == q || pipeline_.winding_down())) cv_.wait_for(lock, 20ms);   // the previous round has been taken by everybody
        if (round_ != q) { host_rounds += 1; return nullptr; }
        streams_[di] = st;
        n_rows_[di] = my_rows;
        if (++arrived_ == n_dev_) {
            exchange_.join();
            // where the library puts every GPU's rows: the layout it gathers by (csrc/sweep_plan.hpp)
            const ffsamd::GatherLayout lay = ffsamd::gather_layout(devices_, n_rows_, comm_devices_);
            for (uint32_t g = 0; g < n_dev_; ++g) row_at_[g] = lay.row_at(g);
            uint32_t got = 0;
            ok_ = lay.total <= kCap && ffs_multi_gather_rows(streams_.data(), n_dev_, 0, rows_.data(), kCap, &got) == FFS_OK && got == lay.total;
            (ok_ ? rccl_rounds : host_rounds) += 1;
            arrived_ = 0;
            round_ = q + 1;
            cv_.notify_all();
        } else {
            while (!(round_ > q || pipeline_.winding_down())) cv_.wait_for(lock, 20ms);
            if (round_ <= q) {   // the round cannot fill up any more (the readers have stopped): everybody reads the host arrays
                arrived_ = 0;
                host_rounds += 1;
                return nullptr;
            }
        }
        return ok_ ? rows_.data() + (size_t)row_at_[di] * 4 : nullptr;
    }
};

// ---- what is done with a collected batch (the reference's post-processing of an image, :901-1087): the pipeline's callback ----------
class BatchReport {
    const Args& args_;
    const ffs_params& prm_;
    const FrameShape shape_;
    const bool rotation_;
    std::vector<ffs_ctx*> ctxs_;
    ffs_stack3d* stack_;
    Exchange& exchange_;
    GatherRound* gather_;   // --gather rccl, or nullptr
    PipeHandler* pipe_;
    std::mutex& print_mutex_;
    std::mutex centers_mutex_;
  public:
    std::map<uint32_t, std::vector<float>> reflection_centers_2d;  // spotfinder.cc:706-708
    std::atomic<uint32_t> validate_mismatches{0};

    BatchReport(const Args& args, const ffs_params& prm, const FrameShape& shape, bool rotation, const std::vector<ffs_ctx*>& ctxs, ffs_stack3d* stack,
                Exchange& exchange, GatherRound* gather, PipeHandler* pipe, std::mutex& print_mutex)
        : args_(args), prm_(prm), shape_(shape), rotation_(rotation), ctxs_(ctxs), stack_(stack), exchange_(exchange), gather_(gather), pipe_(pipe),
          print_mutex_(print_mutex) {}

    bool operator()(const BatchView& batch) {
        const ffs_frame_result* res = batch.results;
        const uint32_t nres = batch.count;
        if (rotation_) {
            // key = image number read (rotation_slices[offset_image_num], :913-918); the stack has its own lock (the
            // reference's rotation_slices_mutex), held only while the transfer is enqueued
            exchange_.join();   // (the exchange's communicators, initialised beside the run so far)
            if (ffs_stack3d_add_batch(stack_, batch.stream) != FFS_OK) {
                std::printf("Error: %s\n", ffs_last_error(ctxs_[batch.gpu]));
                return false;
            }
        }
        const float* round_rows = nullptr;   // --gather rccl: this batch's centre rows as they came back from the collective
        if (gather_) {
            uint32_t my_rows = 0;
            for (uint32_t i = 0; i < nres; ++i) my_rows += res[i].n_reflections;
            round_rows = gather_->rows_of(batch.gpu, batch.q, batch.stream, my_rows);
        }
        // --spot-background: the batch's backgrounds, once, between its wait and the stream's next submit (the collector releases the batch's
        // assembly only after this callback); image i's entries follow image i - 1's, n_reflections each
        SpotBackgrounds backgrounds;
        if (args_.spot_background) {
            uint32_t n_bg = 0;
            const int rc = args_.spot_background_glm ? ffs_stream_spot_backgrounds_glm(batch.stream, args_.spot_background, &backgrounds.glm, &n_bg, nullptr)
                                                     : ffs_stream_spot_backgrounds(batch.stream, args_.spot_background, &backgrounds.tukey, &n_bg, nullptr);
            if (rc != FFS_OK) {
                std::printf("Error: %s\n", ffs_last_error(ctxs_[batch.gpu]));
                return false;
            }
        }
        // --integrate: the batch's frames into the context's job, once, while they are still where the batch left them (image numbers are
        // consecutive inside a batch: batch_pipeline.hpp)
        if (args_.integrating() && nres > 0 && ffs_stream_shoebox_fold(batch.stream, res[0].frame_id, nullptr) != FFS_OK) {
            std::printf("Error: %s\n", ffs_last_error(ctxs_[batch.gpu]));
            return false;
        }
        // what this batch prints and sends goes out in one piece each (the collector is the one thread between the GPU and a
        // free staging area: a printf and a write per image, into pipes a Python caller drains, were on that path)
        std::string text, json_lines;
        for (uint32_t i = 0; i < nres; ++i) {
            const ffs_frame_result& r = res[i];
            const uint32_t image_num = (uint32_t)r.frame_id;
            if (args_.writeout && r.strong_mask)
                write_overlay(r, batch.staging + (size_t)i * batch.slot_bytes, shape_.bytes_per_pixel, shape_.width, shape_.height);
            if (args_.save_h5 && !rotation_) {  // :919-933
                std::vector<float> coms;
                for (uint32_t qq = 0; qq < r.n_reflections; ++qq) {
                    coms.push_back(r.reflections[qq].com_x);
                    coms.push_back(r.reflections[qq].com_y);
                    coms.push_back(r.reflections[qq].com_z);
                }
                std::lock_guard<std::mutex> lock(centers_mutex_);
                reflection_centers_2d[image_num + args_.start_index] = std::move(coms);
            }
            if (pipe_) append_json(r, batch.stream, i, round_rows, backgrounds, json_lines);
            if (backgrounds.tukey) backgrounds.tukey += r.n_reflections;
            if (backgrounds.glm) backgrounds.glm += r.n_reflections;
            append_text(r, batch.validation ? &batch.validation[i] : nullptr, batch, text);
        }
        if (pipe_ && !json_lines.empty()) pipe_->send_lines(json_lines);
        std::lock_guard<std::mutex> lock(print_mutex_);
        std::fwrite(text.data(), 1, text.size(), stdout);
        return true;
    }

  private:
    // --spot-background: an image's slice of the batch's records under the model asked for (the other pointer is null; both are null for a
    // batch without a single reflection)
    struct SpotBackgrounds {
        const ffs_spot_background* tukey = nullptr;
        const ffs_spot_background_glm* glm = nullptr;
    };
    // one image's JSON line; keys in alphabetical order, as nlohmann dumps them (:997-1008)
    // --radial-bins: the image's profile as three arrays of N integers (behind "num_strong_pixels": the keys stay in alphabetical order)
    // -a radial_profile: what the threshold decided per shell, "radial_cutoff", "radial_median" and "radial_status", between "radial_count" and
    // "radial_sum" (a batch of another algorithm has none: nothing is added)
    static std::string radial_json(ffs_stream* stream, uint32_t frame_in_batch) {
        ffs_radial_profile prof{};
        if (ffs_stream_radial_profile(stream, frame_in_batch, &prof) != FFS_OK) return "";
        std::string c = ",\"radial_count\":[", s = ",\"radial_sum\":[", q = ",\"radial_sum_sq\":[";
        for (uint32_t b = 0; b < prof.n_bins; ++b) {
            const char* sep = b ? "," : "";
            c += sep + std::to_string(prof.count[b]);
            s += sep + std::to_string(prof.sum[b]);
            q += sep + std::to_string(prof.sum_sq[b]);
        }
        std::string t;
        const ffs_radial_shell* shells = nullptr;
        uint32_t n_shells = 0;
        if (ffs_stream_radial_thresholds(stream, frame_in_batch, &shells, &n_shells) == FFS_OK) {
            std::string cut = ",\"radial_cutoff\":[", med = ",\"radial_median\":[", status = ",\"radial_status\":[";
            for (uint32_t b = 0; b < n_shells; ++b) {
                const char* sep = b ? "," : "";
                cut += sep + std::to_string(shells[b].cutoff);
                med += sep + std::to_string(shells[b].median);
                status += sep + std::to_string(shells[b].status);
            }
            t = cut + "]" + med + "]" + status + "]";
        }
        return c + "]" + t + s + "]" + q + "]";
    }
    // --spot-background: a "%.17g" number (it parses back to the same float64), or null where the spot's ring gave no estimate
    static void append_g17(std::string& j, bool valid, double v) {
        char buf[40];
        if (valid) std::snprintf(buf, sizeof buf, "%.17g", v);
        j += valid ? buf : "null";
    }
    void append_json(const ffs_frame_result& r, ffs_stream* stream, uint32_t frame_in_batch, const float*& round_rows, const SpotBackgrounds& bg,
                     std::string& json_lines) const {
        std::string j = "{\"file\":" + json_escape(args_.file) + ",\"file-number\":" + std::to_string((uint32_t)r.frame_id)
                        + ",\"n_spots_total\":" + std::to_string(r.n_boxes)
                        + ",\"num_strong_pixels\":" + std::to_string(r.num_strong_pixels);
        if (args_.radial_bins) j += radial_json(stream, frame_in_batch);
        // the image's spots in reflection order: intensity = sum - pixels x mean; variance = sum + pixels^2 x mean / inliers (the counts' own
        // Poisson variance plus that of the estimated mean; under the GLM the mean rests on all the ring's pixels: / n_pixels); the keys stay
        // in alphabetical order around "spot_centers"
        std::string intensity, variance;
        double total_intensity = 0.0;
        if (args_.spot_background) {   // (bg may be null: a batch without a single reflection)
            j += ",\"spot_background_mean\":[";
            for (uint32_t qq = 0; qq < r.n_reflections; ++qq) {
                const bool glm = args_.spot_background_glm;
                const bool ok = (glm ? bg.glm[qq].status : bg.tukey[qq].status) == FFS_SPOT_BG_OK;
                const double sum = (double)r.reflections[qq].sum_intensity, k = (double)r.reflections[qq].num_pixels;
                const double mean = glm ? bg.glm[qq].mean : bg.tukey[qq].mean, basis = glm ? (double)bg.glm[qq].n_pixels : (double)bg.tukey[qq].n_inliers;
                const double i_spot = sum - k * mean, v_spot = ok ? sum + k * k * mean / basis : 0.0;
                if (qq) { j += ","; intensity += ","; variance += ","; }
                append_g17(j, ok, mean);
                append_g17(intensity, ok, i_spot);
                append_g17(variance, ok, v_spot);
                if (ok) total_intensity += i_spot;
            }
            j += "]";
        }
        if (args_.output_for_index) {
            j += ",\"spot_centers\":[";
            for (uint32_t qq = 0; qq < r.n_reflections; ++qq) {
                if (qq) j += ",";
                if (round_rows) {   // (frame id bits, x, y, z) rows in frame order: the next n_reflections are this image's
                    j += json_number(round_rows[1]) + "," + json_number(round_rows[2]) + "," + json_number(round_rows[3]);
                    round_rows += 4;
                } else {
                    j += json_number(r.reflections[qq].com_x) + "," + json_number(r.reflections[qq].com_y) + ","
                         + json_number(r.reflections[qq].com_z);
                }
            }
            j += "]";
        }
        if (args_.spot_background) {
            j += ",\"spot_intensity\":[" + intensity + "],\"spot_variance\":[" + variance + "],\"total_intensity\":";
            append_g17(j, true, total_intensity);
        }
        json_lines += j;
        json_lines += "}\n";
    }

    // one image's stdout lines; v: the validation context's result for the image, or nullptr
    void append_text(const ffs_frame_result& r, const ffs_frame_result* v, const BatchView& batch, std::string& text) {
        const uint32_t thread_id = batch.submitted_by, image_num = (uint32_t)r.frame_id, nres = batch.count;
        const float* tm = batch.timings;
        char line_buf[512];
        if (v) {  // :1012-1053
            const bool same = r.strong_mask && v->strong_mask && std::memcmp(r.strong_mask, v->strong_mask, shape_.pixels()) == 0
                              && r.num_strong_pixels == v->num_strong_pixels && r.n_boxes == v->n_boxes;
            if (same) std::snprintf(line_buf, sizeof line_buf, "Thread %2u, Image %4u: Compared: \033[32mMatch %u px\033[0m\n", thread_id, image_num, r.num_strong_pixels);
            else {
                std::snprintf(line_buf, sizeof line_buf, "Thread %2u, Image %4u: Compared: \033[1;31mMismatch (%u px from kernel)\033[0m\n", thread_id, image_num, r.num_strong_pixels);
                validate_mismatches += 1;
            }
            text += line_buf;
        }
        std::snprintf(line_buf, sizeof line_buf, "Extracted %u spots\n", r.n_components);  // connected_components.cc:119
        text += line_buf;
        if (prm_.min_spot_size > 0) {
            std::snprintf(line_buf, sizeof line_buf, "Removed %u spots with size < %u pixels\n", r.n_components - r.n_boxes, prm_.min_spot_size);
            text += line_buf;
        }
        if (prm_.want_reflections && r.n_filtered_sep > 0) {
            std::snprintf(line_buf, sizeof line_buf, "Filtered %u spots with peak-centroid distance > %s\n", r.n_filtered_sep, fmt_num(prm_.max_peak_centroid_separation).c_str());
            text += line_buf;
        }
        if (args_.threads == 1) {  // :1056-1076 (timings are per batch here)
            std::snprintf(line_buf, sizeof line_buf, "Thread %2u finished image %4u\n       Copy: %5.1f ms\n     Kernel: %5.1f ms\n  Post Copy: %5.1f ms\n"
                        "       Post: %5.1f ms\n             \xe2\x95\x90\xe2\x95\x90\xe2\x95\x90\xe2\x95\x90\xe2\x95\x90\xe2\x95\x90\xe2\x95\x90\xe2\x95\x90\n"
                        "     Total:  %5.1f ms (%.1f GBps)\n    %u strong pixels\n    %u filtered reflections (%u pixels)\n",
                        thread_id, image_num, tm[0] / nres, tm[1] / nres, tm[3] / nres, tm[2] / nres, tm[4] / nres,
                        (double)shape_.frame_bytes() * nres / (tm[4] * 1e-3) / 1e9, r.num_strong_pixels, r.n_boxes,
                        r.num_strong_pixels_filtered);
        } else {  // :1078-1085
            std::snprintf(line_buf, sizeof line_buf, "Thread %2u finished image %4u with %5u strong pixels, %4u filtered reflections (%u pixels)\n",
                        thread_id, image_num, r.num_strong_pixels, r.n_boxes, r.num_strong_pixels_filtered);
        }
        text += line_buf;
    }
};

// ---- after the run ---------------------------------------------------------------------------------------------------------------

// --index-basis PREFIX, after the sweep's finish: the 3D reflections' centres of mass through the indexer's basis-vector search (the reference's
// indexer.cc:171-245 with its constants), PREFIX.centres / .peaks / .basis_vectors and the lines the reference logs.  `ffs_hosttool indexbasis`
// on PREFIX.centres and the printed geometry writes the same bytes.  -> false on an error, which has been printed
static bool index_basis(const Args& args, ffs_ctx* ctx, const KabschGeometry& kg, const ffs_reflection* refl, uint32_t n) {
    const ffs_scan_geometry g = shoebox_flat_geometry(kg);
    std::vector<double> xyz(3 * (size_t)n), rlp(3 * (size_t)n), s1(3 * (size_t)n), mm(3 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) xyz[3 * (size_t)i] = refl[i].com_x, xyz[3 * (size_t)i + 1] = refl[i].com_y, xyz[3 * (size_t)i + 2] = refl[i].com_z;
    const auto failed = [&](int rc, ffs_ctx* c) {
        if (rc == FFS_OK) return false;
        std::printf("Error: --index-basis: %s\n", ffs_last_error(c));
        return true;
    };
    double dmin = args.index_dmin, b_iso = 0.0;
    if (failed(ffs_index_rlp(&g, xyz.data(), n, rlp.data(), s1.data(), mm.data()), nullptr)) return false;
    if (failed(ffs_index_defaults(rlp.data(), n, args.index_max_cell, args.fft_npoints, &dmin, &b_iso), nullptr)) return false;
    float grid_ms = 0.0f, peaks_ms = 0.0f;
    if (failed(ffs_ctx_index_grid(ctx, rlp.data(), n, dmin, b_iso, args.fft_npoints, nullptr, nullptr, &grid_ms), ctx)) return false;
    uint32_t n_peaks = 0, n_vectors = 0;
    int rc = ffs_ctx_index_peaks(ctx, 15.0, nullptr, 0, &n_peaks, nullptr, nullptr);
    if (rc != FFS_ERR_OVERFLOW && failed(rc, ctx)) return false;
    std::vector<ffs_index_peak> peaks(n_peaks);
    ffs_index_grid_stats st{};
    if (failed(ffs_ctx_index_peaks(ctx, 15.0, peaks.data(), n_peaks, &n_peaks, &st, &peaks_ms), ctx)) return false;
    std::vector<ffs_index_vector> vectors(n_peaks);
    if (failed(ffs_index_basis_vectors(peaks.data(), n_peaks, args.fft_npoints, dmin, 0.15, 3.0, args.index_max_cell, vectors.data(), n_peaks, &n_vectors), nullptr)) return false;
    vectors.resize(n_vectors);
    try {
        write_raw_file(args.index_basis + ".centres", xyz.data(), xyz.size() * sizeof(double));
        write_raw_file(args.index_basis + ".peaks", peaks.data(), peaks.size() * sizeof(ffs_index_peak));
        write_raw_file(args.index_basis + ".basis_vectors", vectors.data(), vectors.size() * sizeof(ffs_index_vector));
    } catch (const std::exception& e) {
        std::printf("Error: --index-basis: %s\n", e.what());
        return false;
    }
    std::printf("Index: %u spots, dmin %.5f, b_iso %.3f, grid of %u points a side, %u voxels selected, %u peaks (%.3f + %.3f ms on the GPU; one GPU)\n", n, dmin, b_iso,
                args.fft_npoints, st.n_selected, n_peaks, (double)grid_ms, (double)peaks_ms);
    std::printf("Index geometry: distance=%.17g beam_x=%.17g beam_y=%.17g pixel_x=%.17g pixel_y=%.17g wavelength=%.17g osc_start=%.17g osc_width=%.17g\n",
                kg.distance_mm, kg.beam_center_x_px, kg.beam_center_y_px, kg.pixel_size_x_mm, kg.pixel_size_y_mm, kg.wavelength, kg.oscillation_start, kg.oscillation_width);
    std::printf("%s", index_vector_lines(vectors.data(), vectors.size()).c_str());
    if (args.index_assign.empty()) return true;
    // --index-assign PREFIX: the candidate settings against the centres (host/index_assign.hpp has the step; `ffs_hosttool indexassign` on
    // PREFIX.centres and the vectors or settings file writes the same bytes)
    try {
        std::vector<ffs_index_setting> settings;
        if (!args.index_settings.empty()) {
            settings = read_settings_file(args.index_settings);
        } else {
            std::vector<double> v(3 * vectors.size());
            for (size_t k = 0; k < vectors.size(); ++k) v[3 * k] = vectors[k].v[0], v[3 * k + 1] = vectors[k].v[1], v[3 * k + 2] = vectors[k].v[2];
            uint32_t n_settings = 0;
            rc = ffs_index_settings(v.data(), (uint32_t)vectors.size(), 1000, nullptr, 0, &n_settings);
            if (rc != FFS_ERR_OVERFLOW && rc != FFS_OK) throw std::runtime_error(ffs_last_error(nullptr));
            settings.resize(n_settings);
            if (ffs_index_settings(v.data(), (uint32_t)vectors.size(), 1000, settings.data(), n_settings, &n_settings) != FFS_OK) throw std::runtime_error(ffs_last_error(nullptr));
        }
        std::vector<double> phi(n);
        for (uint32_t i = 0; i < n; ++i) phi[i] = mm[3 * (size_t)i + 2];
        IndexAssignOps ops;
        ops.assign = [&](const double* A, uint32_t m, ffs_index_assignment* out, int32_t* hkl) {
            if (ffs_ctx_index_assign(ctx, rlp.data(), phi.data(), nullptr, n, A, m, args.index_tolerance, 0, out, hkl, nullptr) != FFS_OK) throw std::runtime_error(ffs_last_error(ctx));
        };
        ops.detect = [](const ffs_index_assignment& r) {
            int32_t t = -1;
            if (ffs_index_absence_detect(&r, 0.9, &t) != FFS_OK) throw std::runtime_error(ffs_last_error(nullptr));
            return t;
        };
        ops.reindex = [](const double* A, int32_t t, double* out) { return ffs_index_reindex(A, t, out) == FFS_OK; };
        std::printf("%s", index_assign_run(ops, settings, n, args.index_assign).c_str());
    } catch (const std::exception& e) {
        std::printf("Error: --index-assign: %s\n", e.what());
        return false;
    }
    return true;
}

// 3D connected components (spotfinder.cc:1099-1148), spot variances for integration (:1152-1215), results_ffs.h5 (:1217-1262)
static bool finish_3d(const Args& args, ffs_ctx* ctx, ffs_stack3d* stack, const ffs_params& prm, const Experiment& ex, Clock::time_point t_joined) {
    std::printf("Processing 3D spots\n");
    const ffs_reflection* refl = nullptr;
    uint32_t n = 0, n_calc = 0, f_size = 0, f_sep = 0;
    FFS_CHECK(ctx, ffs_stack3d_finish(stack, &refl, &n, &n_calc, &f_size, &f_sep));
    if (args.verbose) std::printf("3D finish: %.1f ms\n", ms_between(t_joined, Clock::now()));
    std::printf("Calculated %u spots\n", n_calc);  // connected_components.cc:453-454
    if (f_size > 0) std::printf("Filtered %u spots with size < %u pixels\n", f_size, prm.min_spot_size_3d);
    if (f_sep > 0) std::printf("Filtered %u spots with peak-centroid distance > %s\n", f_sep, fmt_num(prm.max_peak_centroid_separation).c_str());
    std::printf("Found %u spots\n", n);
    if (args.writeout) {
        std::ofstream out("3d_reflections.txt");
        for (uint32_t i = 0; i < n; ++i) {
            const ffs_reflection& r = refl[i];
            out << "X: [" << r.x_min << ", " << r.x_max << "] "
                << "Y: [" << r.y_min << ", " << r.y_max << "] "
                << "Z: [" << r.z_min << ", " << r.z_max << "] "
                << "COM: (" << r.com_x << ", " << r.com_y << ", " << r.com_z << ")\n";
        }
    }
    const uint32_t *sx, *sy, *si;
    const int32_t *sz, *sr;
    uint64_t n_sig = 0;
    FFS_CHECK(ctx, ffs_stack3d_signals(stack, &sx, &sy, &sz, &si, &sr, &n_sig));
    const DetectorGeometry& detector = ex.detector;
    const KabschGeometry geom{detector.distance * 1000.0, detector.beam_center_x, detector.beam_center_y,
                              detector.pixel_size_x * 1000.0, detector.pixel_size_y * 1000.0, ex.wavelength,
                              ex.oscillation_start, ex.oscillation_width};
    const KabschVariances kv = kabsch_variances(geom, refl, n, sx, sy, sz, si, sr, n_sig);
    if (n) std::printf("Estimated sigma_b (degrees): %.6f\n", kv.est_sigma_b_deg);
    if (kv.n_sigma_m)
        std::printf("Estimated sigma_m (degrees): %.6f, calculated on %d spots\n", kv.est_sigma_m_deg, kv.n_sigma_m);
    if (args.save_h5) {
        try {
            std::vector<double> flat;
            for (uint32_t i = 0; i < n; ++i) {
                flat.push_back(refl[i].com_x);
                flat.push_back(refl[i].com_y);
                flat.push_back(refl[i].com_z);
            }
            const std::vector<int> id(n, 0);
            h5_write_reflection_table("results_ffs.h5", "dials/processing/group_0", flat, id, &kv.sigma_b_variance,
                                      &kv.sigma_m_variance, &kv.bbox_depth);
            std::printf("Successfully wrote 3D reflections to HDF5 file\n");
        } catch (const std::exception& e) {
            std::printf("Error writing data to HDF5 file: %s\n", e.what());
        }
    }
    if (args.verbose) std::printf("3D analysis in all: %.1f ms\n", ms_between(t_joined, Clock::now()));
    std::printf("3D spot analysis complete\n");
    const bool ok = args.index_basis.empty() || index_basis(args, ctx, geom, refl, n);
    ffs_stack3d_destroy(stack);
    return ok;
}

// stills with -h5: every image's centres into results_ffs.h5, one experiment id per image (spotfinder.cc:1265-1306)
static void write_2d_h5(const std::map<uint32_t, std::vector<float>>& reflection_centers_2d) {
    std::printf("Processing 2D spots\n");
    try {
        std::vector<double> flat;
        std::vector<int> ids;
        int id = 0;
        for (const auto& kv : reflection_centers_2d) {  // std::map: ascending image number
            for (float v : kv.second) flat.push_back((double)v);
            ids.insert(ids.end(), kv.second.size() / 3, id);
            ++id;
        }
        h5_write_reflection_table("results_ffs.h5", "dials/processing/group_0", flat, ids, nullptr, nullptr, nullptr);
        std::printf("Successfully wrote %zu 2D reflections to HDF5 file\n", ids.size());
    } catch (const std::exception& e) {
        std::printf("Error writing data to HDF5 file: %s\n", e.what());
    }
    std::printf("2D spot analysis complete\n");
}

// the totals (spotfinder.cc:1308-1329)
static void print_summary(const Args& args, const FrameShape& shape, const BatchPipeline& pipeline, const BatchReport& report, const GatherRound* gather,
                          uint32_t n_dev, Clock::time_point all_start, Clock::time_point process_start) {
    const double total = std::chrono::duration<double>(Clock::now() - all_start).count();
    const uint32_t done = pipeline.images_completed();
    std::printf("\n%d images in %.2f s (\033[1;34m%.2f GBps\033[0m) (\033[1;34m%.1f fps\033[0m)\n", (int)done, total,
                (double)shape.width * shape.height * shape.bytes_per_pixel * done / total / 1e9, done / total);
    if (args.verbose) {   // CPU seconds against wall seconds: under a cgroup CPU quota, threads beyond it stall everyone
        struct rusage ru{};
        getrusage(RUSAGE_SELF, &ru);
        const double user = ru.ru_utime.tv_sec + ru.ru_utime.tv_usec * 1e-6, sys = ru.ru_stime.tv_sec + ru.ru_stime.tv_usec * 1e-6;
        const double since_launch = std::chrono::duration<double>(Clock::now() - process_start).count();
        std::printf("CPU time of the process: %.2f s user + %.2f s system over %.2f s since launch (%.1f cores busy on average)\n", user, sys,
                    since_launch, (user + sys) / since_launch);
    }
    if (gather)
        std::printf("Spot lists: %llu rounds of %u batches gathered over RCCL, %llu batch results read from the host arrays\n",
                    (unsigned long long)gather->rccl_rounds.load(), n_dev, (unsigned long long)gather->host_rounds.load());
    if (args.validate)
        std::printf("Validation: %u of %u images differ between the hot path and the gather path\n", report.validate_mismatches.load(), done);
    const double time_waiting = pipeline.seconds_waiting_for_images();
    if (time_waiting < 10) std::printf("Total time waiting for images to appear: %.0f ms\n", time_waiting * 1000);
    else std::printf("Total time waiting for images to appear: %.2f s\n", time_waiting);
}

int main(int argc, char** argv) {
    Stamps stamp(Clock::now());
    std::printf("Spotfinder version: %s\n", FFS_VERSION);
    Args args = parse_args(argc, argv);
    stamp.verbose = args.verbose;
    if (args.spot_background_glm) std::printf("Spot background model: glm (robust Poisson GLM of the ring of %u pixels)\n", args.spot_background);
    std::printf("Algorithm: %s\n", args.algo == FFS_ALGO_DISPERSION_EXTENDED ? "Dispersion Extended" : args.algo == FFS_ALGO_RADIAL_PROFILE ? "Radial Profile" : "Dispersion");
    if (args.threads < 1) {
        std::printf("Error: Thread count must be >= 1\n");
        return 1;
    }
    std::unique_ptr<Reader> reader_ptr;
    std::vector<float> gain_map;   // --gain-map: width x height values, checked; empty: none
    std::vector<float> jungfrau_planes;   // --jungfrau-calibration: 6 x width x height values; empty: the frames are photon counts
    if (const int rc = open_source_beside_runtime(args, stamp, reader_ptr, gain_map, jungfrau_planes)) return rc;
    Reader& reader = *reader_ptr;
    // --jungfrau-pedestal: the source is a dark run; it is folded into pedestal statistics and no spots are found (pedestal_mode.cc)
    if (!args.jungfrau_pedestal.empty()) return run_jungfrau_pedestal(args, reader, jungfrau_planes);
    const bool jungfrau = !jungfrau_planes.empty();

    // (raw Jungfrau words are 16 bits in the source and 32-bit photon counts from the conversion on: the flag decides, not the source's type)
    FrameShape shape;
    shape.bytes_per_pixel = jungfrau ? 4 : reader.get_element_size();
    if (const int rc = check_dtype(args, argv[0], shape.bytes_per_pixel)) return rc;
    const uint32_t num_images = args.images_set ? args.images : (uint32_t)reader.get_number_of_images();
    shape.height = (uint32_t)reader.image_shape()[0];
    shape.width = (uint32_t)reader.image_shape()[1];
    int64_t max_valid = max_valid_pixel(args.max_valid, reader, shape.bytes_per_pixel);
    // (converted frames mark saturated and uncalibrated pixels 0xFFFFFFFF: with a max_valid of at most 2^24 - 1 such a centre is never strong)
    if (jungfrau && args.max_valid == "trusted") max_valid = max_valid < 0 ? (1ll << 24) - 1 : std::min<int64_t>(max_valid, (1ll << 24) - 1);
    Experiment ex;
    if (const int rc = read_experiment(args, reader, ex)) return rc;
    const bool rotation = ex.oscillation_width > 0;

    std::signal(SIGINT, stop_processing);
    stamp("frame source opened, header read");

    // ---- device contexts -----------------------------------------------------------------------------
    // bitshuffle-LZ4 chunks and CBF byte-offset sections go to the GPU as they are (read straight into the pinned staging area)
    // unless the pixels are needed on the host (--writeout) or --cpu-decode asks for the reference's way
    const bool byte_offset = reader.get_raw_chunk_compression() == Reader::BYTE_OFFSET_32;
    // ... and so do raw Jungfrau words (--jungfrau-calibration), converted there
    const bool gpu_decode = (reader.get_raw_chunk_compression() == Reader::BITSHUFFLE_LZ4 || byte_offset || jungfrau) && !args.cpu_decode && !args.writeout;
    const uint32_t n_dev_arg = (uint32_t)std::max<size_t>(1, args.devices.size());
    const uint32_t batch = args.batch ? args.batch : default_batch(gpu_decode, num_images, n_dev_arg);
    std::printf("Image:       %4u x %4u = %u px\n", shape.width, shape.height, shape.width * shape.height);
    std::printf("GPU batches: %u frames per submit, filled by all readers of a GPU; %s\n", batch,
                args.single_buffer ? "one batch in flight" : (gpu_decode ? "four batches in flight per GPU" : "three batches in flight per GPU"));
    std::printf("Running with %u CPU threads\n", args.threads);

    // One context per GPU (the reference has one device, -d: src/ffs/cuda_arg_parser.cc:30-61).  With
    // --devices / --gpus the one frame queue feeds the reader threads of all of them.
    const std::vector<int> devices = args.devices.empty() ? std::vector<int>{args.device} : args.devices;
    const int have = ffs_device_count();
    for (int d : devices)
        if (d < 0 || d >= have) {
            std::printf("Error: device %d does not exist (%d visible)\n", d, have);
            return 1;
        }
    const uint32_t n_dev = (uint32_t)devices.size();
    if (args.threads < n_dev) args.threads = n_dev;  // at least one worker per GPU
    const bool gather_rccl = n_dev > 1 && args.gather == "rccl" && args.output_for_index && !rotation;
    Exchange exchange;
    if (n_dev > 1) {
        std::string list;
        for (int d : devices) list += (list.empty() ? "" : ", ") + std::to_string(d);
        if (rotation || gather_rccl) exchange.start(devices, gather_rccl);
        const char* env = std::getenv("FFS_GATHER");
        std::printf("GPUs:        %s (frame queue shared; exchange of rotation lists: %s)\n", list.c_str(),
                    rotation ? (env ? env : "rccl") : "none needed (stills)");
        if (gather_rccl) std::printf("Spot lists:  gathered over RCCL to GPU %d, one round of batches (one per GPU) at a time\n", devices[0]);
        stamp("exchange between GPUs set going");
    }
    std::vector<ffs_ctx*> ctxs(n_dev, nullptr), vctxs(n_dev, nullptr);
    for (uint32_t di = 0; di < n_dev; ++di) {
        if (!create_context(devices[di], shape, batch, &ctxs[di])) return 1;
        stamp("ffs_ctx_create (code object, mask tables, shared HIP streams)");
    }
    ffs_ctx* ctx = ctxs[0];  // owns the 3D stack; also the context the one-off steps below report from
    upload_masks(ctxs, reader, args, ex, shape);
    const ffs_params prm = make_params(args, rotation, max_valid);
    // (-a radial_profile is refused while the context has no bin map: the parameters go in with the default algorithm here and again, as they
    // are, behind the map below)
    const bool radial_algo = args.algo == FFS_ALGO_RADIAL_PROFILE;
    ffs_params prm_before_map = prm;
    if (radial_algo) prm_before_map.algorithm = FFS_ALGO_DISPERSION;
    for (ffs_ctx* cx : ctxs) {
        FFS_CHECK(cx, ffs_ctx_set_params(cx, &prm_before_map));
        FFS_CHECK(cx, ffs_ctx_set_max_valid_scope(cx, args.max_valid_scope));
        FFS_CHECK(cx, ffs_ctx_set_gain(cx, args.gain));
        if (!gain_map.empty()) FFS_CHECK(cx, ffs_ctx_set_gain_map(cx, gain_map.data()));
        if (jungfrau) FFS_CHECK(cx, set_jungfrau_calibration(cx, jungfrau_planes, shape.pixels()));
    }
    if (jungfrau)
        std::printf("Jungfrau calibration: %s (raw 16-bit words -> photon counts %s; saturated and uncalibrated pixels are masked for their frame)\n",
                    args.jungfrau_calibration.c_str(), gpu_decode ? "on the GPU" : "on the worker threads");
    if (max_valid >= 0 && args.max_valid_scope == FFS_MAX_VALID_WINDOW)
        std::printf("Trusted range: pixels above %lld are masked for their frame (window scope: out of every window's sums, and not spots)\n", (long long)max_valid);
    else if (max_valid >= 0) std::printf("Trusted range: centre pixels above %lld are not spots\n", (long long)max_valid);
    if (args.gain > 0.0) std::printf("Detector gain: %g (a background window's variance is taken as gain x mean)\n", args.gain);
    if (!gain_map.empty())
        std::printf("Detector gain map: %s (%g .. %g)\n", args.gain_map.c_str(), (double)*std::min_element(gain_map.begin(), gain_map.end()),
                    (double)*std::max_element(gain_map.begin(), gain_map.end()));
    if (args.radial_bins) {
        // N shells of equal width in 1/d^2, built here in float64 (radial_bins.hpp); the library only counts into them
        const DetectorGeometry& d = ex.detector;
        const RadialBins shells = radial_bins(RadialGeometry{ex.wavelength, d.distance, d.beam_center_x, d.beam_center_y, d.pixel_size_x, d.pixel_size_y},
                                              shape.width, shape.height, args.radial_bins);
        for (ffs_ctx* cx : ctxs) FFS_CHECK(cx, ffs_ctx_set_radial_bins(cx, shells.bin_of_pixel.data(), shells.n_bins));
        std::string edges;
        for (uint32_t k = 0; k <= shells.n_bins; ++k) {
            char buf[32];
            std::snprintf(buf, sizeof buf, k == 0 ? "inf" : " %.4g", shells.d_edge(k));
            edges += buf;
        }
        std::printf("Radial bins: %u shells, d edges (A): %s\n", shells.n_bins, edges.c_str());
    }
    if (radial_algo) {
        for (ffs_ctx* cx : ctxs) {
            FFS_CHECK(cx, ffs_ctx_set_radial_threshold(cx, args.n_iqr));
            FFS_CHECK(cx, ffs_ctx_set_radial_blur(cx, args.radial_blur));
            FFS_CHECK(cx, ffs_ctx_set_params(cx, &prm));
        }
        std::printf("Radial-profile threshold: a strong pixel stands above median + %g x IQR of its shell\n", args.n_iqr);
        if (args.radial_blur)
            std::printf("Radial blur: %s, a %d x %d kernel over the valid pixels ahead of the threshold\n", args.radial_blur == FFS_RADIAL_BLUR_NARROW ? "narrow" : "wide",
                        2 * args.radial_blur + 1, 2 * args.radial_blur + 1);
    }
    // --pixel-stats: every context accumulates from its first batch on (the validation contexts see the same frames again, and do not)
    if (!args.pixel_stats.empty())
        for (ffs_ctx* cx : ctxs) FFS_CHECK(cx, ffs_ctx_set_pixel_stats(cx, FFS_PIXEL_STATS_START));
    size_t n_shoeboxes = 0;
    if (!args.integrate.empty())
        if (const int rc = open_integration(args, ex, rotation, ctxs, n_shoeboxes)) return rc;
    if (!args.index_basis.empty() && !rotation) {
        std::printf("Error: --index-basis needs a rotation source (an oscillation width above 0): the spots of stills have no rotation angle\n");
        return 1;
    }
    if (!args.predict.empty())
        if (const int rc = open_prediction(args, ex, rotation, num_images, (int)shape.width, (int)shape.height, ctxs, n_shoeboxes)) return rc;
    if (args.validate && !create_validation_contexts(devices, ctxs, shape, batch, prm, args.max_valid_scope, args.gain, gain_map, vctxs)) return 1;
    if (args.validate && jungfrau && gpu_decode)   // (the validation streams are handed the same raw chunks)
        for (ffs_ctx* v : vctxs) FFS_CHECK(v, set_jungfrau_calibration(v, jungfrau_planes, shape.pixels()));
    if (args.save_h5 && !h5_supported()) {
        std::printf("Error: --save-h5 needs an HDF5-enabled build\n");
        return 1;
    }

    std::printf("Dataset type: %s\n", rotation ? "Rotation set" : "Still set");
    ffs_stack3d* stack = nullptr;
    if (rotation) FFS_CHECK(ctx, ffs_stack3d_create(ctx, 0, &stack));

    std::unique_ptr<PipeHandler> pipe;
    if (args.pipe_fd != -1) pipe = std::make_unique<PipeHandler>(args.pipe_fd);
    stamp("masks uploaded, parameters set: the timed loop starts");

    // ---- the run: batches assembled by the readers, reported by the collectors (batch_pipeline.hpp) ---------------------------------
    const auto all_start = Clock::now();
    PipelineConfig cfg;
    cfg.batch = batch;
    cfg.assemblies = args.single_buffer ? 1u : args.assemblies ? std::min(args.assemblies, 32u) : (gpu_decode ? 4u : 3u);
    cfg.gpu_decode = gpu_decode;
    cfg.codec = jungfrau ? FFS_CODEC_JUNGFRAU_RAW : byte_offset ? FFS_CODEC_BYTE_OFFSET : FFS_CODEC_BSLZ4;
    cfg.jungfrau_planes = jungfrau ? jungfrau_planes.data() : nullptr;
    cfg.read_only = args.read_only;
    cfg.verbose = args.verbose;
    cfg.timeout = args.timeout;
    cfg.slot_margin = args.slot_margin;
    cfg.start_index = args.start_index;
    cfg.num_images = num_images;
    cfg.width = shape.width;
    cfg.height = shape.height;
    cfg.bytes_per_pixel = shape.bytes_per_pixel;
    cfg.start = all_start;
    const auto node_cpus = args.no_numa_pinning ? std::vector<std::optional<cpu_set_t>>(n_dev) : numa_cpu_sets(devices, args.verbose);
    for (uint32_t di = 0; di < n_dev; ++di) cfg.gpus.push_back({ctxs[di], args.validate ? vctxs[di] : nullptr, devices[di], node_cpus[di]});
    cfg.readers = reader_count(args, gpu_decode, n_dev);
    BatchPipeline pipeline(cfg, reader, g_stop);
    std::unique_ptr<GatherRound> gather;
    if (gather_rccl) gather = std::make_unique<GatherRound>(devices, pipeline, exchange);
    BatchReport report(args, prm, shape, rotation, ctxs, stack, exchange, gather.get(), pipe.get(), pipeline.print_mutex());
    if (!pipeline.run(std::ref(report))) return 1;

    // ---- post-processing and the totals ------------------------------------------------------------------------------------------
    const auto t_joined = Clock::now();
    if (args.verbose) std::printf("Workers joined %.0f ms after the start\n", ms_between(all_start, t_joined));
    bool finished = true;
    if (rotation) finished = finish_3d(args, ctx, stack, prm, ex, t_joined);
    else if (args.save_h5) write_2d_h5(report.reflection_centers_2d);
    print_summary(args, shape, pipeline, report, gather.get(), n_dev, all_start, stamp.process_start());
    if (!args.pixel_stats.empty() && !write_pixel_stats(args.pixel_stats, ctxs, shape.width, shape.height)) return 1;
    if (args.integrating() && !write_integration(args, ctxs, n_shoeboxes)) return 1;
    if (!finished) return 1;   // (--index-basis has said why)
    pipe.reset();
    exchange.join();
    stamp("timed loop and reports done");
    const int exit_code = (args.validate && report.validate_mismatches.load()) ? 1 : 0;
    if (!args.clean_exit) {
        // Every result is out and nothing is in flight: the process ends here.  Destroying streams and contexts (35-90 ms: pinned
        // staging areas are unregistered, device memory freed) and the runtime's own exit handlers (~100 ms) do nothing a dying
        // process needs -- the kernel driver releases the GPU's resources -- and the service starts one process per request
        // (service.py:497): they were a fifth of a 1000-image request's wall time.  --clean-exit keeps the full teardown.
        std::fflush(stdout);
        std::fflush(stderr);
        std::_Exit(exit_code);
    }
    for (ffs_stream* st : pipeline.streams_to_retire()) ffs_stream_destroy(st);
    stamp("streams destroyed");
    for (ffs_ctx* cx : ctxs) ffs_ctx_destroy(cx);
    for (ffs_ctx* cx : vctxs) if (cx) ffs_ctx_destroy(cx);
    stamp("contexts destroyed: main returns (the runtime's own exit handlers follow)");
    std::fflush(stdout);
    return exit_code;
}
