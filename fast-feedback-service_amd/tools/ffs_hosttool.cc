// ffs_hosttool -- host-side helper for tests and demos (no GPU):
//   ffs_hosttool selftest                 round-trip / known-answer checks of host/codecs.hpp
//   ffs_hosttool mkshm <synth:spec> <dir> write an Eiger-stream style directory the SHM reader takes
//                                         (start_1 JSON header, start_4, start_5 int32 mask,
//                                         image_%06d_2 bitshuffle-LZ4 chunks; spotfinder/shmread.cc)
//   ffs_hosttool mkcbf <synth:spec> <prefix>  write <prefix>0001.cbf ... (miniCBF, byte-offset codec)
//   ffs_hosttool mkh5 <synth:spec> <master.h5> [layout [frames_per_file [n_written]]]
//                                         NXmx master + data files (host/h5_writer.cc)
//   ffs_hosttool h5info <master.h5>       what the HDF5 reader sees; synthinfo prints the same checksums
//   ffs_hosttool jfcal <synth:spec> <file>    the calibration of a synthetic source of raw Jungfrau words, as spotfinder's
//                                         --jungfrau-calibration reads it (6 W H float32: pedestal G0 G1 G2, factor G0 G1 G2)
//   ffs_hosttool jfconvert <raw> <cal> <W> <H> <out>   the host converter of codecs.hpp: frames of W H raw words -> uint32 photon counts
//   ffs_hosttool synthframes <synth:spec> <file>        the source's frames as it hands them over, one behind the other
//   ffs_hosttool jfrepedestal <old cal> <prefix> <new cal> [min_frames [max_rms]]
//                                         the re-pedestalled calibration from spotfinder --jungfrau-pedestal's <prefix>.count.u32, .sum.u64 and
//                                         .sum_sq.u64 (the rule of csrc/jungfrau_pedestal_model.hpp): pedestals replaced, a factor kept where the
//                                         stage's pedestal is usable (count >= min_frames [1], rms <= max_rms [0: no test]) and 0 elsewhere
//   ffs_hosttool spotbgglm [file]         the robust Poisson GLM background (csrc/spot_background_glm_model.hpp, the text the kernel of
//                                         ffs_stream_spot_backgrounds_glm compiles) of histograms read from the file or standard input, 257
//                                         unsigned integers a line (the bins 0 .. 255, then the tail): one record a line, n_pixels n_overflow
//                                         median n_iter status beta mean, the two doubles as the 16 hex digits of their bit patterns
//   ffs_hosttool shoebox key=value ...   summation integration on the CPU by csrc/shoebox_model.hpp, the text the kernel of
//                                         ffs_stream_shoebox_fold compiles: frames=<file of images, one behind the other> width= height=
//                                         bytes=2|4 [mask=<W*H bytes, non-zero = valid>] [max_valid=N] distance= beam_x= beam_y= pixel_x=
//                                         pixel_y= wavelength= osc_start= osc_width= boxes=<the file spotfinder --integrate reads> (or
//                                         predictions=<a PREFIX.predictions file>: the boxes not flagged FFS_PREDICT_BOX_REFUSED, s1 and phi as recorded) sigma_b=
//                                         sigma_m= [n_sigma=3] [algorithm=ellipsoid|dials] [background=tukey|glm] out=<file>: writes the
//                                         ffs_shoebox_sum records spotfinder writes to PREFIX.shoebox_sums and prints its summary line
//   ffs_hosttool shoeboxgeom key=value ...  the geometry keys and boxes= of the above: the ffs_scan_geometry (20 doubles) and every box's
//                                         s1 and phi as host/shoebox_geometry.hpp computes them, 16 hex digits a double
//   ffs_hosttool predict key=value ...   scan prediction on the CPU by csrc/predict_model.hpp, the text the kernels of ffs_ctx_predict compile:
//                                         the geometry keys of the above, width= height= crystal=<nine float64> n_images= dmin= sigma_b= sigma_m=
//                                         [n_sigma=3] [centring=P|I|F|A|B|C|R] out=<file>: writes the ffs_prediction records spotfinder --predict
//                                         writes to PREFIX.predictions and prints its summary line
//   ffs_hosttool indexassign key=value ... index assignment for candidate settings on the CPU by csrc/assign_model.hpp, the text the kernels of
//                                   ffs_ctx_index_assign compile: the twin of `spotfinder --index-assign` (host/index_assign.hpp)
//   ffs_hosttool indexbasis key=value ... the indexer's basis-vector search on the CPU by csrc/index_model.hpp, the text the kernels of
//                                         ffs_ctx_index_grid / index_peaks compile (the twin of spotfinder --index-basis): the geometry keys of
//                                         the above, centres=<n x 3 float64: x_px, y_px, z> max-cell= [dmin=] [npoints=256] out=<PREFIX>:
//                                         writes PREFIX.peaks (ffs_index_peak), PREFIX.basis_vectors (ffs_index_vector) and PREFIX.grid_sha256
//                                         (the digest of the power grid's bytes) and prints the candidate vectors as the reference logs them
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <random>

#include <map>

#include "../csrc/assign_model.hpp"
#include "../csrc/assign_plan.hpp"
#include "../csrc/index_model.hpp"
#include "../csrc/index_plan.hpp"
#include "../csrc/launch_geometry.hpp"
#include "../csrc/predict_model.hpp"
#include "../csrc/predict_plan.hpp"
#include "../csrc/shoebox_model.hpp"
#include "../csrc/shoebox_plan.hpp"
#include "../csrc/spot_background_glm_model.hpp"
#include "shoebox_geometry.hpp"
#include "predict_geometry.hpp"
#include "index_basis.hpp"
#include "index_assign.hpp"
#include "codecs.hpp"
#include "reader.hpp"

using namespace ffshost;

static int fail(const char* what) {
    std::printf("FAIL: %s\n", what);
    return 1;
}

static int selftest() {
    // LZ4 known answer: "aaaaaaaaaaaaaaaaaaaa" (20 x 'a') = token 0x1B? build by hand:
    // literals "a" (1), match offset 1 length 14+4... use a hand-assembled block instead:
    //   token 0x1F: 1 literal, match len 15+ext ; literal 'a'; offset 0x0001; ext 0 -> match 19 bytes
    {
        const uint8_t blk[] = {0x1F, 'a', 0x01, 0x00, 0x00, 0x50, 'b', 'c', 'd', 'e', 'f'};
        uint8_t out[64] = {0};
        const long n = lz4_block_decompress(blk, sizeof blk, out, sizeof out);
        if (n != 25 || std::memcmp(out, "aaaaaaaaaaaaaaaaaaaabcdef", 25) != 0) return fail("lz4 known answer");
    }
    std::mt19937_64 rng(12345);
    for (int round = 0; round < 40; ++round) {
        const size_t n = 1 + rng() % 70000;
        std::vector<uint8_t> data(n);
        const int mode = round % 4;
        for (size_t i = 0; i < n; ++i)
            data[i] = mode == 0 ? (uint8_t)rng() : mode == 1 ? (uint8_t)(i / 97) : mode == 2 ? (uint8_t)((rng() % 50) == 0) : 0;
        auto c = lz4_block_compress(data.data(), n);
        std::vector<uint8_t> back(n + 8);
        if (lz4_block_decompress(c.data(), c.size(), back.data(), n) != (long)n || std::memcmp(back.data(), data.data(), n))
            return fail("lz4 round trip");
    }
    for (size_t es : {2u, 4u})
        for (size_t nelem : {8u, 24u, 4096u, 4097u, 10007u, 70001u}) {
            std::vector<uint8_t> data(nelem * es);
            for (size_t i = 0; i < nelem; ++i) {
                const uint32_t v = (rng() % 100 == 0) ? (uint32_t)rng() : (uint32_t)(rng() % 7);
                std::memcpy(&data[i * es], &v, es);
            }
            if (nelem % 8 == 0) {
                std::vector<uint8_t> sh(nelem * es), un(nelem * es);
                bitshuffle_block(data.data(), sh.data(), nelem, es);
                bitunshuffle_block(sh.data(), un.data(), nelem, es);
                if (un != data) return fail("bitshuffle round trip");
                // plane 0 holds the LSBs: element i at byte i/8, bit i%8
                for (size_t i = 0; i < nelem; ++i)
                    if (((sh[i / 8] >> (i % 8)) & 1) != (data[i * es] & 1)) return fail("bit-plane layout");
            }
            auto c = bshuf_compress_lz4_with_header(data.data(), nelem, es);
            std::vector<uint8_t> back(nelem * es);
            if (bshuf_decompress_lz4(c.data() + 12, c.size() - 12, back.data(), nelem, es) < 0 || back != data)
                return fail("bitshuffle-lz4 round trip");
            uint64_t total = 0;
            for (int i = 0; i < 8; ++i) total = (total << 8) | c[i];
            if (total != nelem * es) return fail("bitshuffle header");
        }
    {
        std::vector<int32_t> v(5000);
        for (auto& x : v) {
            const int m = (int)(rng() % 20);
            x = m == 0 ? (int32_t)(rng() % 100000) - 20000 : m == 1 ? -1 : (int32_t)(rng() % 12);
        }
        auto c = byte_offset_compress(v.data(), v.size());
        std::vector<int32_t> back(v.size());
        if (byte_offset_decompress(c.data(), c.size(), back.data(), back.size()) != v.size() || back != v)
            return fail("byte-offset round trip");
        // known answer: deltas 1, 300 (escape to 16 bit), -70000 (escape to 32 bit)
        const uint8_t ka[] = {0x01, 0x80, 0x2C, 0x01, 0x80, 0x00, 0x80, 0x90, 0xEE, 0xFE, 0xFF};
        int32_t o[3];
        if (byte_offset_decompress(ka, sizeof ka, o, 3) != 3 || o[0] != 1 || o[1] != 301 || o[2] != 301 - 70000)
            return fail("byte-offset known answer");
    }
    std::printf("codecs selftest ok\n");
    return 0;
}

static int mkshm(const std::string& spec, const std::string& dir) {
    auto r = make_synth_reader(spec);
    std::filesystem::create_directories(dir);
    const size_t H = r->image_shape()[0], W = r->image_shape()[1], es = r->get_element_size();
    {
        std::ofstream f(dir + "/start_1");
        f << "{\"nimages\": " << r->get_number_of_images() << ", \"ntrigger\": 1, \"y_pixels_in_detector\": " << H
          << ", \"x_pixels_in_detector\": " << W << ", \"bit_depth_image\": " << es * 8
          << ", \"countrate_correction_count_cutoff\": " << r->get_trusted_range()[1] << ", \"wavelength\": 0.976"
          << ", \"detector_distance\": 300.0, \"y_pixel_size\": 7.5e-05, \"x_pixel_size\": 7.5e-05"
          << ", \"beam_center_y\": " << H / 2.0 << ", \"beam_center_x\": " << W / 2.0;
        if (r->get_oscillation()[1] > 0) f << ", \"omega_start\": 0.0, \"omega_increment\": " << r->get_oscillation()[1];
        f << "}\n";
    }
    { std::ofstream f(dir + "/start_4"); f << "\n"; }
    {
        std::vector<int32_t> m(W * H);
        auto mask = *r->get_mask();
        for (size_t i = 0; i < W * H; ++i) m[i] = mask[i] ? 0 : 1;  // pixel_mask: 0 = good
        std::ofstream f(dir + "/start_5", std::ios::binary);
        f.write(reinterpret_cast<const char*>(m.data()), (std::streamsize)(m.size() * 4));
    }
    std::vector<uint8_t> buf(W * H * es);
    for (size_t i = 0; i < r->get_number_of_images(); ++i) {
        r->get_raw_chunk(i, buf);
        auto c = bshuf_compress_lz4_with_header(buf.data(), W * H, es);
        char name[64];
        std::snprintf(name, sizeof name, "/image_%06zu_2", i);
        std::ofstream f(dir + name, std::ios::binary);
        f.write(reinterpret_cast<const char*>(c.data()), (std::streamsize)c.size());
    }
    return 0;
}

static int mkcbf(const std::string& spec, const std::string& prefix) {
    auto r = make_synth_reader(spec);
    const size_t H = r->image_shape()[0], W = r->image_shape()[1];
    if (r->get_element_size() != 2) return fail("mkcbf writes 16-bit sources only");
    std::vector<uint8_t> buf(W * H * 2);
    auto mask = *r->get_mask();
    for (size_t i = 0; i < r->get_number_of_images(); ++i) {
        r->get_raw_chunk(i, buf);
        std::vector<int32_t> v(W * H);
        for (size_t k = 0; k < W * H; ++k) v[k] = mask[k] ? reinterpret_cast<uint16_t*>(buf.data())[k] : -1;  // flagged = -1
        auto c = byte_offset_compress(v.data(), v.size());
        char name[32];
        std::snprintf(name, sizeof name, "%04zu.cbf", i + 1);
        std::ofstream f(prefix + name, std::ios::binary);
        f << "###CBF: VERSION 1.5\r\n\r\n_array_data.data\r\n;\r\n--CIF-BINARY-FORMAT-SECTION--\r\n"
          << "Content-Type: application/octet-stream;\r\n     conversions=\"x-CBF_BYTE_OFFSET\"\r\n"
          << "X-Binary-Size: " << c.size() << "\r\nX-Binary-Element-Type: \"signed 32-bit integer\"\r\n"
          << "X-Binary-Size-Fastest-Dimension: " << W << "\r\nX-Binary-Size-Second-Dimension: " << H << "\r\n\r\n"
          << "\x0c\x1a\x04\xd5";
        f.write(reinterpret_cast<const char*>(c.data()), (std::streamsize)c.size());
    }
    return 0;
}

// mkh5 <synth:spec> <master.h5> [layout [frames_per_file [n_written]]]
static int mkh5(int argc, char** argv) {
    auto r = make_synth_reader(argv[2]);
    const std::string layout = argc > 4 ? argv[4] : "vds-links";
    const size_t per_file = argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 0;
    const size_t n_written = argc > 6 ? std::strtoull(argv[6], nullptr, 10) : r->get_number_of_images();
    h5_write_nxmx(*r, argv[3], layout, per_file, n_written);
    return 0;
}

// h5info <master.h5>: what the H5 reader sees (metadata + per-frame availability and a pixel checksum)
static int h5info(const std::string& file) {
    auto r = make_h5_reader(file);
    const size_t H = r->image_shape()[0], W = r->image_shape()[1], es = r->get_element_size();
    std::printf("images %zu shape %zu %zu bytes %zu trusted %lld %lld\n", r->get_number_of_images(), H, W, es,
                (long long)r->get_trusted_range()[0], (long long)r->get_trusted_range()[1]);
    std::printf("wavelength %.6g distance %.6g pixel %.6g %.6g beam %.6g %.6g osc %.6g %.6g\n", *r->get_wavelength(),
                *r->get_detector_distance(), (*r->get_pixel_size())[0], (*r->get_pixel_size())[1],
                (*r->get_beam_center())[0], (*r->get_beam_center())[1], r->get_oscillation()[0], r->get_oscillation()[1]);
    if (auto m = r->get_mask()) {
        size_t valid = 0;
        for (auto v : *m) valid += v;
        std::printf("mask valid %zu\n", valid);
    } else {
        std::printf("mask none\n");
    }
    std::vector<uint8_t> chunk(W * H * es + 4096), px(W * H * es);
    for (size_t i = 0; i < r->get_number_of_images(); ++i) {
        if (!r->is_image_available(i)) {
            std::printf("frame %zu unavailable\n", i);
            continue;
        }
        auto c = r->get_raw_chunk(i, chunk);
        if (c.size() < 12 || bshuf_decompress_lz4(c.data() + 12, c.size() - 12, px.data(), W * H, es) < 0)
            return fail("chunk does not decode");
        uint64_t h = 1469598103934665603ull;  // FNV-1a over the pixel bytes
        for (auto b : px) h = (h ^ b) * 1099511628211ull;
        std::printf("frame %zu chunk %zu fnv %016llx\n", i, c.size(), (unsigned long long)h);
    }
    return 0;
}

// synthinfo <synth:spec>: the same per-frame checksums straight from the synthetic source
static int synthinfo(const std::string& spec) {
    auto r = make_synth_reader(spec);
    const size_t H = r->image_shape()[0], W = r->image_shape()[1], es = r->get_element_size();
    std::vector<uint8_t> px(W * H * es);
    for (size_t i = 0; i < r->get_number_of_images(); ++i) {
        r->get_raw_chunk(i, px);
        uint64_t h = 1469598103934665603ull;
        for (auto b : px) h = (h ^ b) * 1099511628211ull;
        std::printf("frame %zu fnv %016llx\n", i, (unsigned long long)h);
    }
    return 0;
}

static std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int jfcal(const std::string& spec, const std::string& file) {
    const std::vector<float> planes = synth_jungfrau_calibration(spec);
    if (planes.empty()) return fail("jfcal: not a source of raw Jungfrau words (synth:tinyraw, synth:jungfrau9mraw, synth:tinydark, synth:jungfrau9mdark)");
    std::ofstream f(file, std::ios::binary);
    f.write(reinterpret_cast<const char*>(planes.data()), (std::streamsize)(planes.size() * sizeof(float)));
    return f ? 0 : fail("jfcal: cannot write the file");
}

static int jfconvert(const std::string& raw_file, const std::string& cal_file, size_t W, size_t H, const std::string& out_file) {
    const std::vector<uint8_t> raw = read_file(raw_file), cal = read_file(cal_file);
    const size_t n_px = W * H;
    if (n_px == 0 || cal.size() != 6 * n_px * sizeof(float) || raw.size() % (2 * n_px) != 0) return fail("jfconvert: file sizes do not match W x H");
    std::vector<float> planes(6 * n_px);
    std::memcpy(planes.data(), cal.data(), cal.size());
    std::vector<uint16_t> words(raw.size() / 2);
    std::memcpy(words.data(), raw.data(), raw.size());
    std::vector<uint32_t> out(words.size());
    for (size_t f = 0; f < words.size() / n_px; ++f) jungfrau_convert(words.data() + f * n_px, n_px, planes.data(), out.data() + f * n_px);
    std::ofstream o(out_file, std::ios::binary);
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * 4));
    return o ? 0 : fail("jfconvert: cannot write the file");
}

static int jfrepedestal(const std::string& old_file, const std::string& prefix, const std::string& new_file, const std::string& min_frames_s,
                        const std::string& max_rms_s) {
    char* end = nullptr;
    const unsigned long long min_frames = std::strtoull(min_frames_s.c_str(), &end, 10);
    if (min_frames_s.empty() || *end || min_frames_s[0] == '-' || min_frames > 0xFFFFFFFFull) return fail("jfrepedestal: min_frames is not a number in 1 .. 2^32 - 1");
    const float max_rms = std::strtof(max_rms_s.c_str(), &end);
    if (max_rms_s.empty() || *end) return fail("jfrepedestal: max_rms is not a number");
    if (!ffsamd::jf_pedestal_args_ok((uint32_t)min_frames, max_rms)) return fail("jfrepedestal: min_frames must be at least 1, max_rms finite and >= 0 (0: no noise test)");
    const std::vector<uint8_t> old = read_file(old_file);
    if (old.empty() || old.size() % (6 * sizeof(float)) != 0) return fail("jfrepedestal: the calibration is not six planes of float32");
    const size_t n_px = old.size() / (6 * sizeof(float));
    const std::vector<uint8_t> count = read_file(prefix + ".count.u32"), sum = read_file(prefix + ".sum.u64"), sum_sq = read_file(prefix + ".sum_sq.u64");
    if (count.size() != 3 * n_px * 4 || sum.size() != 3 * n_px * 8 || sum_sq.size() != 3 * n_px * 8)
        return fail(("jfrepedestal: " + prefix + ".count.u32 / .sum.u64 / .sum_sq.u64 are not three planes each of the calibration's " + std::to_string(n_px) + " pixels").c_str());
    std::vector<float> planes(6 * n_px), pedestal(3 * n_px), rms(3 * n_px), out(6 * n_px);
    std::vector<uint32_t> c(3 * n_px);
    std::vector<uint64_t> s(3 * n_px), q(3 * n_px);
    std::vector<uint8_t> ok(3 * n_px);
    std::memcpy(planes.data(), old.data(), old.size());
    std::memcpy(c.data(), count.data(), count.size());
    std::memcpy(s.data(), sum.data(), sum.size());
    std::memcpy(q.data(), sum_sq.data(), sum_sq.size());
    jungfrau_pedestal_planes(c.data(), s.data(), q.data(), n_px, (uint32_t)min_frames, max_rms, pedestal.data(), rms.data(), ok.data());
    jungfrau_repedestal(planes.data(), n_px, pedestal.data(), ok.data(), out.data());
    std::ofstream o(new_file, std::ios::binary);
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(float)));
    return o ? 0 : fail("jfrepedestal: cannot write the file");
}

static int synthframes(const std::string& spec, const std::string& file) {
    auto r = make_synth_reader(spec);
    std::vector<uint8_t> px(r->image_shape()[0] * r->image_shape()[1] * r->get_element_size());
    std::ofstream o(file, std::ios::binary);
    for (size_t i = 0; i < r->get_number_of_images(); ++i) {
        if (r->get_raw_chunk(i, px).size() != px.size()) return fail("synthframes: short frame");
        o.write(reinterpret_cast<const char*>(px.data()), (std::streamsize)px.size());
    }
    return o ? 0 : fail("synthframes: cannot write the file");
}

static int spotbgglm(const char* path) {
    std::FILE* in = path ? std::fopen(path, "r") : stdin;
    if (!in) return fail("spotbgglm: cannot open the file");
    std::vector<uint32_t> bins((size_t)ffsamd::kSpotBgBins);
    int rc = 0;
    for (unsigned long long line = 0;; ++line) {
        int got = 0;
        for (; got < ffsamd::kSpotBgBins; ++got)
            if (std::fscanf(in, "%" SCNu32, &bins[(size_t)got]) != 1) break;
        if (got == 0) break;
        uint32_t tail = 0;
        if (got != ffsamd::kSpotBgBins || std::fscanf(in, "%" SCNu32, &tail) != 1) {
            std::fprintf(stderr, "spotbgglm: histogram %llu is short: 257 integers each\n", line);
            rc = 2;
            break;
        }
        const ffsamd::SpotBgGlmResult r = ffsamd::spotbg_glm_from_histogram(bins.data(), tail);
        uint64_t beta, mean;
        std::memcpy(&beta, &r.beta, sizeof beta);
        std::memcpy(&mean, &r.mean, sizeof mean);
        std::printf("%" PRIu32 " %" PRIu32 " %" PRId32 " %" PRIu32 " %" PRIu32 " %016" PRIx64 " %016" PRIx64 "\n", r.n_pixels, r.n_overflow, r.median, r.n_iter, r.status,
                    beta, mean);
    }
    if (path) std::fclose(in);
    return rc;
}

// key=value arguments of the two shoebox commands
struct KeyValues {
    std::map<std::string, std::string> kv;
    KeyValues(int argc, char** argv) {
        for (int i = 2; i < argc; ++i) {
            const std::string a = argv[i];
            const size_t eq = a.find('=');
            if (eq == std::string::npos) throw std::runtime_error("expected key=value, got " + a);
            kv[a.substr(0, eq)] = a.substr(eq + 1);
        }
    }
    bool has(const std::string& k) const { return kv.count(k) != 0; }
    std::string str(const std::string& k) const {
        auto it = kv.find(k);
        if (it == kv.end()) throw std::runtime_error("missing " + k + "=");
        return it->second;
    }
    double num(const std::string& k) const { return std::stod(str(k)); }
    KabschGeometry geometry() const {
        return KabschGeometry{num("distance"), num("beam_x"), num("beam_y"), num("pixel_x"), num("pixel_y"), num("wavelength"), num("osc_start"), num("osc_width")};
    }
};

static uint64_t bits_of(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

static int shoeboxgeom(const KeyValues& kv) {
    const KabschGeometry kg = kv.geometry();
    const ffs_scan_geometry g = shoebox_flat_geometry(kg);
    double v[20];   // (ffs_scan_geometry is twenty doubles)
    static_assert(sizeof g == sizeof v, "ffs_scan_geometry is twenty doubles");
    std::memcpy(v, &g, sizeof v);
    for (int i = 0; i < 20; ++i) std::printf("%016" PRIx64 "%c", bits_of(v[i]), i == 19 ? '\n' : ' ');
    for (const ShoeboxRecord& r : read_shoebox_file(kv.str("boxes"))) {
        const ffs_shoebox b = shoebox_from_record(kg, r);
        std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(b.s1[0]), bits_of(b.s1[1]), bits_of(b.s1[2]), bits_of(b.phi));
    }
    return 0;
}

template <typename PixelT>
static void shoebox_fold_all(const ffsamd::ShoeboxGeometry& g, const std::vector<ffsamd::ShoeboxEntry>& table, int algorithm, double delta_b, double delta_m,
                             const std::vector<uint8_t>& frames, int W, int H, const uint8_t* mask, uint32_t limit, std::vector<ffsamd::ShoeboxAcc>& acc,
                             std::vector<uint32_t>& hist) {
    const size_t frame_bytes = (size_t)W * H * sizeof(PixelT), n_images = frames.size() / frame_bytes;
    for (size_t i = 0; i < table.size(); ++i)
        for (int64_t n = std::max<int64_t>(table[i].z_min, 0); n < table[i].z_max && n < (int64_t)n_images; ++n)
            ffsamd::shoebox_fold_image(g, table[i], algorithm, delta_b, delta_m, reinterpret_cast<const PixelT*>(frames.data() + (size_t)n * frame_bytes), (size_t)W, W, H, mask,
                                       limit, n, acc[i], hist.data() + i * (size_t)ffsamd::kSpotBgBins);
}

static int shoebox(const KeyValues& kv) {
    const KabschGeometry kg = kv.geometry();
    const ffs_scan_geometry fg = shoebox_flat_geometry(kg);
    ffsamd::ShoeboxGeometry g;
    static_assert(sizeof g == sizeof fg, "the model's geometry is ffs_scan_geometry");
    std::memcpy(&g, &fg, sizeof g);
    const int W = (int)kv.num("width"), H = (int)kv.num("height"), bytes = (int)kv.num("bytes");
    if (W <= 0 || H <= 0 || (bytes != 2 && bytes != 4)) return fail("shoebox: width and height must be positive, bytes 2 or 4");
    const std::vector<uint8_t> frames = read_file(kv.str("frames"));
    if (frames.size() % ((size_t)W * H * bytes) != 0) return fail("shoebox: the frames file is not a whole number of images");
    std::vector<uint8_t> mask;
    if (kv.has("mask")) {
        mask = read_file(kv.str("mask"));
        if (mask.size() != (size_t)W * H) return fail("shoebox: the mask file is not width * height bytes");
    }
    const long long max_valid = kv.has("max_valid") ? std::stoll(kv.str("max_valid")) : -1;
    const std::string algo = kv.has("algorithm") ? kv.str("algorithm") : "ellipsoid", bg = kv.has("background") ? kv.str("background") : "tukey";
    if ((algo != "ellipsoid" && algo != "dials") || (bg != "tukey" && bg != "glm")) return fail("shoebox: algorithm is ellipsoid or dials, background tukey or glm");
    const double n_sigma = kv.has("n_sigma") ? kv.num("n_sigma") : 3.0;
    const double delta_b = shoebox_delta(n_sigma, kv.num("sigma_b")), delta_m = shoebox_delta(n_sigma, kv.num("sigma_m"));
    std::vector<ffsamd::ShoeboxEntry> table;
    std::vector<ffs_shoebox> boxes;
    if (kv.has("predictions")) boxes = boxes_of_predictions(read_prediction_file(kv.str("predictions")));
    else
        for (const ShoeboxRecord& r : read_shoebox_file(kv.str("boxes"))) boxes.push_back(shoebox_from_record(kg, r));
    for (const ffs_shoebox& b : boxes) {
        ffsamd::ShoeboxEntry e;
        static_assert(sizeof e == sizeof b, "the model's table entry is ffs_shoebox");
        std::memcpy(&e, &b, sizeof e);
        table.push_back(e);
    }
    // (what ffs_ctx_shoebox_begin refuses is refused here, by the same text)
    std::string why = ffsamd::shoebox_job_refusal(g, algo == "dials" ? ffsamd::kShoeboxDials : ffsamd::kShoeboxEllipsoid, delta_b, delta_m);
    if (!why.empty()) return fail(("shoebox: " + why).c_str());
    const int64_t bad = ffsamd::shoebox_table_refusal(table.data(), (uint32_t)table.size(), g.s0, W, H, why);
    if (bad >= 0) return fail(("shoebox: shoebox " + std::to_string(bad) + " " + why).c_str());
    std::vector<ffsamd::ShoeboxAcc> acc(table.size(), ffsamd::ShoeboxAcc{});
    std::vector<uint32_t> hist(table.size() * (size_t)ffsamd::kSpotBgBins, 0u);
    const uint32_t limit = ffsamd::counting_limit(max_valid);
    const int algorithm = algo == "dials" ? ffsamd::kShoeboxDials : ffsamd::kShoeboxEllipsoid;
    if (bytes == 2) shoebox_fold_all<uint16_t>(g, table, algorithm, delta_b, delta_m, frames, W, H, mask.empty() ? nullptr : mask.data(), limit, acc, hist);
    else shoebox_fold_all<uint32_t>(g, table, algorithm, delta_b, delta_m, frames, W, H, mask.empty() ? nullptr : mask.data(), limit, acc, hist);
    std::vector<ffs_shoebox_sum> sums(table.size());
    for (size_t i = 0; i < table.size(); ++i) {
        const ffsamd::ShoeboxSum r = ffsamd::shoebox_sum(acc[i], hist.data() + i * (size_t)ffsamd::kSpotBgBins, bg == "glm" ? ffsamd::kShoeboxBgGlm : ffsamd::kShoeboxBgTukey);
        static_assert(sizeof r == sizeof sums[i], "the model's record is ffs_shoebox_sum");
        std::memcpy(&sums[i], &r, sizeof r);
    }
    std::ofstream o(kv.str("out"), std::ios::binary);
    o.write(reinterpret_cast<const char*>(sums.data()), (std::streamsize)(sums.size() * sizeof(ffs_shoebox_sum)));
    std::printf("%s\n", shoebox_summary_line(sums.data(), sums.size()).c_str());
    return o ? 0 : fail("shoebox: cannot write the file");
}

static int predict(const KeyValues& kv) {
    const KabschGeometry kg = kv.geometry();
    const ffs_scan_geometry fg = shoebox_flat_geometry(kg);
    ffsamd::ShoeboxGeometry g;
    std::memcpy(&g, &fg, sizeof g);
    const int W = (int)kv.num("width"), H = (int)kv.num("height");
    if (W <= 0 || H <= 0) return fail("predict: width and height must be positive");
    const ffs_crystal fx = read_crystal_file(kv.str("crystal"), centring_from_letter(kv.has("centring") ? kv.str("centring") : "P"));
    ffsamd::PredictCrystal x;
    static_assert(sizeof x == sizeof fx, "the model's crystal is ffs_crystal");
    std::memcpy(&x, &fx, sizeof x);
    const long long n_images = std::stoll(kv.str("n_images"));
    if (n_images < 0 || n_images > 0xFFFFFFFFll) return fail("predict: n_images does not fit 32 bits");
    const double n_sigma = kv.has("n_sigma") ? kv.num("n_sigma") : 3.0;
    const double delta_b = shoebox_delta(n_sigma, kv.num("sigma_b")), delta_m = shoebox_delta(n_sigma, kv.num("sigma_m"));
    // (what ffs_ctx_predict refuses is refused here, by the same text)
    ffsamd::PredictSetup u;
    const std::string why = ffsamd::predict_refusal(g, x, (uint32_t)n_images, kv.num("dmin"), delta_b, delta_m, W, H, u);
    if (!why.empty()) return fail(("predict: " + why).c_str());
    std::vector<double> settings(((size_t)n_images + 1) * 9);
    ffsamd::predict_scan_settings(g, x.a_matrix, (uint32_t)n_images, settings.data());
    std::vector<ffsamd::PredictRecord> records;
    ffsamd::predict_all(u, settings.data(), records);
    std::vector<ffs_prediction> out(records.size());
    static_assert(sizeof(ffsamd::PredictRecord) == sizeof(ffs_prediction), "the model's record is ffs_prediction");
    if (!records.empty()) std::memcpy(out.data(), records.data(), records.size() * sizeof(ffs_prediction));
    std::ofstream o(kv.str("out"), std::ios::binary);
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(ffs_prediction)));
    std::printf("%s\n", predict_summary_line(u.n_candidates, out).c_str());
    return o ? 0 : fail("predict: cannot write the file");
}

static int indexbasis(const KeyValues& kv) {
    const ffs_scan_geometry fg = shoebox_flat_geometry(kv.geometry());
    ffsamd::ShoeboxGeometry g;
    std::memcpy(&g, &fg, sizeof g);
    const std::vector<double> xyz = read_centres_file(kv.str("centres"));
    const uint32_t n = (uint32_t)(xyz.size() / 3);
    const double max_cell = kv.num("max-cell");
    const long long points = kv.has("npoints") ? std::stoll(kv.str("npoints")) : 256;
    if (points < 0 || points > 0xFFFFFFFFll) return fail("indexbasis: npoints does not fit 32 bits");
    const uint32_t N = (uint32_t)points;
    double dmin = kv.has("dmin") ? kv.num("dmin") : 0.0, b_iso = 0.0;
    std::vector<double> rlp(xyz.size()), s1(xyz.size()), mm(xyz.size()), weight(n), weights;
    std::vector<uint32_t> cell(n), cells;
    // (what the library's entries refuse is refused here, by the same text)
    std::string why = ffsamd::index_rlp_refusal(&g, xyz.data(), n, rlp.data(), s1.data(), mm.data());
    if (why.empty() && kv.has("dmin") && !(dmin > 0.0)) why = "dmin must be finite and positive";
    if (!why.empty()) return fail(("indexbasis: " + why).c_str());
    for (uint32_t i = 0; i < n; ++i) ffsamd::index_rlp(g, &xyz[3 * (size_t)i], &rlp[3 * (size_t)i], &s1[3 * (size_t)i], &mm[3 * (size_t)i]);
    why = ffsamd::index_defaults_refusal(rlp.data(), n, max_cell, N, &dmin, &b_iso);
    if (!why.empty()) return fail(("indexbasis: " + why).c_str());
    ffsamd::index_defaults(rlp.data(), n, max_cell, N, dmin, b_iso);
    for (uint32_t i = 0; i < n; ++i) cell[i] = ffsamd::index_map_one(&rlp[3 * (size_t)i], dmin, b_iso, N, weight[i]);
    ffsamd::index_map_dedup(cell.data(), weight.data(), n, cells, weights);
    std::vector<double> tw(N), power(ffsamd::index_voxels(N));
    ffsamd::index_twiddles(N, tw.data());
    ffsamd::index_power_grid(cells.data(), weights.data(), cells.size(), N, tw.data(), power.data());
    ffsamd::IndexGridStats st;
    std::vector<ffsamd::IndexPeak> peaks;
    ffsamd::index_peaks(power.data(), N, ffsamd::kIndexRmsdCutoff, st, peaks);
    const std::vector<ffsamd::IndexVector> vectors =
        ffsamd::index_basis_vectors(peaks.data(), (uint32_t)peaks.size(), N, dmin, ffsamd::kIndexPeakVolumeCutoff, ffsamd::kIndexMinCell, max_cell);
    static_assert(sizeof(ffsamd::IndexPeak) == sizeof(ffs_index_peak) && sizeof(ffsamd::IndexVector) == sizeof(ffs_index_vector), "the model's records are the header's");
    const std::string prefix = kv.str("out");
    write_raw_file(prefix + ".peaks", peaks.data(), peaks.size() * sizeof(ffsamd::IndexPeak));
    write_raw_file(prefix + ".basis_vectors", vectors.data(), vectors.size() * sizeof(ffsamd::IndexVector));
    const std::string digest = sha256_hex(power.data(), power.size() * sizeof(double)) + "\n";
    write_raw_file(prefix + ".grid_sha256", digest.data(), digest.size());
    std::printf("index: %u spots, %zu cells, dmin %.5f, b_iso %.3f, %u voxels selected, %zu peaks\n", n, cells.size(), dmin, b_iso, st.n_selected, peaks.size());
    std::printf("%s", index_vector_lines(reinterpret_cast<const ffs_index_vector*>(vectors.data()), vectors.size()).c_str());
    return 0;
}

// indexassign: the CPU twin of `spotfinder --index-assign` (host/index_assign.hpp has the step; the rule is csrc/assign_model.hpp's).
//   centres=FILE and the geometry as for indexbasis; vectors=FILE (40-byte ffs_index_vector records, as indexbasis and --index-basis write
//   them: the settings are their triples) or settings=FILE (raw rows of nine float64); tolerance=0.3; out=PREFIX
static int indexassign(const KeyValues& kv) {
    const ffs_scan_geometry fg = shoebox_flat_geometry(kv.geometry());
    ffsamd::ShoeboxGeometry g;
    std::memcpy(&g, &fg, sizeof g);
    const std::vector<double> xyz = read_centres_file(kv.str("centres"));
    const uint32_t n = (uint32_t)(xyz.size() / 3);
    const double tolerance = kv.has("tolerance") ? kv.num("tolerance") : ffsamd::kAssignTolerance;
    std::vector<double> rlp(xyz.size()), s1(xyz.size()), mm(xyz.size()), phi(n);
    std::string why = ffsamd::index_rlp_refusal(&g, xyz.data(), n, rlp.data(), s1.data(), mm.data());
    if (!why.empty()) return fail(("indexassign: " + why).c_str());
    for (uint32_t i = 0; i < n; ++i) {
        ffsamd::index_rlp(g, &xyz[3 * (size_t)i], &rlp[3 * (size_t)i], &s1[3 * (size_t)i], &mm[3 * (size_t)i]);
        phi[i] = mm[3 * (size_t)i + 2];
    }
    static_assert(sizeof(ffsamd::AssignSetting) == sizeof(ffs_index_setting) && sizeof(ffsamd::AssignRecord) == sizeof(ffs_index_assignment), "the model's records are the header's");
    std::vector<ffs_index_setting> settings;
    if (kv.has("settings")) {
        settings = read_settings_file(kv.str("settings"));
    } else {
        if (!kv.has("vectors")) return fail("indexassign: missing vectors= or settings=");
        std::ifstream f(kv.str("vectors"), std::ios::binary);
        if (!f) return fail("indexassign: cannot open the vectors file");
        const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (raw.size() % sizeof(ffs_index_vector) != 0) return fail("indexassign: the vectors file is not a whole number of 40-byte records");
        std::vector<double> v(3 * (raw.size() / sizeof(ffs_index_vector)));
        for (size_t k = 0; k < v.size() / 3; ++k) std::memcpy(&v[3 * k], raw.data() + k * sizeof(ffs_index_vector), 3 * sizeof(double));
        why = ffsamd::assign_settings_refusal(v.data(), (uint32_t)(v.size() / 3), ffsamd::kAssignMaxCombinations, false, 0, false);
        if (!why.empty()) return fail(("indexassign: " + why).c_str());
        const std::vector<ffsamd::AssignSetting> made = ffsamd::assign_settings(v.data(), (uint32_t)(v.size() / 3), ffsamd::kAssignMaxCombinations);
        settings.resize(made.size());
        if (!made.empty()) std::memcpy(settings.data(), made.data(), made.size() * sizeof(ffs_index_setting));
    }
    const std::vector<ffsamd::AssignAbsenceTest> table = ffsamd::assign_absence_table();
    IndexAssignOps ops;
    ops.assign = [&](const double* A, uint32_t m, ffs_index_assignment* out, int32_t* hkl) {
        // (what ffs_ctx_index_assign refuses is refused here, by the same text)
        const std::string no = ffsamd::assign_refusal(rlp.data(), phi.data(), n, A, m, tolerance, !out);
        if (!no.empty()) throw std::runtime_error(no);
        for (uint32_t k = 0; k < m; ++k) {
            ffsamd::AssignRecord rec;
            ffsamd::assign_setting(rlp.data(), phi.data(), nullptr, n, A + 9 * (size_t)k, tolerance, rec, hkl ? hkl + 3 * (size_t)k * n : nullptr, nullptr);
            std::memcpy(&out[k], &rec, sizeof rec);
        }
    };
    ops.detect = [](const ffs_index_assignment& r) {
        ffsamd::AssignRecord rec;
        std::memcpy(&rec, &r, sizeof rec);
        return ffsamd::assign_detect(rec, ffsamd::kAssignThreshold);
    };
    ops.reindex = [&](const double* A, int32_t t, double* out) { return ffsamd::assign_reindex(A, table[(size_t)t].transform, out); };
    try {
        std::printf("%s", index_assign_run(ops, settings, n, kv.str("out")).c_str());
    } catch (const std::exception& e) {
        return fail((std::string("indexassign: ") + e.what()).c_str());
    }
    return 0;
}

// chunkfnv <chunk file> <nelem> <elem bytes>: decode one bitshuffle-LZ4 chunk with the host codec and
// print the FNV-1a of the pixels (cross-check for chunk writers)
static int chunkfnv(const std::string& path, size_t nelem, size_t es) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> c((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<uint8_t> px(nelem * es);
    if (c.size() < 12 || bshuf_decompress_lz4(c.data() + 12, c.size() - 12, px.data(), nelem, es) < 0)
        return fail("chunk does not decode");
    uint64_t h = 1469598103934665603ull;
    for (auto b : px) h = (h ^ b) * 1099511628211ull;
    std::printf("fnv %016llx\n", (unsigned long long)h);
    return 0;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    try {
        if (cmd == "selftest") return selftest();
        if (cmd == "mkshm" && argc == 4) return mkshm(argv[2], argv[3]);
        if (cmd == "mkcbf" && argc == 4) return mkcbf(argv[2], argv[3]);
        if (cmd == "mkh5" && argc >= 4) return mkh5(argc, argv);
        if (cmd == "h5info" && argc == 3) return h5info(argv[2]);
        if (cmd == "synthinfo" && argc == 3) return synthinfo(argv[2]);
        if (cmd == "chunkfnv" && argc == 5)
            return chunkfnv(argv[2], std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10));
        if (cmd == "jfcal" && argc == 4) return jfcal(argv[2], argv[3]);
        if (cmd == "jfconvert" && argc == 7)
            return jfconvert(argv[2], argv[3], std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10), argv[6]);
        if (cmd == "synthframes" && argc == 4) return synthframes(argv[2], argv[3]);
        if (cmd == "jfrepedestal" && argc >= 5 && argc <= 7) return jfrepedestal(argv[2], argv[3], argv[4], argc > 5 ? argv[5] : "1", argc > 6 ? argv[6] : "0");
        if (cmd == "h5stats" && argc == 4) { h5_print_group_stats(argv[2], argv[3]); return 0; }
        if (cmd == "spotbgglm" && argc <= 3) return spotbgglm(argc == 3 ? argv[2] : nullptr);
        if (cmd == "shoebox") return shoebox(KeyValues(argc, argv));
        if (cmd == "shoeboxgeom") return shoeboxgeom(KeyValues(argc, argv));
        if (cmd == "predict") return predict(KeyValues(argc, argv));
        if (cmd == "indexbasis") return indexbasis(KeyValues(argc, argv));
        if (cmd == "indexassign") return indexassign(KeyValues(argc, argv));
        if (cmd == "h5support") { std::printf("%d\n", h5_supported() ? 1 : 0); return 0; }
    } catch (const std::exception& e) {
        std::printf("Error: %s\n", e.what());
        return 1;
    }
    std::printf("usage: ffs_hosttool selftest | mkshm <synth:spec> <dir> | mkcbf <synth:spec> <prefix> |\n"
                "       mkh5 <synth:spec> <master.h5> [vds-links|vds-files|plain [frames_per_file [n_written]]] |\n"
                "       h5info <master.h5> | synthinfo <synth:spec> | h5support | h5stats <file.h5> <group> |\n"
                "       chunkfnv <chunk> <nelem> <elem bytes> | jfcal <synth:spec> <file> | jfconvert <raw> <cal> <W> <H> <out> |\n"
                "       synthframes <synth:spec> <file> | jfrepedestal <old cal> <prefix> <new cal> [min_frames [max_rms]] |\n"
                "       spotbgglm [histograms] | shoebox key=value ... | shoeboxgeom key=value ... | predict key=value ... |\n"
                "       indexbasis key=value ... | indexassign key=value ...\n");
    return 2;
}
