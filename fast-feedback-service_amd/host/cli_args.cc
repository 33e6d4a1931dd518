// cli_args.cc -- see cli_args.hpp
#include "cli_args.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <sstream>

#include "ffs_hip.h"

namespace fs = std::filesystem;

namespace ffshost {

void usage() {
    std::printf(
      "Usage: spotfinder [-h] [--version] [-v] [-d DEVICE] [--list-devices] [--sample | FILE.nxs]\n"
      "                  [-n NUM] [--validate] [--images NUM] [--writeout] [--min-spot-size N]\n"
      "                  [--min-spot-size-3d N] [--max-peak-centroid-separation N] [--start-index N]\n"
      "                  [-t S] [-fd FD] [-a ALGO] [--dmin MIN D] [--dmax MAX D] [-w \xce\xbb] [--detector JSON]\n"
      "                  [-h5] [--output-for-index] [--batch N] [--cpu-decode] [--strict-dtype]\n"
      "                  [--max-valid trusted|none|N] [--max-valid-scope centre|window] [--min-count N] [--kernel-size N | NX,NY]\n"
      "                  [--gain G] [--gain-map FILE] [--radial-bins N] [--pixel-stats PREFIX]\n"
      "                  [--jungfrau-calibration FILE] [--jungfrau-pedestal PREFIX [--pedestal-min-frames N] [--pedestal-max-rms R]]\n"
      "                  [--spot-background B]\n"
      "                  [--spot-background-model constant|glm]\n"
      "                  [--n-iqr X] [--radial-blur narrow|wide]\n"
      "                  [--integrate FILE --sigma-b DEG --sigma-m DEG --integrate-out PREFIX [--integrate-algorithm ellipsoid|dials]\n"
      "                   [--integrate-background tukey|glm] [--integrate-n-sigma 3]]\n"
      "                  [--predict CRYSTAL --predict-dmin D --sigma-b DEG --sigma-m DEG --integrate-out PREFIX [--predict-centring P|I|F|A|B|C|R]\n"
      "                   [--integrate-n-sigma 3] [--integrate-algorithm ...] [--integrate-background ...]]\n"
      "                  [--index-basis PREFIX --max-cell C [--index-dmin D] [--fft-npoints N]\n"
      "                   [--index-assign PREFIX [--index-settings FILE] [--index-tolerance 0.3]]]\n"
      "                  [--devices D0,D1,... | --gpus N] [--no-numa-pinning] [--single-buffer] [--all-threads] [--read-only] [--clean-exit]\n"
      "--max-valid: a centre pixel above this value is never strong (the reference's kernels test it against the\n"
      "              data set's trusted maximum).  trusted (default) = the frame source's trusted-range maximum when it is\n"
      "              below the pixel type's maximum, none = no test (the CPU baseline's behaviour), N = this value\n"
      "--max-valid-scope: centre (default) = only a centre pixel above --max-valid is refused, and it still counts as a neighbour in\n"
      "              every window around it (the reference's kernels); window = such a pixel is masked for its frame, left out of\n"
      "              every window's count and sums, as the per-image mask of the DIALS pipeline does (the general-window kernel at every\n"
      "              --kernel-size; not with the device flavour of dispersion_extended)\n"
      "--min-count: valid pixels a window needs (default 2, the CPU baseline's; the reference's kernels use 3)\n"
      "--kernel-size: half-size of the dispersion window, both axes (N) or along x and y (NX,NY), each 1..7 (default 3:\n"
      "              the 7x7 window; DIALS spotfinder.threshold.dispersion.kernel_size).  Not with -a dispersion_extended\n"
      "--gain:      the detector gain G > 0 of the dispersion tests, for frames in ADU or keV whose background variance is G x mean,\n"
      "              not mean (DIALS spotfinder.threshold.dispersion.gain; default: none, pixel values are photon counts).  The\n"
      "              general-window kernel at every --kernel-size; also with -a dispersion_extended\n"
      "--gain-map:  the detector gain per pixel, for detectors whose modules or gain stages do not share one gain (DIALS\n"
      "              spotfinder.lookup.gain_map): FILE holds exactly width x height float32 values, little-endian, row-major, nothing\n"
      "              else; every value finite and in [2^-60, 2^60], under masked pixels too.  Each pixel is decided with the --gain\n"
      "              arithmetic and its own value.  Not together with --gain\n"
      "--jungfrau-calibration: the frames are the raw 16-bit words of a Jungfrau (two bits of gain stage, 14 bits of ADC) and are converted\n"
      "              to photon counts, 32 bits a pixel, with the calibration in FILE: exactly 6 x width x height float32 values, little-endian,\n"
      "              row-major, nothing else -- the pedestals of the stages G0, G1, G2, then their factors (photons per ADU; 0 = no\n"
      "              calibration for that pixel in that stage).  On the GPU (2 bytes a pixel cross PCIe), or with --cpu-decode on the worker\n"
      "              thread by the same rule.  Saturated and uncalibrated pixels are masked for their frame; --max-valid trusted becomes\n"
      "              min(trusted maximum, 2^24 - 1).  Needs a source of uncompressed 16-bit frames\n"
      "--jungfrau-pedestal: the frames are a DARK run of raw Jungfrau words (the detector in G0, then forced into G1, then into G2, in any\n"
      "              order: the word decides the stage).  Every frame is folded into per-pixel, per-stage accumulators -- on the GPU, or with\n"
      "              --cpu-decode on the worker threads by the same rule -- and no spots are found: one summary line, no JSON lines.  Written:\n"
      "              PREFIX.count.u32, PREFIX.sum.u64, PREFIX.sum_sq.u64 (the accumulators), PREFIX.pedestal.f32, PREFIX.rms.f32, PREFIX.ok.u8\n"
      "              (mean and noise of the ADC per stage, and whether the stage's pedestal is usable), three planes of width x height values\n"
      "              each (G0, G1, G2), raw little-endian; with --jungfrau-calibration OLD also PREFIX.calibration.f32, OLD with the pedestals\n"
      "              replaced and the factor set to 0 (no calibration) where the pedestal is not usable.  --pedestal-min-frames N (default 1):\n"
      "              usable from N counted frames on; --pedestal-max-rms R (default 0: no test): ... and with a noise of at most R ADU.  One\n"
      "              GPU; not with --validate or --writeout; needs a source of uncompressed 16-bit frames\n"
      "--radial-bins: per image, the count, sum and sum of squares of the valid pixels in each of N (1..1024) resolution shells of equal\n"
      "              width in 1/d^2, from the beam centre to the furthest pixel: the background level and its dispersion per shell, as\n"
      "              \"radial_count\", \"radial_sum\" and \"radial_sum_sq\" arrays in every image's JSON line (pixels above --max-valid and\n"
      "              masked pixels, --dmin / --dmax included, are left out).  Needs the detector geometry and the wavelength --dmin needs\n"
      "-a radial_profile: a pixel is a spot candidate when it stands above median + X x IQR of its resolution shell, both taken per image from\n"
      "              the shell's valid pixels (DIALS spotfinder.threshold.algorithm = radial_profile): for high or steeply\n"
      "              radial background, ice and solvent rings.  The shells are --radial-bins's (default 100 here, at most 128); --n-iqr X\n"
      "              (default 6, 0 .. 2^20).  --min-count, --kernel-size, --gain and --gain-map play no part.  Every image's JSON line gains\n"
      "              \"radial_median\", \"radial_cutoff\" and \"radial_status\" (0 decided, 1 no pixels, 2 more than a quarter at or above 256: no\n"
      "              spots in that shell).  --radial-blur narrow | wide (default none) smooths the image ahead of the threshold, over its valid\n"
      "              pixels only, with the 3 x 3 kernel (1 2 1) x (1 2 1) / 16 or the 5 x 5 kernel (1 4 6 4 1) x (1 4 6 4 1) / 256 (DIALS's\n"
      "              radial_profile.blur: fewer noise peaks, split spots combined); intensities and centroids stay the raw pixels', the three\n"
      "              arrays are the blurred image's.  Not with --validate\n"
      "--pixel-stats: per pixel over the whole run, in how many images it was at or below --max-valid (32-bit pixels: and below 2^24), the sum\n"
      "              and the sum of squares of its values there, and the largest of them: what a mask, a gain map (variance / mean of a\n"
      "              flat run) and the maximum image of a serial run are made from.  Masked pixels are in them.  Written after the last\n"
      "              image as PREFIX.count.u32, PREFIX.sum.u64, PREFIX.sum_sq.u64 and PREFIX.max.u32: raw little-endian, width x height\n"
      "              values, row-major, nothing else (the format --gain-map reads).  With several GPUs their statistics are merged: counts\n"
      "              and sums add, the maximum is the largest\n"
      "--spot-background: per spot, the constant background of the ring of B (1..16) pixels around its bounding box -- the valid pixels of the\n"
      "              padded box outside the box itself (masked pixels, --dmin / --dmax included, and pixels above --max-valid are left out), an\n"
      "              integer histogram of 256 bins, Tukey's fence q1 - 1.5 IQR .. q3 + 1.5 IQR, the mean of what is inside -- and the\n"
      "              background-subtracted intensity: \"spot_background_mean\", \"spot_intensity\" (sum - pixels x mean) and \"spot_variance\"\n"
      "              arrays in every image's JSON line, one entry per spot left after both filters, null where the ring gives no estimate\n"
      "              (no valid pixel, more than a quarter of it at or above 256, or a fence that reaches 256), and \"total_intensity\", the sum\n"
      "              of the image's estimated intensities.  Assumes photon counts (no gain is applied)\n"
      "--spot-background-model: constant (default) is the fenced mean above; glm fits the same ring with the robust Poisson GLM DIALS\n"
      "              integrates with (a constant mean with a log link, Huber's c = 1.345, at most 100 steps), which also answers where the\n"
      "              fence cannot (a ring of mostly zeros).  The same JSON keys are filled from its records, the variance being sum +\n"
      "              pixels^2 x mean / ring pixels; null where the ring has fewer than 10 valid pixels, more than a quarter of it at or above\n"
      "              256, or the fit does not converge.  Needs --spot-background\n"
      "--integrate: summation integration of predicted reflections over the run.  FILE holds raw little-endian records of 48 bytes: the\n"
      "              predicted centre x, y in pixels and z in images (three float64; z = 0 is the start of the first image), then the half-open\n"
      "              shoebox x_min x_max y_min y_max z_min z_max (six int32; it may hang over the image's edge).  On every image of a box its\n"
      "              pixels are foreground or background by an ellipsoid in Kabsch space of --integrate-n-sigma (default 3) x --sigma-b and\n"
      "              x --sigma-m (degrees: the estimates a rotation run prints), or by its first two axes alone (--integrate-algorithm dials);\n"
      "              the background is the box's own, by Tukey's fence or the robust Poisson GLM (--integrate-background).  Needs the detector\n"
      "              geometry and the wavelength --dmin needs, and a rotation source.  Written after the last image: PREFIX.shoebox_sums, one\n"
      "              record of 80 bytes per reflection in FILE's order (ffs_shoebox_sum of ffs_hip.h: foreground sum and count, the centroid\n"
      "              moments, background pixels, flags, background status and mean, intensity, variance), and one summary line.  With several\n"
      "              GPUs their integer accumulators are added.  Masked pixels and pixels above --max-valid do not count; a reflection whose\n"
      "              foreground meets one is flagged.  Not with --validate\n"
      "--predict:   instead of --integrate FILE, the reflections and their shoeboxes are predicted on the GPU before the first batch, for the\n"
      "              source's geometry and image count.  CRYSTAL holds nine raw little-endian float64: the A matrix row-major in 1/Angstrom\n"
      "              (r = A h in the laboratory frame at rotation angle 0).  --predict-dmin D is the resolution limit; --predict-centring leaves\n"
      "              out the lattice's absent indices (default P); the boxes are --integrate-n-sigma x --sigma-b and x --sigma-m in Kabsch\n"
      "              space.  One line says candidates, predictions and flagged records; PREFIX.predictions holds the records of 96 bytes\n"
      "              (ffs_prediction of ffs_hip.h); the boxes not flagged as refused are then integrated exactly as --integrate does\n"
      "--index-assign: after --index-basis, every candidate setting -- the triples of the run's basis vectors as the reference combines them, or\n"
      "              the raw rows of nine float64 (A, 1/Angstrom, row-major) of --index-settings FILE -- is held against the centres on the GPU:\n"
      "              Miller indices within --index-tolerance (default 0.3), duplicates resolved, a non-primitive basis detected and reindexed\n"
      "              (no Niggli reduction, no refinement, no score beyond the indexed count).  Every centre is assigned: the reference's\n"
      "              selection by resolution and rotation angle (ffs_index_select) is not applied, M below is the number of centres.\n"
      "              One line a setting, then the best one and\n"
      "              `Indexed N/M reflections`; PREFIX.settings holds the 160-byte ffs_index_setting records, PREFIX.assignments the 472-byte\n"
      "              ffs_index_assignment records after correction, PREFIX.hkl the best setting's n x 3 int32.\n"
      "--index-basis: after a rotation sweep's finish the 3D reflections' centres of mass are turned into candidate basis vectors on the GPU\n"
      "              (spot FFT on a grid of --fft-npoints a side, default 256, and peak search; the reference's indexer up to peaks_to_rlvs).\n"
      "              --max-cell C is the longest cell edge expected (Angstrom); --index-dmin D the resolution limit (default: from C and the\n"
      "              data).  PREFIX.centres holds the n x 3 float64 used (x_px, y_px, z), PREFIX.peaks the 56-byte ffs_index_peak records,\n"
      "              PREFIX.basis_vectors the 40-byte ffs_index_vector records; the vectors are printed as the reference logs them.  Needs a\n"
      "              rotation sweep; one GPU only; not with --validate\n"
      "--validate:  every image is also decided by an independent path (every valid pixel's window gathered from memory,\n"
      "              no streaming kernel) and the two strong-pixel masks are compared: Match / Mismatch per image\n"
      "--devices / --gpus: one context and worker pool per GPU, all pulling frames from the one queue\n"
      "              (-n threads are dealt round-robin to the GPUs, at least one each); rotation sweeps send\n"
      "              their strong-pixel lists to the first GPU's 3D stack (RCCL over xGMI, else peer copies)\n"
      "--all-threads: every one of the -n threads reads (default: at most eight per GPU when chunks are decoded there)\n"
      "--gather host|rccl: with several GPUs and --output-for-index, where the spot centres of a round of batches (one per GPU) are\n"
      "              collected: read from each context's host arrays (default: seven times cheaper inside one process), or gathered\n"
      "              over RCCL to the first GPU (counts by all-gather, rows by send / recv, one copy to the host)\n"
      "--clean-exit: destroy streams and contexts and let the runtime tear itself down before the process ends (default: the\n"
      "              process leaves as soon as its last result is out -- a request's wall time ends there)\n"
      "--batch N:   frames per GPU batch (default 16 chunks / 4 decoded frames); a batch is filled by all readers of its GPU\n"
      "--single-buffer: one batch per GPU at a time (default: four of chunks / three of decoded frames, filled while the others are on the GPU)\n"
      "--read-only: (diagnostic) read every chunk into the staging areas and submit nothing\n"
      "environment, A/B only: FFS_SHM_PLAIN_READ=1 -- /dev/shm chunks by read() straight into the staging area instead of\n"
      "              through a cache-resident bounce buffer and non-temporal stores\n"
      "--cpu-decode: decompress the frames' chunks (bitshuffle-LZ4, CBF byte-offset) on the worker thread (the reference's way) instead\n"
      "              of sending them to the GPU as they are\n"
      "FILE: NXmx .nxs/.h5 (needs an HDF5 build), a /dev/shm directory, a ####.cbf template, or\n"
      "      synth:<eiger16m|jungfrau9m|jungfrau9mraw|jungfrau9mdark|plumbing1k|sweep16m|tiny|tinyraw|tinydark|tinysweep>[:n_images[:seed]]\n");
}

[[noreturn]] void arg_error(const std::string& m) {  // arg_parser.cc:72-77
    std::printf("Error: %s\n", m.c_str());
    usage();
    std::exit(1);
}

static void list_devices() {  // cuda_arg_parser.cc:39-53
    const int n = ffs_device_count();
    for (int i = 0; i < n; ++i) {
        char name[256];
        ffs_device_name(i, name, sizeof name);
        std::printf("%d: %s\n", i, name);
    }
    std::exit(0);
}

Args parse_args(int argc, char** argv) {
    std::vector<std::string> a(argv + 1, argv + argc);
    if (fs::exists("common.args")) {  // arg_parser.cc:57-71
        std::ifstream f("common.args");
        std::string line;
        while (std::getline(f, line))
            if (!line.empty() && std::find(a.begin(), a.end(), line) == a.end()) a.push_back(line);
    }
    Args r;
    bool model_given = false;   // --spot-background-model, in either spelling: refused without --spot-background
    bool index_option_given = false;       // --max-cell, --index-dmin and --fft-npoints: refused without --index-basis
    bool assign_option_given = false;      // --index-settings and --index-tolerance: refused without --index-assign
    bool predict_option_given = false;     // --predict-dmin and --predict-centring: refused without --predict
    bool integrate_option_given = false;   // --sigma-b, --sigma-m and the --integrate-* options: refused without --integrate
    if (const char* e = std::getenv("SPOTFINDER_TIMEOUT")) {  // spotfinder.cc:293-301
        try { r.timeout = std::stof(e); } catch (...) { std::printf("Ignoring invalid SPOTFINDER_TIMEOUT value: %s\n", e); }
    }
    auto need = [&a](size_t& i, const std::string& flag) -> const std::string& {
        if (i + 1 >= a.size()) arg_error("Too few arguments for '" + flag + "'.");
        return a[++i];
    };
    auto u32 = [](const std::string& v, const std::string& flag) {
        try { size_t used; long long x = std::stoll(v, &used); if (used != v.size() || x < 0) throw 1; return (uint32_t)x; }
        catch (...) { arg_error("pattern not found for '" + flag + "': " + v); }
    };
    auto f32 = [](const std::string& v, const std::string& flag) {
        try { size_t used; float x = std::stof(v, &used); if (used != v.size()) throw 1; return x; }
        catch (...) { arg_error("pattern not found for '" + flag + "': " + v); }
    };
    for (size_t i = 0; i < a.size(); ++i) {
        const std::string& s = a[i];
        if (s == "-h" || s == "--help") { usage(); std::exit(0); }
        else if (s == "--version") { std::printf("%s\n", FFS_VERSION); std::exit(0); }
        else if (s == "-v" || s == "--verbose") r.verbose = true;
        else if (s == "--list-devices") list_devices();
        else if (s == "-d" || s == "--device") r.device = (int)u32(need(i, s), s);
        else if (s == "--sample") r.sample = true;
        else if (s == "-n" || s == "--threads") r.threads = u32(need(i, s), s);
        else if (s == "--validate") r.validate = true;
        else if (s == "--images") { r.images = u32(need(i, s), s); r.images_set = true; }
        else if (s == "--writeout") r.writeout = true;
        else if (s == "--min-spot-size") r.min_spot_size = u32(need(i, s), s);
        else if (s == "--min-spot-size-3d") r.min_spot_size_3d = u32(need(i, s), s);
        else if (s == "--max-peak-centroid-separation") r.max_sep = f32(need(i, s), s);
        else if (s == "--start-index") r.start_index = u32(need(i, s), s);
        else if (s == "-t" || s == "--timeout") r.timeout = f32(need(i, s), s);
        else if (s == "-fd" || s == "--pipe_fd") r.pipe_fd = std::stoi(need(i, s));
        else if (s == "-a" || s == "--algorithm") r.algorithm = need(i, s);
        else if (s == "--cpu-decode") r.cpu_decode = true;
        else if (s == "--dmin") r.dmin = f32(need(i, s), s);
        else if (s == "--dmax") r.dmax = f32(need(i, s), s);
        else if (s == "-w" || s == "--wavelength" || s == "-\xce\xbb") { r.wavelength = f32(need(i, s), s); r.wavelength_set = true; }
        else if (s == "--detector") { r.detector_json = need(i, s); r.detector_set = true; }
        else if (s == "-h5" || s == "--save-h5") r.save_h5 = true;
        else if (s == "--output-for-index") r.output_for_index = true;
        else if (s == "--batch") r.batch = u32(need(i, s), s);
        else if (s == "--assemblies") r.assemblies = u32(need(i, s), s);   // batches in flight per GPU (tuning; default below)
        else if (s == "--slot-margin") r.slot_margin = f32(need(i, s), s);  // per cent of head room per chunk slot (tuning)
        else if (s == "--gpus") { const uint32_t n = u32(need(i, s), s); r.devices.clear(); for (uint32_t d = 0; d < n; ++d) r.devices.push_back((int)d); }
        else if (s == "--devices") {
            r.devices.clear();
            std::stringstream ss(need(i, s));
            std::string tok;
            while (std::getline(ss, tok, ',')) r.devices.push_back((int)u32(tok, s));
        }
        else if (s == "--gather") { r.gather = need(i, s); if (r.gather != "host" && r.gather != "rccl") arg_error("--gather takes host or rccl"); }
        else if (s == "--strict-dtype") r.strict_dtype = true;
        else if (s == "--max-valid") {
            r.max_valid = need(i, s);
            if (r.max_valid != "trusted" && r.max_valid != "none") (void)u32(r.max_valid, s);
        }
        else if (s == "--max-valid-scope") {
            const std::string& v = need(i, s);
            if (v == "centre") r.max_valid_scope = FFS_MAX_VALID_CENTRE;
            else if (v == "window") r.max_valid_scope = FFS_MAX_VALID_WINDOW;
            else arg_error("--max-valid-scope takes centre or window: " + v);
        }
        else if (s == "--kernel-size") {
            const std::string& v = need(i, s);
            const size_t comma = v.find(',');
            auto half = [&u32, &s, &v](const std::string& t) {
                const uint32_t k = u32(t, s);
                if (k < 1 || k > 7) arg_error("--kernel-size takes half-sizes 1..7: " + v);
                return (int)k;
            };
            if (comma == std::string::npos) r.kernel_half_x = r.kernel_half_y = half(v);
            else {
                r.kernel_half_x = half(v.substr(0, comma));
                r.kernel_half_y = half(v.substr(comma + 1));
            }
        }
        else if (s == "--gain") {
            const std::string& v = need(i, s);
            try { size_t used; r.gain = std::stod(v, &used); if (used != v.size()) throw 1; }
            catch (...) { arg_error("pattern not found for '" + s + "': " + v); }
            if (!(r.gain > 0.0) || r.gain > 1.7976931348623157e308) arg_error("--gain takes a finite number above 0: " + v);
        }
        else if (s == "--jungfrau-calibration") {
            r.jungfrau_calibration = need(i, s);
            if (r.jungfrau_calibration.empty() || !fs::is_regular_file(r.jungfrau_calibration))
                arg_error("--jungfrau-calibration: no such file: " + r.jungfrau_calibration);
        } else if (s == "--gain-map") {
            r.gain_map = need(i, s);
            if (r.gain_map.empty() || !fs::is_regular_file(r.gain_map)) arg_error("--gain-map: no such file: " + r.gain_map);
        }
        else if (s == "--jungfrau-pedestal") {
            r.jungfrau_pedestal = need(i, s);
            if (r.jungfrau_pedestal.empty()) arg_error("--jungfrau-pedestal takes the prefix of the files it writes");
        }
        else if (s == "--pedestal-min-frames") {
            r.pedestal_min_frames = u32(need(i, s), s);
            if (r.pedestal_min_frames < 1) arg_error("--pedestal-min-frames must be at least 1");
        }
        else if (s == "--pedestal-max-rms") {
            const std::string& v = need(i, s);
            char* end = nullptr;
            r.pedestal_max_rms = std::strtof(v.c_str(), &end);
            if (v.empty() || *end || !(r.pedestal_max_rms >= 0.0f && r.pedestal_max_rms <= 3.4028234663852886e38f))
                arg_error("--pedestal-max-rms takes a finite number >= 0 (0: no noise test): " + v);
        }
        else if (s == "--pixel-stats") {
            r.pixel_stats = need(i, s);
            if (r.pixel_stats.empty()) arg_error("--pixel-stats takes the prefix of the four files it writes");
        }
        else if (s == "--spot-background") {
            const std::string& v = need(i, s);
            r.spot_background = u32(v, s);
            if (r.spot_background < 1 || r.spot_background > 16) arg_error("--spot-background takes a border in 1..16: " + v);
        }
        else if (s == "--spot-background-model") {
            const std::string& v = need(i, s);
            if (v == "constant") r.spot_background_glm = false;
            else if (v == "glm") r.spot_background_glm = true;
            else arg_error("--spot-background-model takes constant or glm: " + v);
            model_given = true;
        }
        else if (s == "--integrate") {
            r.integrate = need(i, s);
            if (r.integrate.empty()) arg_error("--integrate takes the file of predicted reflections");
        }
        else if (s == "--predict") {
            r.predict = need(i, s);
            if (r.predict.empty()) arg_error("--predict takes the crystal file (nine float64: the A matrix)");
        }
        else if (s == "--predict-dmin") {
            const std::string& v = need(i, s);
            char* end = nullptr;
            r.predict_dmin = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(r.predict_dmin > 0.0 && r.predict_dmin <= 1e6)) arg_error("--predict-dmin takes a finite number > 0 (Angstrom): " + v);
            predict_option_given = true;
        }
        else if (s == "--predict-centring") {
            const std::string& v = need(i, s);
            const size_t at = v.size() == 1 ? std::string("PIFABCR").find(v[0]) : std::string::npos;
            if (at == std::string::npos) arg_error("--predict-centring takes one of P I F A B C R: " + v);
            r.predict_centring = (int)at;
            predict_option_given = true;
        }
        else if (s == "--index-basis") {
            r.index_basis = need(i, s);
            if (r.index_basis.empty()) arg_error("--index-basis takes the prefix of the files it writes");
        }
        else if (s == "--index-assign") {
            r.index_assign = need(i, s);
            if (r.index_assign.empty()) arg_error("--index-assign takes the prefix of the files it writes");
        }
        else if (s == "--index-settings") {
            r.index_settings = need(i, s);
            if (r.index_settings.empty()) arg_error("--index-settings takes a file of raw rows of nine float64");
            assign_option_given = true;
        }
        else if (s == "--index-tolerance") {
            const std::string& v = need(i, s);
            char* end = nullptr;
            const double x = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x > 0.0 && x <= 0.5)) arg_error("--index-tolerance takes a number in (0, 0.5]: " + v);
            r.index_tolerance = x;
            assign_option_given = true;
        }
        else if (s == "--max-cell" || s == "--index-dmin") {
            const std::string& v = need(i, s);
            char* end = nullptr;
            const double x = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x > 0.0 && x <= 1e6)) arg_error(s + " takes a finite number > 0 (Angstrom): " + v);
            (s == "--max-cell" ? r.index_max_cell : r.index_dmin) = x;
            index_option_given = true;
        }
        else if (s == "--fft-npoints") {
            const std::string& v = need(i, s);
            char* end = nullptr;
            const long n = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || n < 16 || n > 256 || (n & (n - 1)) != 0) arg_error("--fft-npoints takes a power of two in 16 .. 256: " + v);
            r.fft_npoints = (uint32_t)n;
            index_option_given = true;
        }
        else if (s == "--integrate-out") {
            r.integrate_out = need(i, s);
            if (r.integrate_out.empty()) arg_error("--integrate-out takes the prefix of the file it writes");
        }
        else if (s == "--sigma-b" || s == "--sigma-m" || s == "--integrate-n-sigma") {
            const std::string& v = need(i, s);
            char* end = nullptr;
            const double x = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x > 0.0 && x <= 1e6)) arg_error(s + " takes a finite number > 0: " + v);
            (s == "--sigma-b" ? r.sigma_b : s == "--sigma-m" ? r.sigma_m : r.integrate_n_sigma) = x;
            integrate_option_given = true;
        }
        else if (s == "--integrate-algorithm") {
            const std::string& v = need(i, s);
            if (v == "ellipsoid") r.integrate_algorithm = FFS_SHOEBOX_ELLIPSOID;
            else if (v == "dials") r.integrate_algorithm = FFS_SHOEBOX_DIALS;
            else arg_error("--integrate-algorithm takes ellipsoid or dials: " + v);
            integrate_option_given = true;
        }
        else if (s == "--integrate-background") {
            const std::string& v = need(i, s);
            if (v == "tukey") r.integrate_background = 0;
            else if (v == "glm") r.integrate_background = 1;
            else arg_error("--integrate-background takes tukey or glm: " + v);
            integrate_option_given = true;
        }
        else if (s == "--radial-bins") {
            const std::string& v = need(i, s);
            r.radial_bins = u32(v, s);
            if (r.radial_bins < 1 || r.radial_bins > 1024) arg_error("--radial-bins takes a number of shells in 1..1024: " + v);
        }
        else if (s == "--n-iqr") {
            const std::string& v = need(i, s);
            char* end = nullptr;
            r.n_iqr = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(r.n_iqr >= 0.0 && r.n_iqr <= 1048576.0)) arg_error("--n-iqr takes a number in 0 .. 2^20: " + v);
        }
        else if (s == "--radial-blur") {
            const std::string& v = need(i, s);
            if (v == "none") r.radial_blur = 0;
            else if (v == "narrow") r.radial_blur = 1;
            else if (v == "wide") r.radial_blur = 2;
            else arg_error("--radial-blur takes narrow or wide (or none): " + v);
        }
        else if (s == "--min-count") { r.min_count = u32(need(i, s), s); if (r.min_count < 2) arg_error("--min-count must be at least 2"); }
        else if (s == "--no-numa-pinning") r.no_numa_pinning = true;
        else if (s == "--single-buffer") r.single_buffer = true;
        else if (s == "--read-only") r.read_only = true;   // diagnostic: frames are read into the staging buffers and not submitted
        else if (s == "--all-threads") r.all_threads = true;
        else if (s == "--clean-exit") r.clean_exit = true;
        else if (!s.empty() && s[0] == '-' && s.size() > 1) arg_error("Unknown argument: " + s);
        else if (r.file.empty()) r.file = s;
        else arg_error("Maximum number of positional arguments exceeded");
    }
    const bool implicit_sample = std::getenv("H5READ_IMPLICIT_SAMPLE") != nullptr;  // spotfinder.cc:268-283
    if (r.sample && !r.file.empty()) arg_error("Argument 'FILE.nxs' not allowed with '--sample'");
    if (!r.sample && r.file.empty() && !implicit_sample) arg_error("One of the arguments '--sample' or 'FILE.nxs' is required");
    if (r.file.empty()) r.sample = true;
    if (!r.jungfrau_pedestal.empty()) {   // (the mode takes one context and finds no spots)
        if (r.devices.size() > 1) arg_error("--jungfrau-pedestal takes one GPU: not with --devices / --gpus of more than one");
        if (r.validate) arg_error("--jungfrau-pedestal finds no spots: not with --validate");
        if (r.writeout) arg_error("--jungfrau-pedestal finds no spots: not with --writeout");
    } else if (r.pedestal_min_frames != 1 || r.pedestal_max_rms != 0.0f) {
        arg_error("--pedestal-min-frames and --pedestal-max-rms belong to --jungfrau-pedestal");
    }
    if (model_given && !r.spot_background) arg_error("--spot-background-model belongs to --spot-background");
    if (!r.predict.empty()) {
        if (!r.integrate.empty()) arg_error("--predict and --integrate exclude each other: the boxes are predicted or read from a file");
        if (!(r.predict_dmin > 0.0)) arg_error("--predict needs --predict-dmin D (Angstrom): the resolution limit of the prediction");
        if (!(r.sigma_b > 0.0) || !(r.sigma_m > 0.0)) arg_error("--predict needs both --sigma-b and --sigma-m (degrees): the boxes are n_sigma x sigma in Kabsch space");
        if (r.integrate_out.empty()) arg_error("--predict needs --integrate-out PREFIX: the records go to PREFIX.predictions and PREFIX.shoebox_sums");
        if (r.validate) arg_error("--predict is not available with --validate");
        if (!r.jungfrau_pedestal.empty()) arg_error("--jungfrau-pedestal finds no spots and integrates none: not with --predict");
    } else if (predict_option_given) {
        arg_error("--predict-dmin and --predict-centring belong to --predict");
    } else if (!r.integrate.empty()) {
        if (!(r.sigma_b > 0.0) || !(r.sigma_m > 0.0)) arg_error("--integrate needs both --sigma-b and --sigma-m (degrees): the foreground is an ellipsoid of n_sigma x sigma");
        if (r.integrate_out.empty()) arg_error("--integrate needs --integrate-out PREFIX: the records go to PREFIX.shoebox_sums");
        if (r.validate) arg_error("--integrate is not available with --validate");
        if (!r.jungfrau_pedestal.empty()) arg_error("--jungfrau-pedestal finds no spots and integrates none: not with --integrate");
    } else if (integrate_option_given || !r.integrate_out.empty()) {
        arg_error("--sigma-b, --sigma-m and the --integrate-* options belong to --integrate");
    }
    if (!r.index_basis.empty()) {
        if (!(r.index_max_cell > 0.0)) arg_error("--index-basis needs --max-cell C (Angstrom): the longest cell edge expected");
        if (r.validate) arg_error("--index-basis is not available with --validate");
        if (r.devices.size() > 1) arg_error("--index-basis takes one GPU: not with --devices / --gpus of more than one");
        if (!r.jungfrau_pedestal.empty()) arg_error("--jungfrau-pedestal finds no spots: not with --index-basis");
    } else if (index_option_given) {
        arg_error("--max-cell, --index-dmin and --fft-npoints belong to --index-basis");
    }
    // (--index-assign runs inside --index-basis' step: what that refuses -- --validate, several GPUs, --jungfrau-pedestal -- is refused with it)
    if (!r.index_assign.empty() && r.index_basis.empty()) arg_error("--index-assign needs --index-basis PREFIX --max-cell C: it assigns this run's centres");
    if (r.index_assign.empty() && assign_option_given) arg_error("--index-settings and --index-tolerance belong to --index-assign");
    if (r.gain > 0.0 && !r.gain_map.empty()) arg_error("--gain and --gain-map exclude each other: a constant map is the scalar gain");
    std::string lower = r.algorithm;   // DispersionAlgorithm, spotfinder.cc:180-203
    std::transform(lower.begin(), lower.end(), lower.begin(), [](unsigned char ch) { return (char)std::tolower(ch); });
    if (lower == "dispersion") r.algo = FFS_ALGO_DISPERSION;
    else if (lower == "dispersion_extended") {
        if (r.kernel_half_x != 3 || r.kernel_half_y != 3)
            arg_error("--kernel-size other than 3 is not available with the dispersion_extended algorithm");
        r.algo = FFS_ALGO_DISPERSION_EXTENDED;
    } else if (lower == "radial_profile") {
        // (the shells are --radial-bins's, 100 unless given; the histogram's LDS table holds 128 of them)
        if (r.radial_bins == 0) r.radial_bins = 100;
        if (r.radial_bins > 128) arg_error("-a radial_profile takes at most 128 shells (--radial-bins): " + std::to_string(r.radial_bins));
        if (r.validate) arg_error("--validate is not available with the radial_profile algorithm: the cross-check path is a dispersion path");
        r.algo = FFS_ALGO_RADIAL_PROFILE;
    } else {
        std::printf("Error: Invalid algorithm specified\n");
        std::exit(1);
    }
    return r;
}

}  // namespace ffshost
