// cli_args.hpp -- the spotfinder driver's command line (spotfinder.cc:291-398, src/ffs/arg_parser.cc, src/ffs/cuda_arg_parser.cc)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#ifndef FFS_VERSION
#define FFS_VERSION "ffs-mi355x 0.1 (gfx950)"
#endif

namespace ffshost {

struct Args {
    std::string file;
    bool sample = false, validate = false, writeout = false, save_h5 = false, output_for_index = false;
    bool verbose = false, strict_dtype = false;
    uint32_t threads = 1, images = 0, min_spot_size = 3, min_spot_size_3d = 3, start_index = 0, batch = 0, assemblies = 0;
    bool images_set = false, wavelength_set = false, detector_set = false;
    float max_sep = 2.0f, timeout = 30.0f, dmin = -1.f, dmax = -1.f, wavelength = 0.f, slot_margin = 2.0f;
    int pipe_fd = -1, device = 0;
    std::vector<int> devices;  // --devices / --gpus: the frame queue is dealt to all of them
    std::string algorithm = "dispersion", detector_json, gather = "host";
    int algo = 0;   // FFS_ALGO_*: `algorithm`, lower-cased and checked by parse_args
    std::string max_valid = "trusted";   // trusted | none | N
    int max_valid_scope = 0;             // --max-valid-scope centre (FFS_MAX_VALID_CENTRE) | window (FFS_MAX_VALID_WINDOW)
    double gain = 0.0;                   // --gain G (> 0); 0 = not given: pixel values are photon counts
    std::string jungfrau_calibration;    // --jungfrau-calibration FILE (raw float32, 6 x width x height values); empty = not given
    std::string jungfrau_pedestal;       // --jungfrau-pedestal PREFIX: fold the source's dark frames into pedestal statistics, write PREFIX.*, find no spots; empty = not given
    uint32_t pedestal_min_frames = 1;    // --pedestal-min-frames N: a stage's pedestal is usable from N counted frames on
    float pedestal_max_rms = 0.0f;       // --pedestal-max-rms R: ... and with a noise of at most R ADU; 0 = no test
    std::string gain_map;                // --gain-map FILE (raw float32, width x height values); empty = not given.  Not with --gain
    uint32_t radial_bins = 0;            // --radial-bins N (1..1024): the per-image radial profile over N resolution shells; 0 = not given
                                         // (-a radial_profile: its shells, 100 unless given, at most 128)
    double n_iqr = 6.0;                  // --n-iqr X: -a radial_profile's cutoff is median + X x IQR of the shell
    int radial_blur = 0;                 // --radial-blur narrow | wide: FFS_RADIAL_BLUR_*, -a radial_profile's smoothing ahead of the threshold; 0 = not given
    bool spot_background_glm = false;    // --spot-background-model glm: the ring's background by the robust Poisson GLM instead of Tukey's fence (constant); needs --spot-background
    uint32_t spot_background = 0;        // --spot-background B (1..16): per spot, the background of the ring of B pixels around its box and the background-subtracted intensity; 0 = not given
    // --integrate FILE: summation integration of the predicted reflections in FILE (48-byte records: centre x, y, z as float64, the half-open box as
    // six int32) over the run; needs --sigma-b, --sigma-m (degrees, > 0) and --integrate-out PREFIX (PREFIX.shoebox_sums); empty = not given
    std::string integrate, integrate_out;
    double sigma_b = 0.0, sigma_m = 0.0, integrate_n_sigma = 3.0;
    int integrate_algorithm = 0;         // --integrate-algorithm ellipsoid (FFS_SHOEBOX_ELLIPSOID) | dials (FFS_SHOEBOX_DIALS)
    int integrate_background = 0;        // --integrate-background tukey (0) | glm (1)
    // --predict CRYSTAL: the reflections and their boxes are predicted on the GPU (ffs_ctx_predict) from CRYSTAL (nine raw float64: the A matrix,
    // row-major, 1/Angstrom) instead of read from --integrate's file; needs --predict-dmin, --sigma-b, --sigma-m and --integrate-out PREFIX
    // (PREFIX.predictions and PREFIX.shoebox_sums); not with --integrate; empty = not given
    std::string predict;
    double predict_dmin = 0.0;           // --predict-dmin D (Angstrom, > 0)
    int predict_centring = 0;            // --predict-centring P|I|F|A|B|C|R: FFS_CENTRING_*
    bool integrating() const { return !integrate.empty() || !predict.empty(); }
    // --index-basis PREFIX: after a rotation sweep's finish the 3D reflections' centres of mass go through the indexer's basis-vector search
    // (ffs_index_rlp .. ffs_ctx_index_grid / index_peaks .. ffs_index_basis_vectors); PREFIX.centres, PREFIX.peaks and PREFIX.basis_vectors are
    // written; needs --max-cell C; one GPU; not with --validate; empty = not given
    std::string index_basis;
    double index_max_cell = 0.0;         // --max-cell C (Angstrom, > 0)
    double index_dmin = 0.0;             // --index-dmin D (Angstrom, > 0); 0 = chosen from max_cell and the data
    uint32_t fft_npoints = 256;          // --fft-npoints N: a power of two in 16 .. 256
    // --index-assign PREFIX (with --index-basis): the candidate settings -- the triples of the run's basis vectors, or the raw rows of nine
    // float64 of --index-settings FILE -- are held against the centres on the GPU (ffs_ctx_index_assign), corrected for a non-primitive basis,
    // and PREFIX.settings, PREFIX.assignments and PREFIX.hkl are written; empty = not given
    std::string index_assign, index_settings;
    double index_tolerance = 0.3;        // --index-tolerance T in (0, 0.5]
    std::string pixel_stats;             // --pixel-stats PREFIX: per-pixel count, sum, sum of squares and maximum over the run, into PREFIX.*; empty = not given
    uint32_t min_count = 2;
    int kernel_half_x = 3, kernel_half_y = 3;   // --kernel-size
    bool cpu_decode = false, no_numa_pinning = false, single_buffer = false, all_threads = false, read_only = false, clean_exit = false;
};

void usage();
[[noreturn]] void arg_error(const std::string& m);   // "Error: ...", the usage text, exit code 1
// Exits by itself for -h, --version, --list-devices and on every error (usage errors: arg_error; an algorithm
// that does not exist: "Error: Invalid algorithm specified", exit code 1).
Args parse_args(int argc, char** argv);

}  // namespace ffshost
