/*
 * ffs_hip.h -- C ABI of libffs_hip.so: the MI355X (gfx950) spot-finder hot path.
 *
 * This is the drop-in boundary for the reference's per-frame device work and the
 * host connected-components stage that follows it.  Each entry point names the
 * reference interface it replaces (paths relative to the reference checkout).
 * Plain C: opaque handles, plain pointers and sizes, int status returns
 * (0 = FFS_OK, negative = error; ffs_last_error() gives the text).  No
 * exceptions cross this boundary and no torch / HIP types appear in it.
 *
 * Data flow of one batch (a window other than 7x7 -- ffs_params.kernel_half_x / _y -- takes
 * the general-window kernel of kernels_window.hpp instead of the streaming kernel below):
 *   frames (u16/u32: dense host rows, pitched device rows, or bitshuffle-LZ4 chunks decoded on the GPU)
 *     -> ONE streaming threshold kernel per batch: exact integer 7x7 window sums, a conservative group
 *        screen, and the oracle's float64 predicate (baseline/spotfinder/standalone.cc:113-174) decided
 *        in its drain -- replaces kernels/thresholding.cu:145-234; the strong mask stays a bit plane
 *     -> ONE sparse launch per batch, a workgroup per frame: strong-pixel compaction, union-find connected
 *        components, centroids and filters (replaces connected_components.cc:17-139, 207-266)
 *     -> per-frame counters and 40-byte records written straight into pinned host memory
 */
#ifndef FFS_HIP_H
#define FFS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libffs_hip.so is built with -fvisibility=hidden: what this header declares is all it exports */
#pragma GCC visibility push(default)

#define FFS_OK 0
#define FFS_ERR_INVALID (-1)   /* bad argument / state */
#define FFS_ERR_DEVICE (-2)    /* HIP runtime error */
#define FFS_ERR_NOMEM (-3)     /* host or device allocation failed */
#define FFS_ERR_OVERFLOW (-4)  /* a frame produced more strong pixels / spots than the context was sized for */
#define FFS_ERR_NODEVICE (-5)  /* no usable GPU */

typedef struct ffs_ctx ffs_ctx;
typedef struct ffs_stream ffs_stream;
typedef struct ffs_stack3d ffs_stack3d;

/* Algorithm parameters.  Defaults (ffs_default_params) are the oracle's,
 * baseline/spotfinder/standalone.cc:16-20: 7x7 window (kernel_half_x = kernel_half_y = 3), min_count 2, nsig_b 6,
 * nsig_s 3, threshold 0; the GPU reference's launch wrapper defaults
 * (spotfinder/spotfinder.cuh:18-20) differ only in min_count = 3. */
typedef struct {
    int32_t min_count;        /* window needs >= this many valid pixels */
    double nsig_b;            /* background (dispersion) significance */
    double nsig_s;            /* signal significance */
    double threshold;         /* centre pixel must be > threshold */
    int64_t max_valid;        /* centre pixel must be <= max_valid (thresholding.cu:208-215);
                                 < 0 = no test (oracle behaviour) */
    uint32_t min_spot_size;   /* --min-spot-size, spotfinder.cc:318-322 (default 3) */
    uint32_t min_spot_size_3d;/* --min-spot-size-3d, :324-328 (default 3) */
    float max_peak_centroid_separation; /* :330-336 (default 2.0) */
    int32_t want_reflections; /* compute find_2d_components output per frame (spotfinder.cc:919-933) */
    int32_t want_strong_list; /* return the sparse strong-pixel list (k, intensity) per frame */
    int32_t want_strong_mask; /* produce and return the dense W*H byte mask per frame (reference D2H, :887-897); 0 (default): the
                               * strong mask stays a bit plane on the device and only lists / boxes / reflections come back */
    int32_t algorithm;        /* FFS_ALGO_DISPERSION (default) or FFS_ALGO_DISPERSION_EXTENDED:
                                 `--algorithm`, spotfinder.cc:338-342, 572-590; or FFS_ALGO_RADIAL_PROFILE (below) */
    int32_t extended_flavour; /* extended only.  0 = baseline.cpp:730-761 rules (default); 1 = where the
                                 device kernels differ structurally: erosion skips masked neighbours
                                 (erosion.cu:101-105), second pass needs n > 0 (thresholding.cu:472) */
    int32_t kernel_half_x;    /* window half-width along x (fast) and ... */
    int32_t kernel_half_y;    /* ... along y (slow): the window is (2*kx+1) x (2*ky+1) pixels (kernel_size_{x,y},
                                 standalone.cc:16,121-122; DIALS dispersion.kernel_size).  1..7 each; 0 means 3, so a
                                 zero-initialised struct keeps the 7x7 window.  Needs 2 <= min_count <= (2kx+1)(2ky+1).
                                 Anything but 3,3 runs the general-window kernel (FFS_PATH_WINDOW); refused together with
                                 FFS_ALGO_DISPERSION_EXTENDED */
} ffs_params;

#define FFS_ALGO_DISPERSION 0
#define FFS_ALGO_DISPERSION_EXTENDED 1
/* The radial-profile threshold: a pixel is strong when it stands far above the background of its shell of the context's radial bin map
 * (ffs_ctx_set_radial_bins, at most 128 bins here), measured per frame by the shell's median and interquartile range.  The reference has
 * no counterpart (its `--algorithm` knows the two above, spotfinder/spotfinder.cc:338-342); modelled on DIALS's
 * spotfinder.threshold.algorithm = radial_profile (its blur: ffs_ctx_set_radial_blur, off by default), and no parity with DIALS is claimed: this definition is the contract.
 *   A pixel COUNTS in shell b under the radial profile's rule (ffs_ctx_set_radial_bins): b != 0xFFFF, its valid-pixel mask bit is set (the
 *   mask as it stands at submit), p <= max_valid when max_valid >= 0 (both scopes), and for 32-bit pixels p < 2^24.
 *   Per frame and shell, over its N counting pixels, from a histogram of one-count bins 0..255 and a tail: n_overflow = those with p >= 256;
 *   status FFS_RADIAL_THR_EMPTY when N = 0; otherwise, with the 1-based sorted positions (N+3)/4, (N+1)/2 and (3N+1)/4 (integer division),
 *   FFS_RADIAL_THR_OVERFLOW when the value at the third position is >= 256 (the position is above N - n_overflow); otherwise
 *   FFS_RADIAL_THR_OK with q1, median, q3 the values at the three positions, iqr = q3 - q1 and
 *   cutoff = floor((double)median + n_iqr * (double)iqr), product and sum each rounded to nearest on their own (no fused multiply-add).
 *   Under the other two statuses the quartiles are -1 and the cutoff is 0.
 *   A pixel is STRONG when it counts in shell b, b's status is 0, p > cutoff[b] (integers) and (double)p > ffs_params.threshold.
 *   min_count, nsig_b, nsig_s, kernel_half_x / _y, extended_flavour, the gain, the gain map and the scope of max_valid beyond the
 *   counting rule play no part (the IQR measures the spread itself); connected components, filters, records, lists, byte mask, 3D stack,
 *   radial profile, pixel statistics and spot backgrounds of such a batch are what they are for any strong plane.
 * ffs_ctx_set_params refuses it (FFS_ERR_INVALID) while the context has no bin map or one of more than 128 bins; ffs_ctx_set_radial_bins
 * refuses NULL and a map of more than 128 bins while the context's parameters say this algorithm.  ffs_params keeps its layout. */
#define FFS_ALGO_RADIAL_PROFILE 2

void ffs_default_params(ffs_params *p);

/* struct Reflection, spotfinder/connected_components/connected_components.hpp:27-30 */
typedef struct {
    uint32_t l, t, r, b;
    int32_t num_pixels;
} ffs_box;

#define FFS_REFL_FILTERED_SIZE 1u /* removed by min_spot_size (connected_components.cc:213-222) */
#define FFS_REFL_FILTERED_SEP 2u  /* removed by peak-centroid distance (:224-233) */

/* class Reflection3D, connected_components.hpp:32-260 (what its getters and
 * center_of_mass() / peak_centroid_distance() return). */
typedef struct {
    uint32_t x_min, x_max, y_min, y_max;
    int32_t z_min, z_max;
    int32_t num_pixels;
    float com_x, com_y, com_z;
    uint32_t peak_x, peak_y;
    int32_t peak_z;
    uint32_t peak_intensity;
    float peak_centroid_distance;
    uint32_t flags;
    uint64_t sum_intensity;
} ffs_reflection;

/* What the reference's worker has in hand after ConnectedComponents(...)
 * (spotfinder.cc:901-933) for one frame.  Pointers stay valid until the next
 * ffs_wait() on the same stream. */
typedef struct {
    int64_t frame_id;
    uint32_t num_strong_pixels;          /* get_num_strong_pixels() */
    uint32_t num_strong_pixels_filtered; /* get_num_strong_pixels_filtered() */
    uint32_t n_components;               /* "Extracted {} spots", connected_components.cc:119 */
    uint32_t n_boxes;                    /* boxes.size() after the min-size filter = JSON n_spots_total */
    const ffs_box *boxes;                /* label order */
    uint32_t n_reflections;              /* find_2d_components(): after both filters, label order */
    const ffs_reflection *reflections;   /* NULL unless want_reflections */
    uint32_t n_filtered_size, n_filtered_sep;
    const uint32_t *strong_k;            /* ascending linear index y*W+x; NULL unless want_strong_list */
    const uint32_t *strong_intensity;
    const uint8_t *strong_mask;          /* dense W*H, NULL unless want_strong_mask */
} ffs_frame_result;

/* ---- devices (replaces CUDAArgumentParser --list-devices / -d, src/ffs/cuda_arg_parser.cc:30-61) */
int ffs_device_count(void);
int ffs_device_name(int device, char *buf, size_t buflen);
int ffs_device_total_mem(int device, uint64_t *bytes);

/* ---- context: one per (GPU, detector geometry) --------------------------------------------- */
/* pixel_bytes: 2 (uint16) or 4 (uint32) -- replaces the compile-time pixel_t switch
 * (h5read/include/h5read.h:16-20, spotfinder/CMakeLists.txt:45-73).
 * max_batch: frames per submit.  max_strong_per_frame: strong pixels per frame the batch lists are sized for,
 * 0 = default min(W*H, 2^18) (and min(that, 65536) components).  Not a limit on the data: a frame that exceeds
 * either is run again on its own with room for it inside ffs_wait() (the reference's std::map of signals,
 * connected_components.cc:24-32, has no bound), at the price of that extra pass. */
int ffs_ctx_create(int device, uint32_t width, uint32_t height, int pixel_bytes,
                   uint32_t max_batch, uint32_t max_strong_per_frame, ffs_ctx **out);
/* Lifetime rules (the reference: RAII members of one worker thread, spotfinder.cc:729-742; CUDA_CHECK aborts by exception,
 * include/cuda_common.hpp:28-45 -- here nothing aborts):
 *  - ffs_ctx_destroy() first closes the streams and 3D stacks that were created on the context and are still alive (waiting for
 *    their work in flight), then the context.  Their handles are dead from then on.
 *  - every destroy call is idempotent: on a handle that was destroyed already (by its own destroy call or with its context) it does
 *    nothing, so a caller's teardown -- finalisers of a binding, unwinding of a driver -- may let go of contexts, streams and stacks
 *    in ANY order.  ffs_submit* / ffs_wait on such a handle return FFS_ERR_INVALID.  (Handles are compared by address: do not keep a
 *    dead handle across the creation of new ones.)
 *  - no other thread may be inside a call on a handle, or on a child of a context, while it is being destroyed.
 *  - a process may exit (exit(), return from main, an interpreter shutting down) with handles alive and batches in flight: the
 *    library's exit handler, which runs before the HIP runtime's own, joins its helper threads and drains the devices; destroy calls
 *    that arrive after that (static destructors, late finalisers) do nothing.  _exit() / quick_exit() skip it, like any handler. */
void ffs_ctx_destroy(ffs_ctx *ctx);
/* Text of the calling thread's most recent error (kept per thread: worker threads drive their own
 * streams of one context).  ctx may be NULL: last error of ffs_ctx_create. */
const char *ffs_last_error(const ffs_ctx *ctx);

/* upload_mask(), spotfinder/spotfinder.cc:61-108: host_mask = W*H bytes, nonzero = valid,
 * or NULL for "all valid" (the reference's cudaMemset(1) branch). */
int ffs_ctx_set_mask(ffs_ctx *ctx, const uint8_t *host_mask);

/* call_apply_resolution_mask(), spotfinder/kernels/masking.cuh:82-97 + masking.cu:37-147:
 * clears mask bits whose d-spacing is outside [dmin, dmax] (<= 0 = unbounded). */
int ffs_ctx_apply_resolution_mask(ffs_ctx *ctx, float wavelength, float distance_m,
                                  float beam_center_x_px, float beam_center_y_px,
                                  float pixel_size_x_m, float pixel_size_y_m, float dmin,
                                  float dmax);
/* Read the current mask back (W*H bytes, 0/1) -- what --writeout copies for mask_calculated.png */
int ffs_ctx_get_mask(ffs_ctx *ctx, uint8_t *host_mask);

int ffs_ctx_set_params(ffs_ctx *ctx, const ffs_params *p);

/* The scope of ffs_params.max_valid.  Replaces nothing in the reference's kernels: there a pixel above the trusted maximum is
 * only never strong itself (thresholding.cu:208-215) and still counts as a neighbour in every window it falls into.  What it
 * stands in for is the per-image mask of the DIALS pipeline (built by dxtbx from the trusted range), which excludes such a pixel
 * before the threshold sees it.
 *   FFS_MAX_VALID_CENTRE (0, default): the reference kernels' behaviour -- only the centre pixel is tested.
 *   FFS_MAX_VALID_WINDOW (1): a pixel p > max_valid is masked for its frame -- left out of the count and both sums of every
 *     window, and never strong: the result is the oracle's on the mask `mask & (img <= max_valid)` (for 32-bit pixels the
 *     oracle's p < 2^24 rule holds on top).  Such a batch takes the general-window kernel at every window (FFS_PATH_WINDOW).
 *     With max_valid < 0 the scope changes nothing.
 * Per context; kept across ffs_ctx_set_params; like the parameters a batch takes it as it is at submit.  FFS_ERR_INVALID, state
 * unchanged: any other value; FFS_MAX_VALID_WINDOW together with extended_flavour 1, whichever call comes second (the device
 * flavour's erosion skips masked neighbours by the static mask, and the reference's kernels have no per-frame mask to copy). */
#define FFS_MAX_VALID_CENTRE 0
#define FFS_MAX_VALID_WINDOW 1
int ffs_ctx_set_max_valid_scope(ffs_ctx *ctx, int scope);

/* The detector gain of both dispersion tests: DIALS spotfinder.threshold.dispersion.gain, as one scalar per context.  The tests
 * assume that a background window's variance equals its mean (photon counts); a detector that delivers ADU or keV (Jungfrau, CCDs,
 * any integrating detector) has variance = gain * mean.  The arithmetic is the reference's threshold_w_gain of
 * baseline/spotfinder/baseline.cpp with a constant gain map; the reference's GPU kernels and standalone.cc have no gain.
 *   0 (default): off -- the same kernels, paths and results as before, bit for bit.
 *   g > 0 (1.0 included): with the window sums m, x, y counted as without a gain and converted once to float64, each operation
 *     rounded separately in this order --
 *       standard algorithm (baseline.cpp:241-247):  a = m*y - x*x;  b = m*p - x;
 *         c = (g*x) * ((m - 1) + nsig_b*sqrt(2*(m - 1)));  d = nsig_s*sqrt((g*x)*m);  strong = a > c && b > d
 *       extended algorithm, flavour 0: first pass a > c with the same a and c (:539-543); erosion unchanged; final pass
 *         p >= mean + nsig_s*sqrt(g*mean) (:709-715).
 *     A gain batch of the standard algorithm takes the general-window kernel at every window (FFS_PATH_WINDOW); the extended
 *     algorithm takes its plain first pass.  Composes with every kernel_half_x / _y and with FFS_MAX_VALID_WINDOW.
 * Per context; kept across ffs_ctx_set_params; like the parameters a batch takes it as it is at submit.  FFS_ERR_INVALID, state
 * unchanged (ffs_last_error has the text): a negative, NaN or infinite gain; a gain > 0 together with extended_flavour 1,
 * whichever call comes second (that flavour copies the reference's device kernels, which have no gain). */
int ffs_ctx_set_gain(ffs_ctx *ctx, double gain);

/* The detector gain per pixel: DIALS spotfinder.lookup.gain_map, for detectors whose modules, tapers or gain stages do not share one
 * gain.  The reference's threshold_w_gain (baseline/spotfinder/baseline.cpp) takes a gain ARRAY and reads the entry of the centre
 * pixel: gain[k] at :244-245 (standard algorithm), :541 (extended first pass), :714 (extended final pass).
 *   host_gain: W*H float32, row-major, dense; copied before the call returns.  NULL = no map (the default).
 *   The arithmetic is exactly that of ffs_ctx_set_gain above, with g = (double)host_gain[y*W + x] of the pixel (x, y) being decided --
 *   the window's CENTRE, never a neighbour's entry.  Window sums, erosion, min_count, threshold and max_valid under both scopes are
 *   what they are without a gain.  The map is float32 because the kernels read it once per pixel and frame and no calibration carries
 *   more than 24 bits; the widening to float64 is exact, so a constant map of value c gives bit for bit the results of
 *   ffs_ctx_set_gain(ctx, (double)(float)c).
 *   A map batch takes the paths a gain batch takes: FFS_PATH_WINDOW at every window, the extended algorithm's plain first pass,
 *   erosion + final pass under tuning "ext_fused", the gather under "threshold_path" 2.  Composes with every kernel_half_x / _y and
 *   with FFS_MAX_VALID_WINDOW.  With no map and gain 0 everything is as before: kernels, paths and results.
 * A property of the context like the mask, not a per-batch snapshot: kept across ffs_ctx_set_params, and it cannot change under a
 * batch.  FFS_ERR_INVALID, state unchanged (ffs_last_error has the text):
 *   - an entry that is not finite or not in [2^-60, 2^60] (zero, negative, NaN, infinite): the text names the index of the first
 *     one.  Entries under masked pixels are checked like all others: replace zeros or NaNs in detector gaps first;
 *   - a map while any stream of the context has a batch between submit and ffs_wait (NULL is accepted then too: the batch in
 *     flight and its re-runs inside ffs_wait go on with the map they were submitted with, which stays on the device);
 *   - a map while a gain > 0 is set, and ffs_ctx_set_gain(g > 0) while a map is set: the two are exclusive
 *     (ffs_ctx_set_gain(ctx, 0) and ffs_ctx_set_gain_map(ctx, NULL) are always accepted otherwise);
 *   - a map together with extended_flavour 1, whichever call comes second, as for the scalar. */
int ffs_ctx_set_gain_map(ffs_ctx *ctx, const float *host_gain);

/* The calibration that turns raw Jungfrau words into photon counts (FFS_CODEC_JUNGFRAU_RAW of ffs_submit_encoded; the rule is stated once,
 * in csrc/jungfrau_model.hpp, and compiled by the kernel, the driver's host converter and a CPU check).  The reference has no counterpart:
 * its readers hand over photon counts.
 *   A raw word r has the gain code g = r >> 14 and adc = r & 0x3FFF; the stage is s = 0, 1, 2 for g = 0, 1, 3.
 *   pedestal[s], factor[s]: W*H float32 each, row-major, dense; copied before the call returns.  The factor is photons per ADU,
 *   1 / (gain_s x photon energy), negative for the inverted stages; 0 marks "no calibration for this pixel in this stage".
 *   The pixel is 0xFFFFFFFF (invalid) when g == 2, r == 0xFFFF, r == 0xC000 (stage G2 with ADC 0: saturated) or factor[s][k] == 0.
 *   Otherwise d = (float)adc - pedestal[s][k], v = d * factor[s][k] (two float32 operations, never fused), q = rintf(v) with ties to
 *   even, and the pixel is 0 for q <= 0, 16777215 for q >= 16777215, (uint32_t)q otherwise.  Bit for bit on the GPU and the host.
 *   An invalid pixel is >= 2^24 and so left out of every window, the radial profile, the pixel statistics, the blur and the spot
 *   backgrounds, as any such 32-bit pixel is; with max_valid <= 2^24 - 1 it is never strong as a centre either.  Without a max_valid
 *   it is compared as a centre like any value and comes out strong: set max_valid (the driver does).
 * cal == NULL drops the calibration.  A property of the context like the mask: kept across ffs_ctx_set_params, replaceable between
 * batches (pedestals drift).  FFS_ERR_INVALID, state unchanged (ffs_last_error has the text):
 *   - a context of pixel_bytes 2, or a NULL plane;
 *   - an entry that is not finite, a pedestal outside [-65536, 65536], a factor that is neither 0 nor of magnitude in [2^-30, 2^16]:
 *     the text names the plane and the index of the first one;
 *   - a calibration (or NULL) while any stream of the context has a batch between submit and ffs_wait. */
typedef struct { const float *pedestal[3]; const float *factor[3]; } ffs_jungfrau_calibration;
int ffs_ctx_set_jungfrau_calibration(ffs_ctx *ctx, const ffs_jungfrau_calibration *cal);

/* The per-frame radial profile: per frame and bin of a caller-defined bin map (resolution shells, usually), how many pixels count, their
 * sum and their sum of squares -- the background level and its dispersion per shell, what DIALS builds its radial_profile threshold, its
 * ice-ring filter and its per-image analysis on.  The reference reports nothing of the kind (its per-image output is the strong mask and
 * the spots, spotfinder/spotfinder.cc:887-933).  Computed on the device from what a batch has there anyway: the pixels, the valid-pixel
 * mask, max_valid.
 *   bin_of_pixel: W*H uint16, row-major, dense; copied before the call returns.  An entry is a bin index < n_bins, or 0xFFFF for "in no
 *   bin".  n_bins: 1..1024.  NULL = no map (the default): every kernel, path and result is as before.
 *   The caller defines the bins and the library never computes a resolution (the resolution mask works in float32 with atanf / sinf;
 *   binning on that would make shell membership a rounding question): any geometry works -- several panels; shells equal in 1/d^2, in d
 *   or in radius; azimuthal sectors.
 *   A pixel (x, y) of a frame counts into bin b = bin_of_pixel[y*W + x] when all of these hold:
 *     - b != 0xFFFF;
 *     - its bit in the context's valid-pixel mask is set -- the mask as it stands at submit, ffs_ctx_apply_resolution_mask included;
 *     - p <= max_valid when ffs_params.max_valid >= 0, under both scopes of max_valid;
 *     - for 32-bit pixels, p < 2^24 (the oracle's neighbour rule, standalone.cc:78,90).
 *   Per frame and bin: count (uint32), sum = the sum of p (uint64), sum_sq = the sum of p*p (uint64, taken modulo 2^64).  sum_sq is exact for
 *   every 16-bit frame (2^32 * 2^25 < 2^64); it can wrap only for 32-bit frames with more than 65 536 pixels near 2^24 in one bin.
 *   All three are integers and independent of the order of summation: the result is exact, bit for bit.
 *   The profile depends on nothing of the threshold stage: algorithm, window, gain, the scope of max_valid beyond the rule above, tuning
 *   keys, or the path a batch takes (a batch that ffs_wait runs again keeps the profile of its first pass).
 * A property of the context like the mask and the gain map: kept across ffs_ctx_set_params; a batch takes it as it is at submit.
 * FFS_ERR_INVALID, state unchanged (ffs_last_error has the text):
 *   - n_bins outside 1..1024;
 *   - an entry >= n_bins that is not 0xFFFF: the text names the index of the first one, with its x and y;
 *   - a map while any stream of the context has a batch between submit and ffs_wait.  As for the gain map, NULL is accepted then too:
 *     the batch in flight goes on with the map it was submitted with, which stays on the device, and hands out its profile. */
int ffs_ctx_set_radial_bins(ffs_ctx *ctx, const uint16_t *bin_of_pixel, uint32_t n_bins);

/* n_iqr of the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE): how many interquartile ranges above its shell's median a strong pixel
 * stands.  Default 6 (DIALS's radial_profile.n_iqr).  Per context, kept across ffs_ctx_set_params; a batch takes it as it is at submit.
 * FFS_ERR_INVALID, state unchanged: n_iqr is not finite, below 0 or above 2^20 (the cutoff is a uint32).  (No counterpart in the reference.) */
int ffs_ctx_set_radial_threshold(ffs_ctx *ctx, double n_iqr);

/* The blur of the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE): a small smoothing of the image ahead of the threshold, DIALS's
 * radial_profile.blur = narrow | wide ("to reduce noise peaks and to combine split spots").  Everything is integers.
 *   Weights, separable, w(dx, dy) = w1(dx) * w1(dy):  narrow w1 = (1, 2, 1), a 3 x 3 kernel of full weight 16 (DIALS's narrow kernel
 *   exactly);  wide w1 = (1, 4, 6, 4, 1), a 5 x 5 kernel of full weight 256 (the binomial of variance 1 in place of DIALS's 5 x 5 table of
 *   rounded Gaussian values: no parity with DIALS is claimed for it, as for the rest of this algorithm).
 *   A pixel is a TAP when it lies inside the image, its bit in the valid-pixel mask (as it stands at submit) is set, p <= max_valid when
 *   max_valid >= 0 (both scopes), and for 32-bit pixels p < 2^24.  The bin map plays no part for taps.  A pixel COUNTS in shell b when it
 *   is a tap and its bin entry is b, not 0xFFFF: the rule of FFS_ALGO_RADIAL_PROFILE.
 *   For a counting pixel at (x, y):  S = sum of w(dx, dy) * p(x + dx, y + dy) and Wn = sum of w(dx, dy), both over the offsets of the
 *   kernel whose pixel is a tap (Wn is at least the centre's weight), and v = floor(S / Wn).  Masked pixels, overloads and the image
 *   border leave the sum and the weight together: a constant patch keeps its value right up to a module gap or the image edge.
 *   S <= 256 * (2^24 - 1) = 4 294 967 040 fits 32 unsigned bits.
 *   With a blur, v takes the place of p in everything the algorithm decides: the histogram of one-count bins 0..255 and a tail (v >= 256),
 *   hence n_pixels, n_overflow, the quartiles, the status and the cutoff of every ffs_radial_shell, and the strong test.  A pixel is
 *   STRONG when it counts in shell b, b's status is 0, v > cutoff[b], (double)v > ffs_params.threshold, and p >= 1: a zero pixel beside a
 *   bright one can have v > cutoff, and the peak search and the centroid division behind the strong plane rely on a strong pixel's
 *   intensity being at least 1 (ffs_stack3d_add_slice).
 *   Everything behind the strong plane reads the raw pixels and is what it is for any strong plane: lists, intensities, boxes,
 *   reflections, the byte mask, the 3D stack, spot backgrounds; so do the radial profile of the batch and the pixel statistics.
 * FFS_RADIAL_BLUR_NONE is the default.  Per context, kept across ffs_ctx_set_params, accepted under any algorithm and at any time; it
 * plays a part only under FFS_ALGO_RADIAL_PROFILE.  A batch takes it as it stands at submit, and keeps it when ffs_wait runs it again;
 * ffs_stream_last_path reports FFS_PATH_RADIAL_BLUR for a batch whose threshold ran blurred.  ffs_params keeps its layout.
 * FFS_ERR_INVALID, state unchanged (ffs_last_error has the text): any other value.  (No counterpart in the reference.) */
#define FFS_RADIAL_BLUR_NONE 0
#define FFS_RADIAL_BLUR_NARROW 1
#define FFS_RADIAL_BLUR_WIDE 2
int ffs_ctx_set_radial_blur(ffs_ctx *ctx, int blur);

/* Per-pixel statistics over a run: count, sum, sum of squares and maximum of every pixel over all frames the context sees -- what a
 * valid-pixel mask (dead pixels: mean 0; hot pixels: a mean far above the neighbours'), a gain map (variance / mean over a flat run) and
 * the maximum image of a serial run (the "virtual powder pattern") are made from; dxtbx.image_average produces the same three images on
 * the host.  The reference has no counterpart.  Accumulated on the device from the frames a batch has there anyway.
 *   While accumulation is on, every frame of every batch submitted on the context -- through ffs_submit, ffs_submit_device,
 *   ffs_submit_compressed or ffs_submit_encoded, on any of its streams -- is folded into four W x H accumulators.
 *   A pixel value p of a frame COUNTS at (x, y) when both of these hold:
 *     - p <= max_valid when ffs_params.max_valid >= 0 for that batch, under both scopes of max_valid;
 *     - for 32-bit pixels, p < 2^24 (the rule of the radial profile).
 *   Unlike the radial profile, the valid-pixel mask plays no part: the statistics are what a mask is made from, so masked pixels are in them.
 *   Per pixel:
 *     count  (uint32) the number of frames in which the pixel counted;
 *     sum    (uint64) the sum of p over those frames;
 *     sum_sq (uint64) the sum of p*p over them, taken modulo 2^64: it can wrap only for 32-bit pixels, and only after more than 65 536
 *            frames near 2^24;
 *     max    (uint32) the largest counted p; 0 when count is 0.
 *   Per context: n_frames (uint64), the frames folded in since the last start; n_frames - count is how often a pixel was above the limit.
 *   All of these are integers: the result is bit for bit independent of batch size, stream, order, path and tuning.
 *   The result is state of the CONTEXT, accumulated across batches and across all of its streams, not an output of a batch.  A batch takes
 *   the on / off state as it is at submit.  A batch that ffs_wait runs again (all of it, or single frames) counts once.  ffs_decode_only*
 *   and the ffs_bench_* entries fold nothing in, except ffs_bench_pixel_stats -- and ffs_bench_pipeline, which IS ffs_submit_device and
 *   ffs_wait in a loop and folds as they do (how the cost of accumulating is measured in the pipeline).  If a batch's ffs_wait fails (a corrupt chunk, say) the
 *   statistics are undefined: start again.
 * Modes:
 *   FFS_PIXEL_STATS_OFF     stop; the accumulated values stay readable.  Accepted at any time: a batch in flight that was submitted
 *                           under "on" still counts.
 *   FFS_PIXEL_STATS_START   allocate on first use, zero all four planes and n_frames, on.
 *   FFS_PIXEL_STATS_RESUME  on, values kept (START if never started).
 * The accumulators are 24 bytes per pixel (434 MB on Eiger-16M), allocated at the first start and freed with the context; a failed
 * allocation is FFS_ERR_NOMEM.
 * FFS_ERR_INVALID, state unchanged (ffs_last_error has the text):
 *   - any other mode;
 *   - START (or a RESUME that is one) while any stream of the context has a batch between submit and ffs_wait. */
#define FFS_PIXEL_STATS_OFF 0
#define FFS_PIXEL_STATS_START 1
#define FFS_PIXEL_STATS_RESUME 2
int ffs_ctx_set_pixel_stats(ffs_ctx *ctx, int mode);

/* Copies the statistics out: each of the four pointers is caller-owned, dense, W*H entries, row-major, and may be NULL (that plane is
 * not copied); n_frames is always written.  Complete for every batch ffs_wait has returned: FFS_ERR_INVALID, nothing written, before any
 * start and while any stream of the context has a batch in flight.  Accumulation may be on or off, and stays as it is. */
typedef struct {
    uint64_t n_frames;   /* out */
    uint32_t *count;
    uint64_t *sum;
    uint64_t *sum_sq;
    uint32_t *max;
} ffs_pixel_stats;
int ffs_ctx_get_pixel_stats(ffs_ctx *ctx, ffs_pixel_stats *out);

/* Jungfrau pedestals from dark frames: what the pedestal planes of ffs_ctx_set_jungfrau_calibration are measured from.  Before a
 * collection the detector takes a few thousand dark frames in G0, then forced into G1, then into G2; these entries fold the raw words of
 * such frames into per-pixel, per-stage accumulators on the device (2 bytes a pixel cross PCIe, as for data) and turn the accumulators
 * into pedestal, noise and "usable" planes.  The per-pixel statistics above cannot do this: they would add the gain bits into the value
 * and mix the stages.  The rule is stated once, in csrc/jungfrau_pedestal_model.hpp, and compiled by the kernel, this library's host
 * function, the driver and a CPU check.  The reference has no counterpart.
 *   FOLD.  A frame is W*H little-endian 16-bit words.  A word r at flat pixel k that is invalid by itself -- gain code 2, 0xFFFF, 0xC000 --
 *   counts nowhere.  Otherwise, with the stage s = 0, 1, 2 for the gain codes 0, 1, 3 and a = r & 0x3FFF:
 *     count[s][k] += 1 (uint32), sum[s][k] += a (uint64), sum_sq[s][k] += a*a (uint64); per context n_frames += 1 per frame.
 *   The word decides the stage: a run needs no label, one accumulator set takes G0, G1 and G2 frames in any order, and no calibration
 *   plays a part.  Nothing can wrap while n_frames < 2^32.  All integers: the result is bit for bit independent of batch size, stream,
 *   thread and order.
 *   PLANES.  One stage of one pixel, c = count: c == 0 gives pedestal 0, rms 0, ok 0.  Otherwise in float64, each operation rounded on its
 *   own: m = (double)sum / (double)c, q = (double)sum_sq / (double)c, v = q - m*m, pedestal = (float)m, rms = (float)sqrt(v > 0 ? v : 0),
 *   ok = c >= min_frames && (max_rms == 0 || rms <= max_rms).  Bit for bit the NumPy float64 / float32 rule.
 *   A RE-PEDESTALLED CALIBRATION takes these pedestal planes and keeps factor[s][k] where ok[s][k] holds, 0 ("no calibration") elsewhere
 *   (the driver's --jungfrau-pedestal and `ffs_hosttool jfrepedestal` write it).
 *
 * ffs_ctx_jungfrau_pedestal_begin: allocates the accumulators on first use (60 bytes a pixel, 566 MB on Jungfrau-9M; FFS_ERR_NOMEM when
 * that fails), zeroes them and n_frames.  Calling it again starts again.
 * ffs_ctx_jungfrau_pedestal_end: frees them; idempotent (FFS_OK when there are none).  They also go with the context.
 * FFS_ERR_INVALID, state unchanged: a context of pixel_bytes 2 (begin; as for the calibration, raw words belong to 32-bit contexts);
 * while any stream of the context has a batch or a fold in flight (both). */
int ffs_ctx_jungfrau_pedestal_begin(ffs_ctx *ctx);
int ffs_ctx_jungfrau_pedestal_end(ffs_ctx *ctx);

/* Folds n_frames dark frames into the context's accumulators.  chunks[i] is exactly width*height 16-bit little-endian words, placed as
 * for FFS_CODEC_JUNGFRAU_RAW: anywhere, or all of them inside the stream's host buffer at offsets that are multiples of 16.
 * SYNCHRONOUS: on return the frames are in the accumulators, and the caller has its memory and the stream's host buffer back.
 * ms_fold may be NULL; otherwise it receives the duration of the fold launch (one per 64 frames; of all of them together) from HIP events
 * on the dispatches.  The fold needs no calibration, runs no conversion, no threshold and no sparse stage, and leaves
 * ffs_stream_last_path, ffs_stream_timings, the pixel statistics, the radial profile and the results of the batches before and after it
 * untouched.  It stages its chunks where an encoded batch stages them and writes nowhere else on the stream: the frames of the last
 * waited batch stay where they are, so ffs_stream_spot_backgrounds REMAINS AVAILABLE after a fold on its stream and gives what it gave
 * before it.
 * Folds on different streams of one context may be called from different threads at once: the library keeps their launches on the
 * accumulators apart (one HIP stream of the context, one launch behind the other), and the result does not depend on their order.
 * FFS_ERR_INVALID, each with a text of its own, nothing folded and the state unchanged: a NULL stream, chunks or chunk_bytes; no
 * accumulators (before ffs_ctx_jungfrau_pedestal_begin, after _end); a batch in flight on the stream; n_frames outside 1..max_batch; a
 * NULL chunk or one of any size other than width*height*2; chunks partly inside the stream's host buffer; a chunk inside it at an
 * offset that is not a multiple of 16; a fold that would take n_frames past 2^32 - 1. */
int ffs_stream_jungfrau_pedestal_fold(ffs_stream *s, const void *const *chunks, const size_t *chunk_bytes,
                                      uint32_t n_frames, float *ms_fold);

/* Copies the accumulators out: each of the nine pointers is caller-owned, dense, W*H entries, row-major, and may be NULL (that plane is
 * not copied); n_frames is always written.  Every fold that has returned is in them.  FFS_ERR_INVALID, nothing written: NULL out; no
 * accumulators (before begin, after end); while any stream of the context has a batch or a fold in flight. */
typedef struct {
    uint64_t n_frames;   /* out (ffs_ctx_get_jungfrau_pedestal); not read by ffs_jungfrau_pedestal_planes */
    uint32_t *count[3];
    uint64_t *sum[3];
    uint64_t *sum_sq[3];
} ffs_jungfrau_pedestal_stats;
int ffs_ctx_get_jungfrau_pedestal(ffs_ctx *ctx, ffs_jungfrau_pedestal_stats *out);

/* The PLANES rule above on the host: no context, no GPU.  stats: nine planes of n_px entries, all needed.  pedestal[s], rms[s], ok[s]:
 * n_px entries each; the three arrays of pointers must be given, any pointer in them may be NULL (that plane is not written).
 * min_frames >= 1; max_rms finite and >= 0, 0 = no noise test.  FFS_ERR_INVALID, nothing written (ffs_last_error(NULL) has the text):
 * NULL stats, a NULL plane in it, a NULL pedestal, rms or ok array; min_frames 0; a negative, infinite or NaN max_rms. */
int ffs_jungfrau_pedestal_planes(const ffs_jungfrau_pedestal_stats *stats, size_t n_px, uint32_t min_frames, float max_rms,
                                 float *const pedestal[3], float *const rms[3], uint8_t *const ok[3]);

/* Selects between paths that give the SAME results (A/B partners, fall-backs, capacities that tests shrink) --
 * per context, never through the environment; nothing here can change a result.  Keys (default):
 *   "threshold_path"   (0) 0 = windows the streaming kernel cannot vouch for go onto a list (fix-up kernel),
 *                          1 = they are marked in the plane and an exact kernel filters it (also the fall-back
 *                          when that list overflows), 2 = no streaming kernel at all: the window of EVERY valid pixel is
 *                          gathered from memory and decided by the exact kernel (~10 ms per Eiger frame: the independent
 *                          partner `spotfinder --validate` compares the hot path with, spotfinder.cc:1012-1053)
 *   "ext_first_pass"   (2) extended algorithm, 16-bit pixels: 2 = streaming kernel, 0 = plain one-pixel-per-lane kernel
 *   "sparse_stage"     (2) one launch per batch, a workgroup per frame: 3 = always, 2 = unless the stream's previous batch
 *                          held a frame with more strong pixels than that workgroup's LDS holds; 1 = four grid-wide kernels
 *   "device_lists"     (2) a batch leaves its strong-pixel lists on the device: 1 = always, 0 = only when the host asked for them
 *                          (want_strong_list), 2 = also while a 3D stack of the process is alive (ffs_stack3d_add_batch reads them:
 *                          create the stack before submitting).  Without them the sparse launch saves two scattered stores per pixel
 *   "strong_log"       (1) 16-bit standard path: the streaming kernel appends its strong groups to per-wave logs which the
 *                          one-launch sparse stage merges (dense stores; the kernel's time no longer depends on where the
 *                          stream's buffers lie); 0 = plane bytes, counters and an occupancy bitmap as in rounds 1-3b
 *   "chain_runs"       (1) with "sparse_stage" 2: such dense batches of 16-bit frames stay in the one launch, its union-find
 *                          over runs of strong pixels instead of pixels (up to 16384 runs per frame); 0 = they take the grid-wide kernels;
 *                          2 = every frame of 16-bit pixels goes over runs (A/B partner: no faster on sparse frames)
 *   "sparse_bands"     (1) standard path with wave logs when nobody reads the pixel lists or the byte mask: the sparse stage in small
 *                          workgroups -- a wave per band of a frame, then a merge per frame (round 5) -- instead of the one workgroup per
 *                          frame, which holds a whole CU: 1 = with one or with four and more batches in flight, and always on a context with
 *                          four or more streams (where it measures faster), 2 = always, 0 = never.  A band beyond its plan (768 strong pixels, 256 components) sends the batch back
 *                          through the one-workgroup launch inside ffs_wait
 *   "wait_ahead"       (1) a thread of the context turns each batch's records into the result arrays as soon as the GPU has finished
 *                          it, so ffs_wait finds them ready (0: ffs_wait does it, as in rounds 1-4)
 *   "stream_prio"      (1) bit 1: the 16-bit streaming kernel's waves run at issue priority 3 (s_setprio), ahead of the band waves on their
 *                      SIMDs; bit 2: the band and merge waves do (measured slower: DESIGN.md section 3.4c); 0..3
 *   "dense_overlap"    (0) 1 = consecutive streaming kernels of the wave-log path on two HIP streams, handed over by a value the launch's
 *                          last workgroup writes as it starts (hipStreamWaitValue32) instead of the queue's barrier between two dispatches;
 *                          works in isolation, measured 8-10 % slower in the pipeline: off, kept as the A/B partner
 *   "sparse_priority"  (0) priority of the context's two sparse HIP streams: 0 = highest, 1 = lowest, 2 = the dense stream's (before
 *                          the first stream is created; measured: 0 and 1 alike, 2 costs 15 %)
 *   "sched"            (3) 3 = shared dense / sparse / upload HIP streams per context, 0 = one per ffs_stream
 *                          (before the first stream is created)
 *   "direct_records"   (1) records written straight into pinned host memory (before the first stream is created)
 *   "chain_first" (2), "bright_cap" (2^20), "frames_per_group", "target_waves" (16384), "stream_bands" (0: from target_waves; > 0: that many bands, any number), "dense_mask" (0),
 *   "occupancy_bitmap" (1), "decode_in_dense_stream" (1), "rows_ahead" (3: rows of loads a streaming wave keeps in flight), "ccl_grid" (32),
 *   "window_kernel"    (0) 0 = the general-window threshold kernel (any kernel_half_x / _y in 1..7, exact sums, the oracle's float64
 *                          predicate) runs only for windows other than 3,3; 1 = it runs for every window, 3,3 included (the A/B and
 *                          cross-check partner of the 7x7 streaming kernels: same results)
 *   "radial_stream"    (0) the radial profile's two launches (ffs_ctx_set_radial_bins): 0 = in the batch's sparse stream behind its sparse
 *                          launch, 1 = in the dense stream behind the threshold stage's kernels (measured 11 % slower in the pipeline: the A/B partner).
 *                          1 is taken as 0 where there is no dense stream to tell from the sparse one ("sched" 0: one HIP stream per
 *                          ffs_stream) and under "dense_overlap" 1 (the stage's kernel may be in the dense stream's partner)
 *   "stats_stream"     (0) the per-pixel statistics' launch (ffs_ctx_set_pixel_stats): 0 = in a HIP stream of the context's own, beside the
 *                          batch's threshold stage, 1 = in the dense stream behind the threshold stage's kernels (the A/B partner).  1 is taken
 *                          as 0 under "sched" 0 and under "dense_overlap" 1, where the dense stream is not one stream for the whole context.
 *                          Accepted only while no batch of the context is in flight
 *   "radial_map8"      (0) the radial profile reads a bin map of at most 255 bins in one byte an entry (1) instead of two (0): DESIGN.md section 3.6
 *                          has the measurement
 *   "radthr_bands"     (0) the radial-profile threshold's histogram launch: 0 = the launch chooses its bands of rows per frame, > 0 = that many,
 *                          clamped to 1..H, each ceil(H / bands) rows tall (tests put the band seams where they want them)
 *   "radthr_form"      (0) ... and how a lane's counts meet the workgroup's table in LDS: 1 = one add per counting pixel, 2 = a run of equal
 *                          (shell, value) pairs kept in registers, 0 = the one that measured faster for the pixel size (2 for 16-bit
 *                          pixels, 1 for 32-bit: DESIGN.md section 3.8c)
 *   "assembly_threads" (7: helper threads that build a batch's result arrays; 3, 12 and 15 measure the same): see DESIGN.md.
 *   "band_taper" (0), "ext_rest_aside" (0), "ext_fused" (0): round 4's A/B partners (tapered bands of the streaming kernels;
 *                          extended algorithm: erosion + final pass in the sparse stream / fused into one kernel) -- measured, no
 *                          gain, off (DESIGN.md sections 3.2c, 4)
 *   "ext_erode"        (2) extended algorithm, the erosion kernel: 2 / 1 = a wave per 62 word columns of the bit plane and 16 / 32
 *                          rows (one load per row and lane, all in flight, neighbours' words by DPP, XCD-aware block map), 0 = round 1's
 *                          kernel (a lane per word column, three loads per row); "ext_e_sparse" (0): 1 = the signal-region plane is
 *                          cleared behind the previous batch and only its non-zero words are stored (measured: the fill costs the
 *                          first pass more than the stores cost the erosion)
 * The reference has no counterpart (its launch wrapper has one path, spotfinder/spotfinder.cu:148-189). */
int ffs_ctx_set_tuning(ffs_ctx *ctx, const char *key, long long value);

/* ---- streams: one in-flight batch each (replaces one worker thread's CudaStream +
 *      pinned/device buffers, spotfinder.cc:729-742) --------------------------------------------
 * An ffs_stream owns its buffers and its batch; the HIP streams underneath belong to the context (one for
 * the dense kernels of all its ffs_streams, in submission order, two for the sparse launches, one for uploads:
 * DESIGN.md section 3.4).  Distinct ffs_streams may be driven from distinct threads at the same time; keep
 * two or more batches in flight (two or more ffs_streams) for throughput -- a batch's sparse stage runs beside
 * the next batch's threshold kernel. */
int ffs_stream_create(ffs_ctx *ctx, ffs_stream **out);
/* Waits for the stream's batch in flight, if any, and frees its buffers (idempotent: see ffs_ctx_destroy). */
void ffs_stream_destroy(ffs_stream *s);

/* The stream's pinned staging area (max_batch dense frames): decode straight into it, as the
 * reference's workers decompress into their pinned host_image (spotfinder.cc:731, :828-842),
 * then pass the same pointer to ffs_submit(). */
int ffs_stream_host_buffer(ffs_stream *s, void **ptr, size_t *bytes);
/* The staging area is pinned memory, which costs ~170 ms per GB to allocate (and the runtime serialises the
 * allocations of all threads): it is allocated on first use, max_batch raw frames by default.  A producer of
 * compressed chunks that knows it needs less (max_batch chunks, not max_batch frames) says so BEFORE its first
 * ffs_stream_host_buffer(); a later call with a larger size grows the area (contents are not kept; not while a
 * batch is in flight).  Staging areas of destroyed streams are reused by the context's next streams. */
int ffs_stream_reserve_host(ffs_stream *s, size_t bytes);

/* cudaMemcpy2DAsync H2D + call_do_spotfinding_dispersion + D2H + ConnectedComponents
 * (spotfinder.cc:846-905), for n_frames dense host frames (each W*H pixels, consecutive).
 * Asynchronous; results are collected with ffs_wait(). */
int ffs_submit(ffs_stream *s, const void *host_pixels, uint32_t n_frames,
               int64_t first_frame_id);
/* Same, frames already in device memory (rows pitch_bytes apart, frames frame_stride_bytes
 * apart; pitch_bytes a multiple of 16).  For producers that decode on the GPU, and for bench.py's
 * resident-in-HBM measurement.  The pixels must stay valid and unchanged until ffs_wait() has returned
 * (a frame that exceeds the stream's list capacity is read a second time there). */
int ffs_submit_device(ffs_stream *s, const void *device_pixels, size_t pitch_bytes,
                      size_t frame_stride_bytes, uint32_t n_frames, int64_t first_frame_id);
/* Device layout this context prefers for ffs_submit_device (and uses internally). */
int ffs_ctx_device_layout(const ffs_ctx *ctx, size_t *pitch_bytes, size_t *frame_stride_bytes);

/* Blocks until the stream's batch is done; results[i] describes frame i of the batch. */
/* Same as ffs_submit, but each frame arrives as the raw bitshuffle-LZ4 chunk the detector wrote
 * (12-byte header + blocks: what Reader::get_raw_chunk returns, h5read.c:428-456, shmread.cc) and is
 * decoded on the GPU -- replaces bshuf_decompress_lz4 on the worker thread (spotfinder.cc:823-842,
 * h5read/src/read_chunks.cc:22-24) and moves 4-6x fewer bytes over PCIe.  chunks[i] may point
 * anywhere (copied into the stream's pinned staging buffer) or, for zero copy, inside the buffer
 * ffs_stream_host_buffer returns (then all of them must).  The call starts the PCIe copy and returns;
 * a helper thread of the stream indexes the blocks and enqueues the kernels meanwhile (ffs_wait
 * joins it).  A chunk whose header does not say width*height*pixel_bytes is refused here
 * (FFS_ERR_INVALID); block lengths that run past chunk_bytes[i] and corrupt LZ4 streams are
 * reported by ffs_wait (FFS_ERR_INVALID). */
int ffs_submit_compressed(ffs_stream *s, const void *const *chunks, const size_t *chunk_bytes,
                          uint32_t n_frames, int64_t first_frame_id);
/* Decode only, for tests and benchmarks: n_frames chunks -> the stream's device image buffer
 * (default layout); the average duration of one decode launch in ms_decode (HIP events, iters
 * launches).  host_out (may be NULL) receives the decoded frames, W*H*pixel_bytes each. */
int ffs_decode_only(ffs_stream *s, const void *const *chunks, const size_t *chunk_bytes,
                    uint32_t n_frames, uint32_t iters, float *ms_decode, void *host_out);

/* The two entries above for any codec of the frames' chunks.
 * FFS_CODEC_BSLZ4: exactly ffs_submit_compressed / ffs_decode_only.
 * FFS_CODEC_BYTE_OFFSET: miniCBF (Pilatus) frames.  chunks[i] is the binary section as it lies in the file -- everything behind the
 * 0c 1a 04 d5 marker to the end of the file, what CBFRead::get_raw_chunk returns: no header, and bytes behind the last element
 * (padding, the MIME trailer), which are ignored -- and is decoded on the GPU into the context's pixel type: replaces
 * decompress_byte_offset on the reading thread (cbfread.hpp:49-106, called from CBFRead::get_image) and the upload of the raw
 * frame (spotfinder.cc:846-862).  Placement as for ffs_submit_compressed (anywhere, or all of them inside the stream's host
 * buffer).  A chunk shorter than width*height bytes cannot hold a frame and is refused here (FFS_ERR_INVALID, "byte-offset ...");
 * a chunk that ends before its last element is reported by ffs_wait / ffs_decode_only_encoded (FFS_ERR_INVALID, "corrupt
 * byte-offset chunk"), its missing pixels are zeros.
 * FFS_CODEC_JUNGFRAU_RAW: frames as a Jungfrau delivers them.  chunks[i] is exactly width*height 16-bit little-endian words, dense and
 * row-major -- two bits of gain stage, 14 bits of ADC -- and is converted on the GPU into 32-bit photon counts with the context's
 * calibration (ffs_ctx_set_jungfrau_calibration, which has the rule): 2 bytes a pixel cross PCIe instead of the 4 of a frame converted
 * on the host.  One launch per batch of up to 64 frames.  Placement as for ffs_submit_compressed.  Refused here (FFS_ERR_INVALID, each
 * with a text of its own, state unchanged): a chunk of any other size; a context of pixel_bytes 2; a context without a calibration; a
 * chunk that lies in the stream's host buffer at an offset that is not a multiple of 16 (the words are loaded 16 bytes at a time).
 * Any other codec: FFS_ERR_INVALID. */
#define FFS_CODEC_BSLZ4 0        /* what ffs_submit_compressed / ffs_decode_only take */
#define FFS_CODEC_BYTE_OFFSET 1  /* CBF byte-offset, cbfread.hpp:49-106; chunk = bytes after the binary marker */
#define FFS_CODEC_JUNGFRAU_RAW 2 /* raw Jungfrau words (gain stage << 14 | ADC); chunk = width*height*2 bytes */
int ffs_submit_encoded(ffs_stream *s, int codec, const void *const *chunks, const size_t *chunk_bytes,
                       uint32_t n_frames, int64_t first_frame_id);
/* ffs_decode_only for any codec (byte-offset: the three decode launches of kernels_byteoffset.hpp are timed together) --
 * the GPU's side of what cbfread.hpp:49-106 does per frame. */
int ffs_decode_only_encoded(ffs_stream *s, int codec, const void *const *chunks, const size_t *chunk_bytes,
                            uint32_t n_frames, uint32_t iters, float *ms_decode, void *host_out);

/* (ffs_wait turns the batch's records into the arrays below; for large batches the frames are spread over the calling thread and
 * three helper threads that belong to the context -- created on first use, joined by ffs_ctx_destroy.) */
int ffs_wait(ffs_stream *s, const ffs_frame_result **results, uint32_t *n_results);

/* The whole batch's boxes and reflections as two contiguous arrays (frame i's slice starts
 * where frame i-1's ends; lengths are results[i].n_boxes / .n_reflections) -- lets a binding
 * wrap a batch without touching every frame. */
int ffs_stream_batch_arrays(ffs_stream *s, const ffs_box **boxes, uint32_t *n_boxes,
                            const ffs_reflection **reflections, uint32_t *n_reflections);

/* Timings of the last completed batch on this stream, milliseconds (HIP events on the
 * stream): [0] H2D, [1] threshold kernels, [2] compaction + connected components,
 * [3] D2H, [4] total.  (The reference prints Copy/Kernel/Post Copy/Post, spotfinder.cc:1056-1076.) */
int ffs_stream_timings(ffs_stream *s, float ms[5]);

/* Which launches the stream's last batch took -- for tests and tools that must know that the path they mean to exercise ran
 * (results never depend on it): a mask of the bits below; *reruns = how many times ffs_wait ran the batch again because a plan
 * did not hold it (list / component capacity, LDS forests, wave logs, band plan).  Either pointer may be NULL.
 * (The reference has one path: spotfinder/spotfinder.cu:148-189 + the host's ConnectedComponents.) */
#define FFS_PATH_WAVE_LOGS 1u      /* the streaming kernel's strong groups travelled in per-wave logs, not the bit plane */
#define FFS_PATH_FRAME_CHAIN 2u    /* sparse stage: one launch, a workgroup per frame */
#define FFS_PATH_BANDS 4u          /* sparse stage: a wave per band of a frame + a merge per frame */
#define FFS_PATH_RUNS 8u           /* ... the one launch's forest over runs of strong pixels (dense frames) */
#define FFS_PATH_GRID_KERNELS 16u  /* sparse stage: four grid-wide kernels */
#define FFS_PATH_EXTENDED 32u      /* extended dispersion */
#define FFS_PATH_WINDOW 64u        /* the general-window threshold kernel (a window other than 3,3, or tuning "window_kernel" = 1) */
#define FFS_PATH_RADIAL 128u       /* the batch computed a radial profile (ffs_ctx_set_radial_bins) */
#define FFS_PATH_PIXEL_STATS 256u  /* the batch was folded into the per-pixel statistics (ffs_ctx_set_pixel_stats) */
#define FFS_PATH_RADIAL_THRESHOLD 512u /* the radial-profile threshold decided the strong pixels (FFS_ALGO_RADIAL_PROFILE; no counterpart in the reference) */
#define FFS_PATH_RADIAL_BLUR 1024u /* ... on the blurred image (ffs_ctx_set_radial_blur narrow or wide) */
int ffs_stream_last_path(ffs_stream *s, uint32_t *path_bits, uint32_t *reruns);

/* The radial profile (ffs_ctx_set_radial_bins) of frame `frame_in_batch` of the last batch ffs_wait returned on this stream: n_bins
 * entries each, complete when ffs_wait returns.  The pointers stay valid until the next ffs_wait on the stream, like the pointers in
 * ffs_frame_result (the stream's next batch may be in flight meanwhile).  FFS_ERR_INVALID: that batch was submitted without a map;
 * frame_in_batch is out of range; a dead handle. */
typedef struct {
    uint32_t n_bins;
    const uint32_t *count;
    const uint64_t *sum;
    const uint64_t *sum_sq;
} ffs_radial_profile;
int ffs_stream_radial_profile(ffs_stream *s, uint32_t frame_in_batch, ffs_radial_profile *out);

/* What the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE) decided per shell of frame `frame_in_batch` of the last batch ffs_wait
 * returned on this stream: *n_bins records, one per bin of the map the batch was submitted with, complete when ffs_wait returns and valid
 * until the next ffs_wait on the stream (two pinned host buffers take turns, as for the profile).  The fields are FFS_ALGO_RADIAL_PROFILE's.
 * FFS_ERR_INVALID: that batch did not run this algorithm; frame_in_batch is out of range; a dead handle.  (No counterpart in the
 * reference: it has no such algorithm.) */
#define FFS_RADIAL_THR_OK 0u
#define FFS_RADIAL_THR_EMPTY 1u
#define FFS_RADIAL_THR_OVERFLOW 2u
typedef struct {
    uint32_t n_pixels;            /* N, the shell's counting pixels */
    uint32_t n_overflow;          /* ... those at or above 256 */
    int32_t q1, median, q3;       /* -1 under a status other than FFS_RADIAL_THR_OK */
    uint32_t cutoff, status, reserved;
} ffs_radial_shell;               /* 32 bytes */
int ffs_stream_radial_thresholds(ffs_stream *s, uint32_t frame_in_batch, const ffs_radial_shell **out, uint32_t *n_bins);

/* The per-spot background and what a background-subtracted intensity needs: for every reflection of the last batch ffs_wait returned on
 * this stream, a constant background level estimated from the ring of pixels around its bounding box, with Tukey's fence against
 * outliers.  The model is the constant background of the reference's integrator (include/integrator/background.hpp,
 * tukey_constant_background: an integer histogram of 256 one-count bins and a high tail, quartiles by 1-based position, rejection
 * outside q1 - 1.5 IQR .. q3 + 1.5 IQR, no estimate when the tail or the fence says the range is too small), restated in integers; it
 * assumes photon counts, as the reference's header says, and applies no gain.  The reference runs it over a 3D shoebox at integration
 * time; here it runs over a 2D ring at spot-finding time, on the device, where the pixels are.
 *   Ring.  For a reflection with bounding box x_min..x_max, y_min..y_max in its frame and a border b in 1..16: the pixels of
 *   [x_min - b, x_max + b] x [y_min - b, y_max + b], clipped to the image, that lie OUTSIDE the bounding box.  The spot's own box
 *   contributes nothing (its non-strong tails are not background); a neighbour's strong pixels that fall into the ring stay in it
 *   (rejecting them is the model's job).
 *   A ring pixel p is VALID when all of these hold (the rules of the radial profile):
 *     - its bit in the context's valid-pixel mask is set -- the mask as it stands at the call, ffs_ctx_apply_resolution_mask included;
 *     - p <= max_valid when the batch's ffs_params.max_valid >= 0, under both scopes of max_valid;
 *     - for 32-bit pixels, p < 2^24.
 *   From the valid ring pixels, in integers:
 *     n_pixels = N, their number; n_overflow = those with p >= 256.
 *     status, decided in this order:
 *       FFS_SPOT_BG_NO_PIXELS (1)   N = 0;
 *       FFS_SPOT_BG_OVERFLOW (2)    4 * n_overflow > N: too much of the ring lies above the histogram;
 *       otherwise q1, median, q3 = the values at the 1-based sorted positions (N + 3) / 4, (N + 1) / 2, (3 N + 1) / 4 (integer
 *       division); all three are below 256 then.  With iqr = q3 - q1:
 *       FFS_SPOT_BG_RANGE (3)       2 * q3 + 3 * iqr >= 512: the upper fence reaches the end of the histogram;
 *       otherwise the inliers are the pixels with 2 * q1 - 3 * iqr <= 2 * p <= 2 * q3 + 3 * iqr and p < 256; n_inliers is their
 *       number and inlier_sum their sum;
 *       FFS_SPOT_BG_NO_INLIERS (4)  there are none.  Cannot be reached once 1-3 are excluded (the bin of q1 is never empty and always
 *                                   inside the fence); kept for parity with the reference's order of checks;
 *       FFS_SPOT_BG_OK (0)          else.
 *     Under status 1 and 2 the quartiles are -1.  Under any non-zero status n_inliers = inlier_sum = 0.
 *     mean (float64) = (double)inlier_sum / (double)n_inliers, divided on the host; 0 when status != 0.
 *   Everything up to that division is integer arithmetic: the result is exact, bit for bit, and independent of path, tuning and order.
 *   A background-subtracted intensity is sum_intensity - num_pixels * mean (the reflection's fields); its variance under Poisson
 *   statistics is sum_intensity + num_pixels^2 * mean / n_inliers.
 * One entry is written per reflection of the batch, in the order and with the per-frame slices of ffs_stream_batch_arrays: frame i's slice
 * starts where frame i-1's ends and is results[i].n_reflections long (the reflections left after both filters).  *out stays valid until
 * the next call of this function or the next ffs_wait on the stream.  kernel_ms may be NULL; otherwise it receives the kernel's time from
 * HIP events on its dispatch (0 when nothing was launched).  A batch with no reflections: FFS_OK, *n = 0, nothing is launched.
 * The call is synchronous -- it launches in a HIP stream of the ffs_stream's own, waits and returns -- and belongs between ffs_wait and the
 * stream's next submit.  It reads the reflections ffs_wait handed out and the frames where the batch left them, so it sees the final
 * records whatever path, re-run or one-frame recovery produced them, and:
 *   - for an ffs_submit_device batch the caller's frames must still be where they were at submit, unchanged;
 *   - the context's mask must not have been replaced since the batch (the ring is judged by the mask as it stands at the call);
 *   - ffs_decode_only* on the stream decodes into the stream's frame buffer: after it the call is refused until the next ffs_wait.
 * FFS_ERR_INVALID (ffs_last_error names the reason): a dead handle; NULL out or n; border outside 1..16; no batch waited on the stream
 * yet, or the last ffs_wait on it failed; a batch in flight on the stream (its frames replace the last batch's); the last batch was
 * submitted without want_reflections. */
#define FFS_SPOT_BG_OK 0u
#define FFS_SPOT_BG_NO_PIXELS 1u
#define FFS_SPOT_BG_OVERFLOW 2u
#define FFS_SPOT_BG_RANGE 3u
#define FFS_SPOT_BG_NO_INLIERS 4u
typedef struct {
    uint32_t n_pixels, n_overflow;
    int32_t q1, median, q3;
    uint32_t n_inliers;
    uint64_t inlier_sum;
    uint32_t status, reserved;
    double mean;
} ffs_spot_background;            /* 48 bytes */
int ffs_stream_spot_backgrounds(ffs_stream *s, uint32_t border, const ffs_spot_background **out, uint32_t *n, float *kernel_ms);

/* The same ring under the second model of the reference's integrator: the robust Poisson GLM with a constant mean (Parkhurst et al. 2016,
 * J. Appl. Cryst. 49, 1912; include/integrator/background.hpp, glm_constant_background; what DIALS calls `glm constant3d`).  It fits the
 * rings the Tukey fence has no answer for (FFS_SPOT_BG_RANGE): a Poisson(0.1) ring has q1 = q3 = 0 and a fence of 0..0.
 *   Ring, validity of a pixel, n_pixels = N and n_overflow: exactly those of ffs_stream_spot_backgrounds, from the same histogram of 256
 *   one-count bins and a counted tail.  status, decided in this order:
 *     FFS_SPOT_BG_NO_PIXELS (1)      N = 0;
 *     FFS_SPOT_BG_FEW_PIXELS (5)     N < 10;
 *     FFS_SPOT_BG_OVERFLOW (2)       4 * n_overflow > N;
 *     otherwise median = the value at the 1-based sorted position N / 2 + 1 (integer division; below 256 then), and
 *     the ALL-ZERO RING -- n_overflow = 0 and every counting pixel 0 -- is FFS_SPOT_BG_OK with mean = 0, beta = -inf, n_iter = 0.  It has
 *     no finite beta; the reference walks beta down some seventy steps and returns a mean near 1e-33 whose digits are rounding noise.  0
 *     is the maximum-likelihood mean and the limit of the fit; this is the one documented departure from the reference;
 *     otherwise beta = log(median, or 1 when the median is 0) and at most 100 steps of iteratively reweighted least squares with Huber's
 *     c = 1.345: mu = exp(beta), s = sqrt(mu), j1 = floor(mu - c s), j2 = floor(mu + c s); epsi1 = E[psi_c] and epsi2 of Poisson(mu) as
 *     the reference's glm_expectation forms them from the Poisson probabilities around j1 and j2; b = epsi2 mu^2 / s;
 *     U = sum over the pixels of (psi_c((p - mu) / s) - epsi1) mu / s, a pixel of the tail entering at psi = +c;
 *     delta = U / (N b); beta += delta; the loop ends when sqrt(delta^2 / max(beta^2, 1e-10)) < 1e-3, beta taken before the update;
 *     FFS_SPOT_BG_DEGENERATE (6)     inside the loop: mu or s not > 0, mu not < 512, b or delta not finite; after it: beta outside
 *                                    (-300, 300).  The bound mu < 512 is this library's, not the reference's: it bounds the Poisson sums
 *                                    at 600 terms and keeps exp(-mu) a normal number; with bins that end at 255 and at most a quarter of
 *                                    the ring clipped at +c no fit the reference accepts gets there.  No histogram tried reached 6;
 *     FFS_SPOT_BG_NOT_CONVERGED (7)  100 steps without meeting the tolerance (a ring of two levels far apart can cycle);
 *     FFS_SPOT_BG_OK (0)             else: mean = exp(beta).
 *   median is -1 under status 1, 2 and 5.  n_iter is the steps taken.  beta is the last value reached (0 under status 1, 2 and 5).  mean
 *   is 0 when status != 0.
 *   U is computed from four integers of the histogram's prefix sums (psi_c is -c up to j1, +c above j2, the residual between) and the
 *   probabilities by one recurrence t_k = t_(k-1) mu / k; every floating-point operation is + - * / sqrt floor or an integer conversion,
 *   exp and log included (csrc/spot_background_glm_model.hpp has its own), compiled without contraction.  So the record is the same,
 *   bit for bit, on the device and from the same header on a CPU (`ffs_hosttool spotbgglm`), and independent of path, tuning and order.
 *   Against the reference's own function the mean differs by rounding only (DESIGN.md section 3.8b has the measured figure).
 *   A background-subtracted intensity is sum_intensity - num_pixels * mean; the model puts all N ring pixels at the fitted mean, so the
 *   mean's variance is mean / N and the intensity's sum_intensity + num_pixels^2 * mean / n_pixels.
 * One entry per reflection of the batch, in the order and with the per-frame slices of ffs_stream_batch_arrays, as for
 * ffs_stream_spot_backgrounds; the device stores the whole record, the host computes nothing.  The result buffer is this call's own: *out
 * stays valid until the next call of THIS function or the next ffs_wait on the stream, so both models may be asked for one batch and both
 * pointers held.  kernel_ms may be NULL; a batch with no reflections: FFS_OK, *n = 0, nothing is launched.  The call is synchronous and
 * belongs between ffs_wait and the stream's next submit; what it reads, and what must still be in place (an ffs_submit_device batch's
 * frames, the context's mask, no ffs_decode_only* in between), is word for word ffs_stream_spot_backgrounds'.
 * FFS_ERR_INVALID (ffs_last_error names the reason and this entry point): a dead handle; NULL out or n; border outside 1..16; no batch
 * waited on the stream yet, or the last ffs_wait on it failed; a batch in flight on the stream; the last batch was submitted without
 * want_reflections. */
#define FFS_SPOT_BG_FEW_PIXELS 5u
#define FFS_SPOT_BG_DEGENERATE 6u
#define FFS_SPOT_BG_NOT_CONVERGED 7u
typedef struct {
    uint32_t n_pixels, n_overflow;
    int32_t median;
    uint32_t n_iter;
    uint32_t status, reserved;
    double beta, mean;
} ffs_spot_background_glm;        /* 40 bytes */
int ffs_stream_spot_backgrounds_glm(ffs_stream *s, uint32_t border, const ffs_spot_background_glm **out, uint32_t *n, float *kernel_ms);

/* Summation integration of predicted reflections' shoeboxes in Kabsch space: the stage of the reference's pipeline
 * that follows spot finding (integrator/kabsch.cu, integrator/integrator.cc), for a flat panel without parallax correction.  A job is a
 * table of shoeboxes on a context; every batch's frames are folded into it after their ffs_wait; at the end one record per shoebox gives
 * the foreground sum, the centroid moments, the background under one of the two models above, I = fg_sum - fg_count * b and its variance.
 * THE RULE is stated once, in csrc/shoebox_model.hpp, which the kernel, this library's host side and `ffs_hosttool shoebox` compile; no
 * parity with the reference's binaries (whose scalar type may be float) is claimed.  Every operation is an IEEE float64 + - * / sqrt in
 * the order written there, compiled without contraction:
 *   corner (cx, cy) -- integers, may lie outside the image: x = cx * pixel_size_mm[0], y = cy * pixel_size_mm[1],
 *     L_i = (D[3i]*x + D[3i+1]*y) + D[3i+2], s = (L / |L|) / wavelength;
 *   per reflection: e1 = normalized(cross(s1, s0)), e2 = normalized(cross(s1, e1)), len = |s1|, zeta = dot(rot_axis, e1);
 *   per corner: eps1 = dot(e1, s - s1) / len, eps2 = dot(e2, s - s1) / len;
 *   image n (0-based position in the scan): phi_low = (osc_start_deg + n * osc_width_deg) * (pi / 180), phi_high the same with n + 1,
 *     centre = phi_low <= phi <= phi_high;
 *   FFS_SHOEBOX_ELLIPSOID: a corner is foreground when (eps1^2 + eps2^2) / delta_b^2 + e3^2 / delta_m^2 <= 1 for e3 = zeta * (phi_low - phi),
 *     e3 = zeta * (phi_high - phi) or, when centre holds, e3 = 0;  FFS_SHOEBOX_DIALS: (eps1^2 + eps2^2) / delta_b^2 <= 1;
 *   a pixel is foreground when any of its four corners {px, px+1} x {py, py+1} is.
 * A pixel COUNTS when it lies in the image, its mask bit is set, it is <= max_valid when that is set and, for 32-bit pixels, < 2^24 (the
 * rule of ffs_stream_spot_backgrounds).  On image n a pixel p of a box with z_min <= n < z_max:
 *   foreground and counting      fg_sum += p, fg_count += 1, m_x += p (2 px + 1), m_y += p (2 py + 1), m_z += p (2 n + 1);
 *   foreground and not counting  flags |= FFS_SHOEBOX_FG_INVALID (the reference's d_success = 0);
 *   background and counting      the box's histogram: bin p for p < 256, n_overflow otherwise;
 *   background and not counting  nothing.
 * Everything accumulated is an integer, so the result is bit for bit independent of batch size, stream, order and tuning.  (A bin and
 * fg_count are 32 bits: a box of 2^20 pixels holds 4096 images.) */
#define FFS_SHOEBOX_ELLIPSOID 0
#define FFS_SHOEBOX_DIALS 1
#define FFS_SHOEBOX_FG_INVALID 1u
typedef struct {
    double d_matrix[9];        /* row-major: lab = D (x_mm, y_mm, 1) */
    double pixel_size_mm[2];
    double wavelength;
    double s0[3];
    double rot_axis[3];
    double osc_start_deg, osc_width_deg;
} ffs_scan_geometry;              /* 160 bytes */
typedef struct {
    double s1[3];              /* the predicted diffracted beam vector */
    double phi;                /* the predicted rotation angle, radians */
    int32_t x_min, x_max, y_min, y_max, z_min, z_max;   /* half-open; pixels may lie outside the image, z counts images of the scan */
} ffs_shoebox;                    /* 56 bytes */
typedef struct {
    uint64_t fg_sum, m_x, m_y, m_z;
    uint32_t fg_count, n_background, n_overflow, flags;
    uint32_t bg_status, reserved;   /* FFS_SPOT_BG_* of the chosen model */
    double bg_mean, intensity, variance;
} ffs_shoebox_sum;                /* 80 bytes */
/* ffs_ctx_shoebox_begin opens a job: it copies the table, builds an index over the boxes' z-ranges, allocates and zeroes the accumulators
 * (1072 bytes a shoebox; FFS_ERR_NOMEM with a text when they do not fit).  n = 0 is allowed.  delta_b and delta_m are n_sigma * sigma_b and
 * n_sigma * sigma_m in radians.  FFS_ERR_INVALID, state unchanged (ffs_last_error has the text): a NULL geometry, or a NULL table with
 * n > 0; a batch of the context in flight; a job already open; delta_b or delta_m not finite or not positive; an unknown algorithm; a
 * geometry entry that is not finite, a wavelength or pixel size that is not positive; a table entry -- the text names it -- that is empty
 * or reversed, wider or higher than 1024 pixels, does not meet the image padded by 1024 pixels, has a non-finite s1 or phi, or an s1
 * parallel to s0.
 * ffs_ctx_shoebox_end frees the job; idempotent (FFS_OK when there is none).  The job also goes with the context. */
int ffs_ctx_shoebox_begin(ffs_ctx *ctx, const ffs_scan_geometry *geometry, const ffs_shoebox *shoeboxes, uint32_t n, int algorithm,
                          double delta_b, double delta_m);
int ffs_ctx_shoebox_end(ffs_ctx *ctx);
/* Folds the frames of the last batch ffs_wait returned on the stream into the context's job: frame f of the batch is image
 * first_image + f of the scan.  Runs between ffs_wait and the stream's next submit, on the frames where the batch left them (as
 * ffs_stream_spot_backgrounds, with the same three conditions on what must still be in place), under the context's mask and the batch's
 * max_valid.  Synchronous: one launch in a HIP stream of the job's own, a wave per shoebox the images meet; the folds of a context follow
 * one another under a mutex, whichever streams and threads they come from.  kernel_ms may be NULL; otherwise the kernel's time from HIP
 * events on its dispatch (0 when nothing was launched).  A fold that meets no box launches nothing and returns FFS_OK.  The stream's last
 * batch stays as it was: its results, ffs_stream_last_path and ffs_stream_spot_backgrounds* are unchanged by a fold.
 * FOLDING AN IMAGE TWICE COUNTS IT TWICE: which images have been folded is the caller's business.
 * FFS_ERR_INVALID, nothing folded: a dead handle; a batch in flight on the stream; no batch waited on the stream yet, or the last
 * ffs_wait on it failed; no job open; first_image negative, or first_image + frames beyond 2^31 - 1. */
int ffs_stream_shoebox_fold(ffs_stream *s, int64_t first_image, float *kernel_ms);
/* One record per shoebox, in table order, from everything folded so far; the job stays open.  background_model 0: the Tukey fence
 * (ffs_stream_spot_backgrounds' model), 1: the robust Poisson GLM (ffs_stream_spot_backgrounds_glm's), each over the box's histogram and
 * n_overflow, computed on the host by the function the kernels' wave-parallel forms are held to.  n_background is the model's n_pixels;
 * bg_status its status; bg_mean = b = its mean when the status is 0, else 0.  B = b * fg_count, intensity = fg_sum - B,
 * variance = |intensity| + |B| * (1 + fg_count / n_background) (the ratio taken as 0 without background pixels); a shoebox without
 * foreground has intensity 0 and variance -1 (integrator.cc:1107-1161).  *n = the job's shoeboxes, always written; at most cap records
 * are written, and FFS_ERR_OVERFLOW is returned when cap is smaller (the records written are valid).
 * FFS_ERR_INVALID: no job open; NULL n, or NULL out with cap > 0; a background_model other than 0 and 1. */
int ffs_ctx_get_shoebox_sums(ffs_ctx *ctx, int background_model, ffs_shoebox_sum *out, uint32_t cap, uint32_t *n);
/* The raw 256 bins of shoebox `index`, for callers with a model of their own.  FFS_ERR_INVALID: no job open, index outside the table,
 * NULL bins. */
int ffs_ctx_get_shoebox_histogram(ffs_ctx *ctx, uint32_t index, uint32_t bins[256]);

/* Scan prediction for a rotation sweep: the two stages of the reference between indexing and integration -- the
 * per-image ray predictor (predictor/predict.cc:31-128 over predict_ray_monochromatic_sv, predictor/ray_predictors.cc:115-201) and the
 * Kabsch bounding boxes (compute_kabsch_bounding_boxes, integrator/extent.cc:14-198) -- for one flat panel, one s0 and one crystal setting
 * over the scan.  A crystal setting and the scan's geometry give the table ffs_ctx_shoebox_begin takes.  THE RULE is stated once, in
 * csrc/predict_model.hpp, which the kernels, this library's host side and `ffs_hosttool predict` compile; no parity with the reference's
 * binaries is claimed.  Every operation is an IEEE float64 + - * / sqrt floor ceil, a comparison or an integer-to-double conversion in the
 * order written there, compiled without contraction; the device evaluates no trigonometric function:
 *   scan points k = 0 .. n_images: A_k = R(phi_k) A, phi_k = (osc_start_deg + k * osc_width_deg) * (pi / 180), R by Rodrigues' formula about
 *     the normalized rot_axis, cos and sin from the host's libm once per call (ffs_predict_scan_settings hands the matrices out);
 *   candidates: h_max = floor(|real-space axis| / dmin) + 1 per axis from the rows of inverse(A) (cofactors); every (h, k, l) of the box
 *     [-h_max, h_max]^3 but (0,0,0) and the indices absent under the centring, numbered h slowest, l fastest;
 *   image n: r1 = A_n h, r2 = A_{n+1} h; a ray when the two ends lie on different sides of the Ewald sphere (squared norms compared) and
 *     r1.r1 <= 1 / dmin^2; alpha from the two quadratics, s1 = r1 + alpha (r2 - r1) + s0, phi = (phi_n + alpha osc_width) in radians,
 *     entering = r1 outside;
 *   impact: v = inverse(D) s1, v2 > 0, x_px = v0 / v2 / pixel_size_mm[0], y_px likewise, kept when 0 <= x_px < W and 0 <= y_px < H;
 *     z = n + alpha in images from the scan's first;
 *   extent: the four corners (+-delta_b, +-delta_b) in Kabsch space through inverse(D), floor and ceil of their extremes; the images from
 *     phi -+ delta_m / zeta, clamped to the scan; the whole scan when |zeta| <= 1e-10.
 * Records come in the order of candidate number, then image: the same bytes whatever the scheduling. */
#define FFS_CENTRING_P 0
#define FFS_CENTRING_I 1
#define FFS_CENTRING_F 2
#define FFS_CENTRING_A 3
#define FFS_CENTRING_B 4
#define FFS_CENTRING_C 5
#define FFS_CENTRING_R 6           /* obverse setting: (-h + k + l) mod 3 == 0 is present */
#define FFS_PREDICT_ENTERING 1u    /* the reflection starts the image outside the Ewald sphere */
#define FFS_PREDICT_CORNER_LOST 2u /* a corner of the extent had a negative b (or no intersection) and was left out (extent.cc:98-112) */
#define FFS_PREDICT_ZETA_SMALL 4u  /* |zeta| <= 1e-10: the box spans the whole scan (extent.cc:187-192) */
#define FFS_PREDICT_BOX_REFUSED 8u /* ffs_ctx_shoebox_begin would refuse the box: no corner survived, an empty side, or one above 1024 pixels */
typedef struct {
    double a_matrix[9];        /* row-major, 1/Angstrom: r = A h in the laboratory frame at rotation angle 0, fixed and setting rotations applied */
    int32_t centring, reserved;
} ffs_crystal;                    /* 80 bytes */
typedef struct {
    ffs_shoebox box;           /* s1, phi in radians, the half-open box: what ffs_ctx_shoebox_begin takes */
    double x_px, y_px, z;      /* the predicted centre; z in images from the scan's first */
    int32_t h, k, l;
    uint32_t flags;            /* FFS_PREDICT_* */
} ffs_prediction;                 /* 96 bytes */
/* The scan-point settings A_k, k = 0 .. n_images, as ffs_ctx_predict computes them (what predict.cc:68-73 builds per image with its Rotator):
 * out receives (n_images + 1) * 9 doubles, row-major.  Host only: no context, no GPU.  This is the one place libm enters the prediction.
 * FFS_ERR_INVALID (ffs_last_error(NULL) has the text): a NULL argument, an entry that is not finite, a zero rot_axis, n_images 0 or above
 * 65 535. */
int ffs_predict_scan_settings(const ffs_scan_geometry *geometry, const ffs_crystal *crystal, uint32_t n_images, double *out);
/* Predicts the reflections of images 0 .. n_images - 1 of the scan on the context's image (its width and height are the panel's) and their
 * shoeboxes for delta_b = n_sigma * sigma_b and delta_m = n_sigma * sigma_m in radians, as ffs_ctx_shoebox_begin takes them (replaces
 * predict_rotation's thread pool over images, predict.cc:130-, and compute_kabsch_bounding_boxes).  Synchronous, in a HIP stream of its
 * own: a count pass, a scan over the workgroups' counts and a write pass, a lane per candidate.  It changes no batch's plan, reads and
 * writes no state of the context's streams and may run while batches are in flight; calls on one context follow one another under a mutex.
 * *n = the number of predictions, always written when the call is taken; at most cap records are written, and FFS_ERR_OVERFLOW is returned
 * when cap is smaller (the records written are valid): cap 0 with out NULL asks for the size.  kernel_ms may be NULL; otherwise the sum of
 * the launches' times from HIP events on their dispatches.
 * FFS_ERR_INVALID with a text, nothing changed: a NULL geometry, crystal or n, or a NULL out with cap > 0; an entry that is not finite; a
 * singular a_matrix or d_matrix; dmin, delta_b, delta_m, wavelength or a pixel size not positive; osc_width_deg 0; a zero rot_axis or s0;
 * n_images 0 or above 65 535; an unknown centring; a candidate box of more than 2^31 - 1 indices. */
int ffs_ctx_predict(ffs_ctx *ctx, const ffs_scan_geometry *geometry, const ffs_crystal *crystal, uint32_t n_images, double dmin,
                    double delta_b, double delta_m, ffs_prediction *out, uint32_t cap, uint32_t *n, float *kernel_ms);

/* The indexer's basis-vector search: from a sweep's spot centres to candidate real-space lattice vectors, the chain
 * xyz_to_rlp -> fft3d -> flood_fill -> flood_fill_filter -> peaks_to_rlvs of the reference (baseline/indexer/indexer.cc:171-245) for one flat
 * panel without parallax correction and identity setting and sample rotations.  THE RULE is stated once, in csrc/index_model.hpp, which the
 * kernels, this library's host side and `ffs_hosttool indexbasis` compile; no parity with the reference's binaries is claimed.  The device
 * evaluates no libm function: cos, sin (spot rotation, twiddles), exp (weights), log, acos and round enter on the host.
 *   grid: n_points a side, a power of two 16 .. 256; a spot's cell is c2 + N c1 + N^2 c0 with c_j = (int)round(rlp_j * dmin * N / 2) + N/2;
 *     where several spots meet in a cell the highest spot number gives the weight;
 *   FFT: forward, complex float64, unnormalised, radix 2 decimation in time along axis 0, then 1, then 2, by the schedule of the header, so
 *     that the device's grid is bit for bit the CPU twin's; power = re * re;
 *   statistics: float64 sums in a balanced tree (x-lines, then the lines of a plane, then the planes); a voxel is selected at v >= cutoff;
 *   peaks: six-connected components, periodic in all three axes, numbered by their smallest flat index (root), coordinates unwrapped relative
 *     to the root, frac_j = sum_j / (n_voxels * N) with j = 0 the slowest grid axis; records in ascending order of root. */
typedef struct {
    uint32_t root, n_voxels;
    int64_t sum[3];
    double frac[3];
} ffs_index_peak;                 /* 56 bytes */
typedef struct {
    double sum, mean, rmsd, cutoff;
    uint32_t n_selected, n_peaks;
} ffs_index_grid_stats;           /* 40 bytes */
typedef struct {
    double v[3], length;
    uint32_t volume, reserved;
} ffs_index_vector;               /* 40 bytes */
/* Host only, no context, no GPU; FFS_ERR_INVALID with its text in ffs_last_error(NULL), nothing written: a NULL argument; an entry that is not
 * finite; n_points not a power of two in 16 .. 256; dmin or max_cell not positive; a wavelength or pixel size not positive; a singular
 * d_matrix; a zero rot_axis.
 * ffs_index_rlp (replaces xyz_to_rlp, xyz_to_rlp.cc:46-109): xyz_px is n x 3 (x_px, y_px, z in images from the scan's first, the z of
 *   ffs_prediction); rlp, s1 and xyz_mm (x_mm, y_mm, angle in radians) receive n x 3 doubles each.
 * ffs_index_defaults (indexer.cc:184-206): *dmin 0 on entry = choose max(5 max_cell / n_points, the data's highest resolution); b_iso from it.
 * ffs_index_twiddles: the FFT's table, n_points doubles: (cos, -sin) of 2 pi k / n_points for k = 0 .. n_points/2 - 1.
 * ffs_index_map (map_centroids_to_reciprocal_space_grid, fft3d.cc:37-91): per spot its cell (0xFFFFFFFF: not used) and weight.
 * ffs_index_basis_vectors (flood_fill_filter, flood_fill.cc:158-192, and peaks_to_rlvs, peaks_to_rlvs.cc:74-186): the candidate vectors in
 *   Angstrom, sorted by volume; *n_out = their number, at most cap are written, FFS_ERR_OVERFLOW when cap is smaller. */
int ffs_index_rlp(const ffs_scan_geometry *geometry, const double *xyz_px, uint32_t n, double *rlp, double *s1, double *xyz_mm);
int ffs_index_defaults(const double *rlp, uint32_t n, double max_cell, uint32_t n_points, double *dmin, double *b_iso);
int ffs_index_twiddles(uint32_t n_points, double *out);
int ffs_index_map(const double *rlp, uint32_t n, double dmin, double b_iso, uint32_t n_points, uint32_t *cell, double *weight);
int ffs_index_basis_vectors(const ffs_index_peak *peaks, uint32_t n, uint32_t n_points, double dmin, double peak_volume_cutoff,
                            double min_cell, double max_cell, ffs_index_vector *out, uint32_t cap, uint32_t *n_out);
/* ffs_ctx_index_grid (replaces fft3d, fft3d.cc:102-182: pocketfft's c2c on a thread pool): maps the n reciprocal-lattice points, transforms
 * the grid on the device and leaves the power grid resident on the context.  used (may be NULL) receives n bytes, 1 where the spot was
 * mapped; power_out (may be NULL) the N^3 doubles; kernel_ms (may be NULL) the launches' time from HIP events.  The grids are allocated at
 * the first call for an n_points (24 N^3 bytes: 403 MB at 256) and freed with the context; a call at another n_points replaces them.
 * ffs_ctx_index_load_grid puts a caller's power grid in place of the resident one: for tests and callers with a transform of their own.
 * ffs_ctx_index_peaks (replaces flood_fill, flood_fill.cc:31-149) takes the resident grid's statistics, selects v >= rmsd_cutoff * rmsd and
 * gives one record per connected peak.  *n = the number of peaks, always written when the call is taken; at most cap records are written,
 * and FFS_ERR_OVERFLOW is returned when cap is smaller (the records written are valid): cap 0 with out NULL asks for the size.  stats may
 * be NULL.  The list of selected voxels is sized from their count: 36 bytes a selected voxel.
 * All three are synchronous, in a HIP stream of their own; they change no batch's plan, read and write no state of the context's streams
 * and may run while batches are in flight (but see the first call's allocations below); index calls on one context follow one another
 * under a mutex.
 * FFS_ERR_INVALID with a text, state unchanged: a NULL rlp with n > 0, power or n, or a NULL out with cap > 0; an entry that is not finite;
 * n_points not a power of two in 16 .. 256; dmin not positive; a negative or non-finite rmsd_cutoff; ffs_ctx_index_peaks with no grid
 * resident. */
int ffs_ctx_index_grid(ffs_ctx *ctx, const double *rlp, uint32_t n, double dmin, double b_iso, uint32_t n_points, uint8_t *used,
                       double *power_out, float *kernel_ms);
int ffs_ctx_index_load_grid(ffs_ctx *ctx, const double *power, uint32_t n_points);
int ffs_ctx_index_peaks(ffs_ctx *ctx, double rmsd_cutoff, ffs_index_peak *out, uint32_t cap, uint32_t *n, ffs_index_grid_stats *stats,
                        float *kernel_ms);
/* The first call at an n_points allocates (and a call at another n_points first frees) the grids: hipMalloc and hipFree make the whole
 * device wait, so THAT call can stall batches in flight; every later call uses only its own stream.  A call at another n_points drops the
 * resident grid before its allocations can fail: after FFS_ERR_NOMEM no grid is resident.
 * ffs_ctx_index_launch_ms: where the launches' time of the last ffs_ctx_index_grid (entries 0 .. 4) and the last ffs_ctx_index_peaks
 * (5 .. 8) went, in ms from HIP events recorded between the stages in the calls' stream: 0 fill and scatter, 1 FFT along axis 0, 2 along
 * axis 1, 3 along axis 2 with the power grid and the line sums, 4 the sums' trees; 5 the second statistic, 6 selection (count, scan,
 * write), 7 union and flatten, 8 per-root sums and the records' compaction.  Zeros before the first call and for stages a call did not
 * reach.  For measurements (tools/index_cost.py); FFS_ERR_INVALID: NULL out.  (No counterpart in the reference.) */
#define FFS_INDEX_LAUNCH_SPANS 9
int ffs_ctx_index_launch_ms(ffs_ctx *ctx, float *out);

/* Index assignment for candidate crystal settings: how many spots a setting A explains and which Miller index each
 * gets -- the reference's assign_indices_global (assign_indices.cc:56-165), the absence tests and reindexing of non_primitive_basis.cc
 * (:25-34, :43-146, :158-177, :214-217), the spot selection of indexer.cc:266-276 and the candidate settings of combinations.cc, for MANY
 * settings in one call.  THE RULE is stated once, in csrc/assign_model.hpp, which the kernels, this library's host side and
 * `ffs_hosttool indexassign` compile; no parity with the reference's binaries is claimed.  No fit, no refinement, no Niggli reduction, no
 * reflection filter and no score are part of it.  The device evaluates no libm function.
 *   A: 3x3 row-major in 1/Angstrom with r = A h at rotation angle 0 (ffs_ctx_predict's); rlp and phi (radians): ffs_index_rlp's rlp and
 *     column 2 of its xyz_mm.
 *   Per selected spot: hf = inverse(A) rlp (cofactors in one written order), h = round half away from zero, lsq = |h - hf|^2; accepted when
 *     lsq <= tolerance^2 and h != 0; |hf_j| >= 2^19 is out of range (counted, lsq -1).  Of two accepted spots on one index within pi/4 of
 *     phi the one with the smaller lsq stays (pairs in ascending spot number, a tie kills the later spot); survivors are indexed.
 *   A singular setting (det == 0 or a non-finite inverse) has status FFS_INDEX_ASSIGN_SINGULAR, all counts 0, all indices 0, every lsq -1.
 *   sum_lsq_q40 = the sum over indexed spots of (uint64)(lsq * 2^40); absent0[t] = the indexed spots with (h . v_t) mod m_t == 0 for the
 *     111 absence tests of ffs_index_absence_table. */
#define FFS_INDEX_ABSENCE_TESTS 111
#define FFS_INDEX_ASSIGN_SINGULAR 1u
typedef struct {
    uint32_t status, n_accepted, n_indexed, n_out_of_range;
    uint64_t sum_lsq_q40;
    uint32_t absent0[FFS_INDEX_ABSENCE_TESTS];
    uint32_t reserved;
} ffs_index_assignment;           /* 472 bytes */
typedef struct {
    int32_t v[3];
    int32_t modularity;
    int32_t transform[9];
    int32_t reserved;
} ffs_index_absence_test;         /* 56 bytes */
typedef struct {
    uint32_t triple[3];
    uint32_t reserved;
    double axes[9];
    double A[9];
} ffs_index_setting;              /* 160 bytes */
/* Host only, no context, no GPU; FFS_ERR_INVALID with its text in ffs_last_error(NULL), nothing written: a NULL argument, an entry that is
 * not finite, a value outside its range.
 * ffs_index_select (indexer.cc:266-276): selected[i] = 0 when 1 / |rlp_i| <= dmin or phi_i in degrees > osc_start_deg + 360, else 1 (an rlp
 *   of zero is selected and never accepted).
 * ffs_index_settings (combinations.cc): vectors is n x 3 (Angstrom, ffs_index_vector.v in order); the triples i < j < k of the first 100,
 *   stable-sorted by i^2 + j^2 + k^2, the first max_combinations of them through the reference's angle tests (20 degrees), sign flips and
 *   the volume test V > a b c / 100 on the cell as built (NOT Niggli-reduced); per survivor the triple, the axes (rows) and A =
 *   inverse(axes).  *n_out = their number, at most cap are written, FFS_ERR_OVERFLOW when cap is smaller.
 * ffs_index_absence_table: the FFS_INDEX_ABSENCE_TESTS entries (direction, modularity, integer reindexing transform).
 * ffs_index_absence_detect (:158-177): *test = the first t with absent0[t] / n_indexed > threshold, or -1.
 * ffs_index_reindex (:214-217): A_out = inverse(transpose(inverse(T_test)) inverse(A)); FFS_ERR_INVALID when A is singular. */
int ffs_index_select(const double *rlp, const double *phi, uint32_t n, double dmin, double osc_start_deg, uint8_t *selected);
int ffs_index_settings(const double *vectors, uint32_t n, uint32_t max_combinations, ffs_index_setting *out, uint32_t cap, uint32_t *n_out);
int ffs_index_absence_table(ffs_index_absence_test *out);
int ffs_index_absence_detect(const ffs_index_assignment *assignment, double threshold, int32_t *test);
int ffs_index_reindex(const double *A, int32_t test, double *A_out);
/* ffs_ctx_index_assign: rlp n x 3, phi n, selected n bytes or NULL (= all), A n_candidates x 9; out receives n_candidates records; hkl
 * (NULL or n_candidates x n x 3 int32) the final indices, (0, 0, 0) where a spot is not indexed; lsq (NULL or n_candidates x n) each spot's
 * lsq, -1 for unselected and out-of-range spots and under a singular setting.  n = 0 and n_candidates = 0 are allowed.  The settings are
 * taken in passes of as many as fit workspace_bytes of device state (0 = 256 MiB; csrc/assign_plan.hpp has the bytes per setting);
 * FFS_ERR_NOMEM with a text when not even one fits.  The result does not depend on the passes.  Synchronous, in a HIP stream of its own;
 * it changes no batch's plan and may run while batches are in flight; calls on one context follow one another under a mutex.
 * FFS_ERR_INVALID with a text, nothing written: a NULL rlp or phi with n > 0, a NULL A or out with n_candidates > 0; an entry of rlp, phi
 * or A or a tolerance that is not finite; tolerance outside (0, 0.5]; n > 2^20; n_candidates > 4096.
 * ffs_ctx_index_assign_launch_ms: the launches' time of the last call over all its passes, in ms from HIP events: 0 assign (with the key
 * table), 1 duplicates (place, fill, resolve), 2 reduce.  Zeros before the first call. */
int ffs_ctx_index_assign(ffs_ctx *ctx, const double *rlp, const double *phi, const uint8_t *selected, uint32_t n, const double *A,
                         uint32_t n_candidates, double tolerance, size_t workspace_bytes, ffs_index_assignment *out, int32_t *hkl,
                         double *lsq);
int ffs_ctx_index_assign_launch_ms(ffs_ctx *ctx, float *out);

/* Centres of mass of the last batch's reflections as rows (frame_id, x, y, z) of float32 -- the
 * payload of `--output-for-index` (spot_centers, spotfinder.cc:919-933,1004-1006), in frame order;
 * used to feed a multi-GPU gather without a per-frame loop on the caller's side.  Lane 0 carries the
 * low 32 bits of the frame id as a BIT PATTERN (read it as uint32: as a float value ids would collide
 * from 2^24 on).  Writes at most `cap` rows, then one more row whose first two lanes are, again as uint32
 * bit patterns, (rows written, rows wanted): rows4 must hold (cap + 1) * 4 floats.  Returns
 * FFS_ERR_OVERFLOW (rows written are valid) when wanted > cap.  Needs want_reflections.  Reads the last ffs_wait's results
 * only: may run (on another thread) while the stream's next batch is in flight, until the next ffs_wait on this stream. */
int ffs_stream_spot_centres(ffs_stream *s, float *rows4, uint32_t cap, uint32_t *n_written);

/* ---- measurement entry points (bench.py roofline leg, tools/) -------------------------------- */
/* Runs the threshold stage alone on device-resident frames, `iters` times, every launch on the state the hot
 * path gives it (zeroed counters, empty plane) and returns the average duration of ONE launch of its dense
 * kernel (ms_dense: the streaming kernel; extended algorithm: its first pass) and of what follows it inside the
 * stage (ms_rest: the bright-window fix-up; extended: erosion + final pass), each from HIP events that ride on
 * the dispatches themselves, on the stream the kernels are launched on.  (The reference prints "Kernel: ms" per
 * image from events around its launch wrapper, spotfinder/spotfinder.cc:1056-1076.) */
int ffs_bench_threshold(ffs_stream *s, const void *device_pixels, size_t pitch_bytes,
                        size_t frame_stride_bytes, uint32_t n_frames, uint32_t iters,
                        float *ms_dense, float *ms_rest);
/* Runs the radial profile (ffs_ctx_set_radial_bins: the context needs a map) alone on device-resident frames, `iters` times, and
 * returns the average duration of one batch's profile -- its two launches, from HIP events that ride on the dispatches themselves.  The
 * profile ffs_stream_radial_profile hands out is not touched.  (No counterpart in the reference.) */
int ffs_bench_radial(ffs_stream *s, const void *device_pixels, size_t pitch_bytes, size_t frame_stride_bytes,
                     uint32_t n_frames, uint32_t iters, float *ms);
/* Runs the per-pixel statistics' kernel alone on device-resident frames, `iters` times, and returns the average duration of one batch's
 * launch from HIP events that ride on the dispatch.  It uses the context's own accumulators (allocated here if need be) and leaves them
 * undefined: FFS_ERR_INVALID while accumulation is on or a batch of the context is in flight.  (No counterpart in the reference.) */
int ffs_bench_pixel_stats(ffs_stream *s, const void *device_pixels, size_t pitch_bytes, size_t frame_stride_bytes,
                          uint32_t n_frames, uint32_t iters, float *ms);
/* The submit / wait loop of a resident-frames benchmark, natively: `steps` batches of the same device-resident
 * frames through `n_streams` streams of ONE context, all of them in flight (ffs_submit_device / ffs_wait).  For
 * drivers with one host thread per GPU (bench.py --single-process, the threading model of
 * spotfinder/spotfinder.cc:725-752 spread over several devices).  Returns the sums over all frames. */
int ffs_bench_pipeline(ffs_stream *const *streams, uint32_t n_streams, const void *device_pixels,
                       size_t pitch_bytes, size_t frame_stride_bytes, uint32_t n_frames, uint32_t steps,
                       int64_t first_frame_id, uint64_t *n_boxes, uint64_t *n_strong_pixels);
/* Memory ceiling measured on this device (BASELINE.md section 3 asks for one beside the nominal 8 TB/s): the
 * stream's own buffers are read linearly, 16 B per lane (read_gbps), and read while one 8-byte zero store per
 * 16 bytes read goes to the byte-mask buffer -- the threshold kernel's 2:1 read/write mix with the friendliest
 * possible addresses (mix_gbps).  GB/s of bytes moved.  Overwrites the stream's byte masks; no batch in flight.
 * (The reference prints GBps per image, spotfinder/spotfinder.cc:1056-1076, against no ceiling.) */
int ffs_bench_hbm(ffs_stream *s, uint32_t iters, float *read_gbps, float *mix_gbps);
/* Device pointers of the last batch's dense planes (strong byte mask rows are
 * mask_pitch apart) -- for parity tests that want the raw kernel output.  The byte masks hold the last batch's
 * result only if that batch ran with want_strong_mask = 1. */
int ffs_stream_debug_planes(ffs_stream *s, const uint8_t **device_strong_bytes,
                            size_t *mask_pitch, size_t *mask_frame_stride);
/* Copies one frame's bit plane of the last completed batch to host memory, unpacked to W*H
 * bytes (0/1): which = 0 strong pixels, 1 the extended algorithm's first-pass "not background"
 * mask (first_pass_dispersion_result in the reference's --writeout, spotfinder.cu:268-279),
 * 2 its eroded signal region (eroded_dispersion_result, :300-311). */
int ffs_stream_debug_bitplane(ffs_stream *s, uint32_t frame_in_batch, int which, uint8_t *host_out);

/* Known-answer self test of the one non-trivial fp64 operation the exact predicate relies on:
 * sum (mod 2^64) of the bit patterns of sqrt((double)n) for integers n in [begin, end), computed on
 * the device with the same code path k_exact uses.  The caller compares it with libm's correctly
 * rounded sqrt (tests/test_gpu_numerics.py does, exhaustively for every n = x*m a uint16 frame
 * can produce). */
int ffs_selftest_sqrt(ffs_ctx *ctx, uint64_t begin, uint64_t end, uint64_t *sum_of_bits);

/* ---- rotation sweeps: 3D connected components (replaces
 *      ConnectedComponents::find_3d_components, connected_components.cc:270-470) -------------- */
int ffs_stack3d_create(ffs_ctx *ctx, uint64_t max_total_strong, ffs_stack3d **out);
/* (idempotent: see ffs_ctx_destroy; the stack's buffers are kept by the context for its next sweep) */
void ffs_stack3d_destroy(ffs_stack3d *st);
/* Adds the strong pixels of every frame of the stream's last completed batch, keyed by frame_id
 * (the reference keys its rotation_slices map by image number, spotfinder.cc:913-918). */
int ffs_stack3d_add_batch(ffs_stack3d *st, ffs_stream *s);
/* Adds one slice from host memory (k ascending) -- what a gather from other GPUs delivers.
 * A frame id added twice: the later list counts.  Intensities are expected to be at least 1, as
 * every list the threshold produces is: for a strong pixel of intensity 0 the reference's peak
 * search (which starts from numeric_limits<double>::min()) and the packed maximum used here
 * (which starts from 0) legitimately disagree about the peak. */
int ffs_stack3d_add_slice(ffs_stack3d *st, int64_t frame_id, const uint32_t *k,
                          const uint32_t *intensity, uint32_t n);
/* Orders slices by frame_id (std::map order, spotfinder.cc:1105-1108), z = rank, runs the 3D
 * union-find on the device, filters with min_spot_size_3d / max_peak_centroid_separation.
 * reflections are in label order; n_calculated = "Calculated {} spots".
 * Centroids are bit-exact with the reference while sum (2c+1) * I < 2^53 per component and axis
 * (c = x, y or z; the sums are kept as 64-bit integers, the reference adds (c + 0.5) * I in
 * double, exact while its partial sums stay below 2^52): beyond that the reference's own result
 * depends on its summation order. */
int ffs_stack3d_finish(ffs_stack3d *st, const ffs_reflection **reflections,
                       uint32_t *n_reflections, uint32_t *n_calculated,
                       uint32_t *n_filtered_size, uint32_t *n_filtered_sep);
/* ---- several GPUs in one process ------------------------------------------------------------------
 * The reference drives ONE device (-d, src/ffs/cuda_arg_parser.cc:30-61).  A driver that owns several makes
 * one ffs_ctx per GPU and deals its frame queue to all of them (spotfinder --devices / --gpus); stills need
 * no exchange.  For rotation sweeps ffs_stack3d_add_batch() accepts a stream of ANOTHER context with the same
 * frame shape: the batch's strong-pixel lists are packed on their GPU and sent to the stack's GPU -- by RCCL
 * point-to-point over xGMI when ffs_multi_init() could load librccl and build the communicators, else by
 * peer copies.  `devices`: the GPUs in use (duplicates allowed); transport: "rccl", "peer" or NULL (= the
 * FFS_GATHER environment variable, default "rccl").  ffs_multi_transport(): "rccl", "peer" or "none".
 * Call it before the first batch is added to a stack, not while batches are being added.  A frame that
 * overflowed its stream's lists reaches the stack from any GPU (its list goes up from the host, as on one GPU). */
int ffs_multi_init(const int *devices, int n_devices, const char *transport);
const char *ffs_multi_transport(void);
/* The gather of the per-frame spot lists over RCCL (BASELINE.json north_star, SURVEY section 8(e): "ncclAllGather of per-rank record
 * counts, then grouped ncclSend / ncclRecv of the packed spot records to rank 0, then a single D2H"; the reference has one device and
 * no such step).  streams[i]: one stream per taking-part context, each with a completed batch (after ffs_wait) whose centre rows
 * (frame id bits, x, y, z: ffs_stream_spot_centres) are what travels; every rank of the communicator ffs_multi_init built needs at
 * least one stream, contexts that share a GPU share its rank (their rows travel as one message).  The rows arrive in rows4_out (host
 * memory, room for cap rows of four floats) rank after rank, inside a rank in the order of `streams`; *n_rows = rows wanted.  FFS_ERR_OVERFLOW: they do not fit cap; FFS_ERR_INVALID: no RCCL
 * communicators (ffs_multi_transport() != "rccl").  A stream of the root's own GPU hands its rows over by a device copy unless the
 * transport was forced (ffs_multi_init(.., "rccl") or FFS_GATHER): then it sends to its own rank -- what a one-GPU box can rehearse.
 * In ONE process the rows are on the host already after ffs_wait; reading them there is the faster gather:
 * this entry point is the A/B partner and the building block for drivers that keep the rows on the devices. */
int ffs_multi_gather_rows(ffs_stream *const *streams, uint32_t n_streams, uint32_t root, float *rows4_out, uint32_t cap,
                          uint32_t *n_rows);
/* NUMA node the GPU hangs off (sysfs), -1 if unknown: where a driver should keep the worker threads that feed
 * it (the reference pins nothing: one device, spotfinder.cc:725-742). */
int ffs_device_numa_node(int device);
/* Device time of the last ffs_stack3d_finish (upload of the slice table to the labels of every strong pixel), ms. */
int ffs_stack3d_last_finish_ms(const ffs_stack3d *st, float *ms);
/* Per-signal view of the last ffs_stack3d_finish: every strong pixel of the stack in the reference's
 * vertex order (slice by slice, ascending linear index -- the order Reflection3D::signals_ is filled
 * in, connected_components.cc:409-446) with the index of its reflection in the array finish
 * returned, or -1 if that spot was filtered.  For per-signal sums the caller owns, e.g.
 * Reflection3D::variances_in_kabsch_space (connected_components.cc:159-203).  Pointers stay valid
 * until the next finish / destroy. */
int ffs_stack3d_signals(ffs_stack3d *st, const uint32_t **x, const uint32_t **y, const int32_t **z,
                        const uint32_t **intensity, const int32_t **reflection, uint64_t *n);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif
