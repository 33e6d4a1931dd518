/*
 * ffs_synth.h -- deterministic synthetic detector frames and masks.
 *
 * The reference's only synthetic source is h5read_generate_samples()
 * (h5read/src/h5read.c:203-276: six fixed Eiger-16M frames, PCG32 at :189-201;
 * module-gap mask at :1131-1156).  This generator produces the workloads
 * BASELINE.json / SURVEY.md section 8(d) name (Poisson background + Gaussian
 * spots, optional rocking curve across a sweep, u16 or u32 pixels) from a seed,
 * with integer RNG and home-grown exp so that the same bytes come out on every
 * machine.  It also restates the reference's sample images 0..5 and its
 * Eiger-2XE-16M module-gap mask so the reference's own synthetic cases can be
 * run through the pipeline.
 */
#ifndef FFS_SYNTH_H
#define FFS_SYNTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t width;       /* fast axis */
    uint32_t height;      /* slow axis */
    int32_t pixel_bytes;  /* 2 (uint16) or 4 (uint32) */
    uint64_t seed;        /* dataset seed */
    double background;    /* Poisson mean per pixel */
    uint32_t n_spots;     /* spots per frame (stills) or per sweep (rotation) */
    double sigma_min, sigma_max; /* in-plane Gaussian sigma, px */
    double peak_min, peak_max;   /* expected peak counts, log-uniform */
    uint32_t max_value;   /* clamp (e.g. 65535) */
    /* rotation sweep: if n_frames > 0 and sigma_z_max > 0 the spot list is
     * drawn once per dataset and every spot gets a centre frame and a Gaussian
     * rocking width; otherwise spots are redrawn for every frame. */
    uint32_t n_frames;
    double sigma_z_min, sigma_z_max;
} ffs_synth_params;

/* Fill `out` (width*height pixels of pixel_bytes) with frame number `frame`. */
int ffs_synth_frame(const ffs_synth_params *p, uint32_t frame, void *out);

/* Module-gap mask (1 = valid): n_fast x n_slow modules of mod_fast x mod_slow
 * pixels separated by gap_fast / gap_slow masked pixels.
 * Eiger 2XE 16M = (1028, 512, 12, 38, 4, 8), h5read/include/eiger2xe.h:6-19. */
int ffs_synth_mask_modules(uint8_t *mask, uint32_t width, uint32_t height,
                           uint32_t mod_fast, uint32_t mod_slow, uint32_t gap_fast,
                           uint32_t gap_slow);

/* Knock out `n_dead` pseudo-random pixels (sets them to 0). */
int ffs_synth_mask_dead_pixels(uint8_t *mask, uint32_t width, uint32_t height,
                               uint64_t seed, uint32_t n_dead);

/* Mask a rectangle [x0,x1) x [y0,y1). */
int ffs_synth_mask_rect(uint8_t *mask, uint32_t width, uint32_t height, uint32_t x0,
                        uint32_t x1, uint32_t y0, uint32_t y1);

/* The reference's generated sample images n = 0..5 (h5read.c:203-276), always
 * Eiger-2XE-16M shaped (4148 x 4362), written as pixel_bytes-wide pixels. */
int ffs_synth_reference_sample(uint32_t n, int32_t pixel_bytes, void *out);

/* A Jungfrau calibration as a pure function of (pixel, seed), for raw-word sources (ffs_ctx_set_jungfrau_calibration of ffs_hip.h has the
 * conversion): six planes of width*height float32, pedestal G0, G1, G2 then factor G0, G1, G2 -- the layout of the driver's
 * --jungfrau-calibration file.  Pedestals are multiples of 1/2 ADU near 2900 / 14700 / 15400; the factors are those of 480-543 ADU per
 * photon in G0, 17-17.75 in G1 and 1.25-1.44 in G2 (both inverted: negative factors); about one pixel in 500 has factor 0, "no
 * calibration", in one stage.  Only IEEE division and exact sums: the same bytes on every host. */
int ffs_synth_jungfrau_calibration(uint32_t width, uint32_t height, uint64_t seed, float *planes);

/* Photon counts (width*height uint32) as the raw 16-bit words of a Jungfrau (gain code << 14 | ADC) under `planes` (as above).  The stage
 * goes by magnitude: G0 below 24 photons, G1 below 800, G2 above; ADC = rint(pedestal + photons / factor), so the conversion gives the
 * photons back to within the ADC's resolution.  A count that drives G2's ADC to 0 or below comes out as the saturated word 0xC000; a
 * pixel without calibration in its stage keeps its stage and is invalid by its factor; and about one word in 4096 each is 0xFFFF,
 * carries the gain code 2, or is 0xC000, as a pure function of (seed, frame, pixel). */
int ffs_synth_jungfrau_encode(const uint32_t *photons, uint32_t width, uint32_t height, const float *planes, uint64_t seed,
                              uint32_t frame, uint16_t *raw);

/* One frame of a DARK run under `planes` (as above; only the pedestals are read): what the pedestals are measured from
 * (ffs_stream_jungfrau_pedestal_fold of ffs_hip.h).  Frame `frame` of `n_frames` is forced into stage 3 * frame / n_frames: the first third
 * of a run is G0, the second G1, the last G2.  A pixel's word is that stage's gain code with ADC = clamp(floor(pedestal_s) + e, 0, 16383),
 * e in -2 .. 2 a pure function of (seed, frame, pixel): every measured pedestal lies within 2 ADU of floor(pedestal).  About one word
 * in 4096 is replaced by one of the three invalid words (0xFFFF, the gain code 2, 0xC000), and about one pixel in 1024 -- a pure function
 * of (seed, pixel) -- is STUCK: it reports G0, with G0's pedestal, whatever the run forces, so its G1 and G2 counts stay 0.
 * -1: a NULL pointer, a zero size, frame >= n_frames. */
int ffs_synth_jungfrau_dark(uint32_t width, uint32_t height, const float *planes, uint64_t seed, uint32_t frame, uint32_t n_frames,
                            uint16_t *raw);

#ifdef __cplusplus
}
#endif
#endif
