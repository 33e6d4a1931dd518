"""The truth for the detector gain (ffs_ctx_set_gain; a helper module, not a test): a NumPy float64 restatement of the reference's
threshold_w_gain arithmetic with a scalar gain -- baseline/spotfinder/baseline.cpp:241-247 (standard algorithm), :539-543 and
:709-715 (extended algorithm, flavour 0).  The compiled oracle has no gain; tests/test_gain_oracle.py ties this restatement to it
at gain 1.0, by powers of two, and against a pixel loop.

Window sums are exact int64 (valid neighbours; 32-bit pixels only those below 2^24, standalone.cc:78,90), converted once to
float64; every operation of the predicate is then one NumPy float64 operation, in the order of the C++ text.  The erosion is
restated from oracle/ffs_oracle.c:296-315 (a not-background pixel stays in the signal region when every in-image pixel within
Chebyshev distance 2 is not background; masked pixels are background)."""
import numpy as np

BIG = 1 << 24


def window_sums(vals, ok, kx, ky):
    """(m, x, y) as int64 planes: count, sum and sum of squares of `vals` where `ok`, over the (2kx+1) x (2ky+1) window clipped to
    the frame (standalone.cc:126-130)."""
    H, W = vals.shape
    pv = np.where(ok, vals, 0).astype(np.int64)

    def box(a):
        p = np.pad(a, ((ky, ky), (kx, kx)))
        rows = sum(p[:, dx:dx + W] for dx in range(2 * kx + 1))
        return sum(rows[dy:dy + H, :] for dy in range(2 * ky + 1))

    return box(ok.astype(np.int64)), box(pv), box(pv * pv)


def _gain_a_c(m, x, y, gain, nsig_b):
    md, xd, yd = m.astype(np.float64), x.astype(np.float64), y.astype(np.float64)
    g, nb = np.float64(gain), np.float64(nsig_b)
    with np.errstate(invalid="ignore"):   # (m = 0: sqrt(-2); such a pixel fails m >= min_count)
        a = md * yd - xd * xd                                          # :242
        c = (g * xd) * ((md - 1.0) + nb * np.sqrt(2.0 * (md - 1.0)))   # :244
    return md, xd, a, c


def dispersion_gain(img, mask, gain, kx=3, ky=3, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0, max_valid=-1):
    """Strong pixels (uint8 HxW) of the standard algorithm under a scalar gain > 0, baseline.cpp:241-247."""
    assert gain > 0
    v = img.astype(np.int64)
    valid = mask != 0
    m, x, y = window_sums(v, valid & (v < BIG), kx, ky)
    md, xd, a, c = _gain_a_c(m, x, y, gain, nsig_b)
    src = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        b = md * src - xd                                              # :243
        d = np.float64(nsig_s) * np.sqrt((np.float64(gain) * xd) * md)  # :245
        strong = valid & (m >= min_count) & (src > threshold) & (a > c) & (b > d)
    if max_valid >= 0:
        strong &= v <= max_valid
    return strong.astype(np.uint8)


def erode(first, mask):
    """The signal region (1 = stays in it) from the first-pass plane, oracle/ffs_oracle.c:296-315 with the 7x7 kernel."""
    H, W = first.shape
    d = np.pad(first.astype(bool), 2, constant_values=True)   # (pixels outside the image are no sources of distance)
    keep = np.ones((H, W), bool)
    for dy in range(5):
        for dx in range(5):
            keep &= d[dy:dy + H, dx:dx + W]
    return ((mask != 0) & first.astype(bool) & keep).astype(np.uint8)


def dispersion_extended_gain(img, mask, gain, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0, max_valid=-1):
    """(strong, first, eroded) of the extended algorithm, flavour 0, under a scalar gain > 0: first pass a > c (baseline.cpp:539-543),
    erosion, final pass p >= mean + nsig_s sqrt(gain mean) over the 11x11 window's background pixels (:709-715).  The guard of
    max_valid >= 0 is the device kernels' (centre pixels above it are neither not-background nor strong), as in the oracle."""
    assert gain > 0
    v = img.astype(np.int64)
    valid = mask != 0
    m, x, y = window_sums(v, valid & (v < BIG), 3, 3)
    _, _, a, c = _gain_a_c(m, x, y, gain, nsig_b)
    with np.errstate(invalid="ignore"):
        first = valid & (m >= min_count) & (a > c)
    if max_valid >= 0:
        first &= v <= max_valid
    eroded = erode(first, mask).astype(bool)
    m2, x2, _ = window_sums(v, valid & ~eroded & (v < BIG), 5, 5)
    src = v.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(m2 >= 2, x2.astype(np.float64) / m2.astype(np.float64), 0.0)        # :712
        local = src >= (mean + np.float64(nsig_s) * np.sqrt(np.float64(gain) * mean))        # :713-714
    strong = valid & eroded & (src > threshold) & local
    if max_valid >= 0:
        strong &= v <= max_valid
    return strong.astype(np.uint8), first.astype(np.uint8), eroded.astype(np.uint8)


# ---- the frames the gain tests share (CPU and GPU): photon counts, and the same frame as a detector with a gain delivers it
def photon_frame(seed, W=530, H=97, masked=True):
    """Poisson(3) photons plus 1 % spot pixels, 12 % of the pixels masked: (int64 photons, uint8 mask)."""
    rng = np.random.default_rng(seed)
    photons = rng.poisson(3.0, size=(H, W)).astype(np.int64)
    spots = rng.random((H, W)) < 0.01
    photons[spots] = rng.integers(20, 900, size=spots.sum())
    mask = (rng.random((H, W)) > 0.12).astype(np.uint8) if masked else np.ones((H, W), np.uint8)
    return photons, mask


def adu(photons, gain, dtype):
    """The photon frame in ADU: rint(photons x gain)."""
    return np.rint(photons * np.float64(gain)).astype(dtype)


def blob_photons(seed, W=300, H=200, masked=True):
    """Fat spots on a quiet background behind a module mask (what the extended algorithm's signal region needs): (uint16 photons, mask)."""
    from ffs_amd import synth
    from util import _blob_frame
    img = _blob_frame(W, H, seed, 25)
    return img, synth.mask_modules(W, H, 140, 90, 6, 8) if masked else np.ones((H, W), np.uint8)
