"""The truth for the per-pixel gain map (ffs_ctx_set_gain_map; a helper module, not a test): the NumPy float64 restatement of
tests/gain_oracle.py with the gain an H x W float32 ARRAY, widened to float64 (exactly), of which every pixel's decision reads the
entry of the window's CENTRE -- the reference's threshold_w_gain, baseline/spotfinder/baseline.cpp: gain[k] at :244-245 (standard
algorithm), :541 (extended first pass), :714 (extended final pass).  tests/test_gain_map_oracle.py ties it to gain_oracle on
constant maps and to a pixel loop.

Window sums, erosion, min_count, threshold and max_valid are gain_oracle's (no gain enters them); one NumPy float64 operation per
C++ operation, in the order of the C++ text."""
import numpy as np

import gain_oracle as G


def _widen(gain_map, shape):
    g32 = np.ascontiguousarray(gain_map, dtype=np.float32)
    assert g32.shape == shape and np.all(np.isfinite(g32)) and np.all(g32 > 0)
    return g32.astype(np.float64)   # exact


def _a_c(m, x, y, g, nsig_b):
    md, xd, yd = m.astype(np.float64), x.astype(np.float64), y.astype(np.float64)
    nb = np.float64(nsig_b)
    with np.errstate(invalid="ignore"):   # (m = 0: sqrt(-2); such a pixel fails m >= min_count)
        a = md * yd - xd * xd                                          # :242, :540
        c = (g * xd) * ((md - 1.0) + nb * np.sqrt(2.0 * (md - 1.0)))   # :244, :541 -- g = gain[k], the centre's
    return md, xd, a, c


def dispersion_gain_map(img, mask, gain_map, kx=3, ky=3, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0, max_valid=-1):
    """Strong pixels (uint8 HxW) of the standard algorithm under a gain map, baseline.cpp:241-247."""
    g = _widen(gain_map, img.shape)
    v = img.astype(np.int64)
    valid = mask != 0
    m, x, y = G.window_sums(v, valid & (v < G.BIG), kx, ky)
    md, xd, a, c = _a_c(m, x, y, g, nsig_b)
    src = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        b = md * src - xd                                              # :243
        d = np.float64(nsig_s) * np.sqrt((g * xd) * md)                # :245
        strong = valid & (m >= min_count) & (src > threshold) & (a > c) & (b > d)
    if max_valid >= 0:
        strong &= v <= max_valid
    return strong.astype(np.uint8)


def dispersion_extended_gain_map(img, mask, gain_map, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0, max_valid=-1):
    """(strong, first, eroded) of the extended algorithm, flavour 0, under a gain map: first pass a > c (baseline.cpp:539-543),
    erosion, final pass p >= mean + nsig_s sqrt(gain[k] mean) (:709-715).  max_valid as in gain_oracle."""
    g = _widen(gain_map, img.shape)
    v = img.astype(np.int64)
    valid = mask != 0
    m, x, y = G.window_sums(v, valid & (v < G.BIG), 3, 3)
    _, _, a, c = _a_c(m, x, y, g, nsig_b)
    with np.errstate(invalid="ignore"):
        first = valid & (m >= min_count) & (a > c)
    if max_valid >= 0:
        first &= v <= max_valid
    eroded = G.erode(first, mask).astype(bool)
    m2, x2, _ = G.window_sums(v, valid & ~eroded & (v < G.BIG), 5, 5)
    src = v.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(m2 >= 2, x2.astype(np.float64) / m2.astype(np.float64), 0.0)        # :712
        local = src >= (mean + np.float64(nsig_s) * np.sqrt(g * mean))                       # :713-714
    strong = valid & eroded & (src > threshold) & local
    if max_valid >= 0:
        strong &= v <= max_valid
    return strong.astype(np.uint8), first.astype(np.uint8), eroded.astype(np.uint8)


# ---- the maps the gain-map tests share (CPU and GPU); made for 530 x 97, they scale to any shape
def module_map(W=530, H=97):
    """Six regions, rows split at 48/97 of the height, columns at 250/530 and 500/530 of the width: gains 7 / 2.5 / 0.3 over
    1 / 0.3 / 7.  At 530 x 97 the boundary x = 500 sits 4 px from the general-window kernel's 496-px strip edge."""
    ys = (48 * H + 96) // 97
    x0, x1 = (250 * W + 529) // 530, (500 * W + 529) // 530
    g = np.empty((H, W), np.float32)
    for rows, gains in ((slice(0, ys), (7.0, 2.5, 0.3)), (slice(ys, H), (1.0, 0.3, 7.0))):
        g[rows, :x0], g[rows, x0:x1], g[rows, x1:] = gains
    return g


def random_map(seed, W=530, H=97):
    """Uniform [0.5, 8), float32, independent per pixel."""
    return np.random.default_rng(1000 + seed).uniform(0.5, 8.0, size=(H, W)).astype(np.float32)


def adu_under_map(photons, gain_map, dtype):
    """The photon frame as a detector with this gain map delivers it: rint(photons x map)."""
    return np.rint(photons * gain_map.astype(np.float64)).astype(dtype)
