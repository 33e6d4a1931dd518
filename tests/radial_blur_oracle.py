"""NumPy truth for the blur of the radial-profile threshold (ffs_ctx_set_radial_blur, include/ffs_hip.h): a separable integer convolution
of p * tap and of tap, a floor division, then radial_threshold_oracle's shells over the blurred values and the strong rule with its
p >= 1 clause.  Everything is integers (the cutoff's two float64 operations are radial_threshold_oracle.cutoff's)."""
import numpy as np

import radial_threshold_oracle as RT

NONE, NARROW, WIDE = 0, 1, 2
W1 = {NARROW: (1, 2, 1), WIDE: (1, 4, 6, 4, 1)}
FULL = {NARROW: 16, WIDE: 256}
NO_BIN = RT.NO_BIN


def taps(img, mask=None, max_valid=-1):
    """Which pixels enter the sums: the valid-pixel mask, max_valid, and p < 2^24 for 32-bit pixels.  The bin map plays no part."""
    ok = np.ones(img.shape, bool)
    if mask is not None:
        ok &= mask != 0
    if max_valid >= 0:
        ok &= img.astype(np.uint64) <= max_valid
    if img.dtype.itemsize == 4:
        ok &= img < (1 << 24)
    return ok


def counting_limit(dtype, max_valid=-1):
    """The value rule of `taps` as one number, p < limit (csrc/launch_geometry.hpp, counting_limit)."""
    return min(int(max_valid), (1 << 24) - 1) + 1 if max_valid >= 0 else 1 << 24


def _separable(a, w1):
    """sum over dy, dx of w1[dy] * w1[dx] * a[y + dy, x + dx], zero outside the image; int64."""
    r = len(w1) // 2
    H, W = a.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    pad[r:r + H, r:r + W] = a
    vert = sum(w * pad[k:k + H, :] for k, w in enumerate(w1))
    return sum(w * vert[:, k:k + W] for k, w in enumerate(w1))


def sums(img, blur, mask=None, max_valid=-1):
    """(S, Wn, tap) of every pixel."""
    tap = taps(img, mask, max_valid)
    S = _separable(np.where(tap, img.astype(np.int64), 0), W1[blur])
    Wn = _separable(tap.astype(np.int64), W1[blur])
    return S, Wn, tap


def blurred(img, blur, mask=None, max_valid=-1):
    """(v, tap): v = floor(S / Wn) at every tap pixel, 0 elsewhere.  blur NONE: v = p."""
    if blur == NONE:
        tap = taps(img, mask, max_valid)
        return np.where(tap, img.astype(np.int64), 0), tap
    S, Wn, tap = sums(img, blur, mask, max_valid)
    assert int(S.max(initial=0)) < 1 << 32
    return np.where(tap, S // np.maximum(Wn, 1), 0), tap


def histograms(v, tap, bins, n_bins):
    ok = tap & (bins != NO_BIN)
    at = bins[ok].astype(np.int64) * (RT.VALUES + 1) + np.minimum(v[ok], RT.VALUES)
    return np.bincount(at, minlength=n_bins * (RT.VALUES + 1)).reshape(n_bins, RT.VALUES + 1).astype(np.uint32)


def strong_mask(img, v, tap, bins, shells, thr=0.0):
    ok = tap & (bins != NO_BIN)
    idx = np.where(bins == NO_BIN, 0, bins).astype(np.int64)
    cut = shells["cutoff"].astype(np.int64)[idx]
    good = (shells["status"] == RT.OK)[idx]
    return (ok & good & (v > cut) & (v.astype(np.float64) > float(thr)) & (img >= 1)).astype(np.uint8)


def threshold(img, bins, n_bins, blur, n_iqr=6.0, thr=0.0, mask=None, max_valid=-1):
    """(strong mask, shells) of one frame under a blur."""
    v, tap = blurred(img, blur, mask, max_valid)
    shells = RT.shells_from_histograms(histograms(v, tap, bins, n_bins), n_iqr)
    return strong_mask(img, v, tap, bins, shells, thr), shells


def fixture_frames(dtype, B, H, W, bins, seed):
    """Test frames: test_gpu_radial_threshold.py's recipe over the shells `bins` (Poisson(3) + 20 x (shell mod 5), the corner's shell raised
    by Poisson(400), 1 % bright pixels in 100..60000, 32-bit frames with values at and above 2^24), plus Gaussian blobs of peak 200..30 000
    and sigma 0.7..1.5, one per 400 pixels, so that blurred spots survive, and 2 % zero pixels."""
    rng = np.random.default_rng(seed)
    shell = np.where(bins == NO_BIN, 0, bins).astype(np.int64)
    f = rng.poisson(3.0, (B, H, W)).astype(np.int64) + 20 * (shell % 5)[None]
    raised = int(shell[0, W - 1])
    f += np.where(shell == raised, 1, 0)[None] * rng.poisson(400.0, (B, H, W))
    bright = rng.random((B, H, W)) < 0.01
    f[bright] = rng.integers(100, 60000, int(bright.sum()))
    y, x = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(max(1, W * H // 400)):
            cy, cx, peak, sigma = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(200.0, 30000.0), rng.uniform(0.7, 1.5)
            f[b] += np.floor(peak * np.exp(-((x + 0.5 - cx) ** 2 + (y + 0.5 - cy) ** 2) / (2.0 * sigma * sigma))).astype(np.int64)
    f = np.minimum(f, 65535)
    f[rng.random((B, H, W)) < 0.02] = 0
    if np.dtype(dtype) == np.dtype(np.uint32):
        top = rng.random((B, H, W)) < 0.01
        f[top] = rng.choice(np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 7, 0xFFFFFFFF], np.int64), int(top.sum()))
    return f.astype(dtype)


def gappy_mask(W, H, seed):
    """A 3-column gap, a 2-row gap, 2 % dead pixels."""
    rng = np.random.default_rng(seed)
    m = np.ones((H, W), np.uint8)
    m[:, W // 3:W // 3 + 3] = 0
    m[H // 2:H // 2 + 2, :] = 0
    m[rng.random((H, W)) < 0.02] = 0
    return m


def blurred_loop(img, blur, mask=None, max_valid=-1):
    """The definition once more as a pixel loop in Python integers (small frames only): (v, tap) as lists of lists."""
    H, W = img.shape
    w1 = W1[blur]
    r = len(w1) // 2

    def is_tap(y, x):
        if not (0 <= y < H and 0 <= x < W):
            return False
        p = int(img[y, x])
        return not ((mask is not None and not mask[y, x]) or (max_valid >= 0 and p > max_valid) or (img.dtype.itemsize == 4 and p >= 1 << 24))

    v = [[0] * W for _ in range(H)]
    tap = [[False] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if not is_tap(y, x):
                continue
            S = Wn = 0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    if is_tap(y + dy, x + dx):
                        w = w1[dy + r] * w1[dx + r]
                        S += w * int(img[y + dy, x + dx])
                        Wn += w
            assert Wn >= w1[r] * w1[r] and S < 1 << 32
            v[y][x], tap[y][x] = S // Wn, True
    return v, tap
