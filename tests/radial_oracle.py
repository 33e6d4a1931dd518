"""The truth of the per-frame radial profile (ffs_ctx_set_radial_bins): count, sum and sum of squares per bin, as exact integers.

A pixel (x, y) counts into bin b = bins[y, x] when b != 0xFFFF, the mask is set there, p <= max_valid when max_valid >= 0, and -- for
32-bit pixels -- p < 2^24 (the oracle's neighbour rule).  The sums are uint64 with the wrap of sum_sq written out in uint64
arithmetic: np.bincount's weights are float64 and would lose bits, so the weighted sums go through np.add.at on uint64 arrays.
"""
import numpy as np

NO_BIN = 0xFFFF


def included(img, bins, mask=None, max_valid=-1):
    """The inclusion rule as a boolean H x W array."""
    img = np.asarray(img)
    bins = np.asarray(bins)
    assert img.shape == bins.shape and img.dtype in (np.dtype(np.uint16), np.dtype(np.uint32))
    ok = bins != NO_BIN
    if mask is not None:
        ok &= np.asarray(mask) != 0
    if max_valid >= 0:
        ok &= img.astype(np.int64) <= int(max_valid)
    if img.dtype == np.dtype(np.uint32):
        ok &= img < (1 << 24)
    return ok


def radial_profile(img, bins, n_bins, mask=None, max_valid=-1):
    """-> (count uint32[n_bins], sum uint64[n_bins], sum_sq uint64[n_bins], the last modulo 2^64)."""
    ok = included(img, bins, mask, max_valid)
    b = np.asarray(bins)[ok].astype(np.int64)
    p = np.asarray(img)[ok].astype(np.uint64)
    assert b.size == 0 or int(b.max()) < n_bins
    count = np.bincount(b, minlength=n_bins).astype(np.uint32)
    s = np.zeros(n_bins, np.uint64)
    q = np.zeros(n_bins, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(s, b, p)
        np.add.at(q, b, p * p)   # (p < 2^32: the product is exact in uint64; the additions wrap modulo 2^64)
    return count, s, q


def radial_profile_loop(img, bins, n_bins, mask=None, max_valid=-1):
    """The same by a plain loop over the pixels in Python integers (small frames only)."""
    img = np.asarray(img)
    H, W = img.shape
    is32 = img.dtype == np.dtype(np.uint32)
    count, s, q = [0] * n_bins, [0] * n_bins, [0] * n_bins
    for y in range(H):
        for x in range(W):
            b, p = int(bins[y][x]), int(img[y][x])
            if b == NO_BIN:
                continue
            if mask is not None and not mask[y][x]:
                continue
            if max_valid >= 0 and p > max_valid:
                continue
            if is32 and p >= 1 << 24:
                continue
            count[b] += 1
            s[b] += p
            q[b] += p * p
    return (np.array(count, np.uint32), np.array([v % (1 << 64) for v in s], np.uint64),
            np.array([v % (1 << 64) for v in q], np.uint64))


def shell_bins(W, H, n_bins, cx=None, cy=None):
    """Concentric shells of equal width in r^2 about (cx, cy): a realistic map for tests (long runs of equal bins)."""
    cx = W / 2.0 if cx is None else cx
    cy = H / 2.0 if cy is None else cy
    y, x = np.mgrid[0:H, 0:W]
    r2 = (x + 0.5 - cx) ** 2 + (y + 0.5 - cy) ** 2
    top = r2.max()
    return np.minimum((r2 / top * n_bins).astype(np.int64), n_bins - 1).astype(np.uint16) if top > 0 else np.zeros((H, W), np.uint16)
