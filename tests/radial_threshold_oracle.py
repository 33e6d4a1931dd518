"""NumPy truth for the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE, include/ffs_hip.h): per frame and shell of a bin map the
count, the tail count, the three quartiles, the status and the cutoff floor(median + n_iqr * iqr); then the strong mask.

Two forms of the same definition: shells_sort takes the quartiles from the sorted values of a shell, shells_hist from a histogram of
one-count bins 0..255 and a tail, as the device does.  The cutoff is two float64 operations, each rounded on its own (NumPy float64
scalars never fuse)."""
import numpy as np

NO_BIN = 0xFFFF
OK, EMPTY, OVERFLOW = 0, 1, 2
VALUES = 256                      # one-count bins; a value at or above is in the tail
MAX_BINS = 128
SHELL_DT = np.dtype([("n_pixels", "<u4"), ("n_overflow", "<u4"), ("q1", "<i4"), ("median", "<i4"), ("q3", "<i4"), ("cutoff", "<u4"),
                     ("status", "<u4"), ("reserved", "<u4")])


def positions(n):
    """1-based sorted positions of q1, the median and q3 among n values (integer division)."""
    n = int(n)
    return (n + 3) // 4, (n + 1) // 2, (3 * n + 1) // 4


def cutoff(median, iqr, n_iqr):
    product = np.float64(n_iqr) * np.float64(iqr)
    return int(np.floor(np.float64(median) + product))


def counting(img, bins, mask=None, max_valid=-1):
    """The radial profile's rule: which pixels count in the shell their bin-map entry names."""
    ok = bins != NO_BIN
    if mask is not None:
        ok &= mask != 0
    if max_valid >= 0:
        ok &= img.astype(np.uint64) <= max_valid
    if img.dtype.itemsize == 4:
        ok &= img < (1 << 24)
    return ok


def _record(out, b, n, n_over, quartiles, n_iqr):
    """quartiles(position) -> the value at a 1-based sorted position that lies inside the bins."""
    out[b]["n_pixels"], out[b]["n_overflow"] = n, n_over
    out[b]["q1"] = out[b]["median"] = out[b]["q3"] = -1
    if n == 0:
        out[b]["status"] = EMPTY
        return
    p25, p50, p75 = positions(n)
    if p75 > n - n_over:
        out[b]["status"] = OVERFLOW
        return
    q1, med, q3 = quartiles(p25), quartiles(p50), quartiles(p75)
    out[b]["status"] = OK
    out[b]["q1"], out[b]["median"], out[b]["q3"] = q1, med, q3
    out[b]["cutoff"] = cutoff(med, q3 - q1, n_iqr)


def shells_sort(img, bins, n_bins, n_iqr=6.0, mask=None, max_valid=-1):
    ok = counting(img, bins, mask, max_valid)
    out = np.zeros(n_bins, SHELL_DT)
    for b in range(n_bins):
        v = np.sort(img[ok & (bins == b)].astype(np.int64))
        _record(out, b, len(v), int((v >= VALUES).sum()), lambda pos: int(v[pos - 1]), n_iqr)
    return out


def histograms(img, bins, n_bins, mask=None, max_valid=-1):
    """[n_bins][257]: the counters the device keeps."""
    ok = counting(img, bins, mask, max_valid)
    at = bins[ok].astype(np.int64) * (VALUES + 1) + np.minimum(img[ok].astype(np.int64), VALUES)
    return np.bincount(at, minlength=n_bins * (VALUES + 1)).reshape(n_bins, VALUES + 1).astype(np.uint32)


def shells_from_histograms(hist, n_iqr=6.0):
    out = np.zeros(len(hist), SHELL_DT)
    for b, h in enumerate(hist):
        cum = np.cumsum(h[:VALUES].astype(np.int64))
        _record(out, b, int(cum[-1]) + int(h[VALUES]), int(h[VALUES]), lambda pos: int(np.searchsorted(cum, pos, side="left")), n_iqr)
    return out


def shells_hist(img, bins, n_bins, n_iqr=6.0, mask=None, max_valid=-1):
    return shells_from_histograms(histograms(img, bins, n_bins, mask, max_valid), n_iqr)


def strong_mask(img, bins, shells, threshold=0.0, mask=None, max_valid=-1):
    """uint8 H x W: counts in shell b, b's status is 0, p > cutoff[b] (integers) and (double)p > threshold."""
    ok = counting(img, bins, mask, max_valid)
    idx = np.where(bins == NO_BIN, 0, bins).astype(np.int64)
    cut = shells["cutoff"].astype(np.int64)[idx]
    good = (shells["status"] == OK)[idx]
    p = img.astype(np.int64)
    return (ok & good & (p > cut) & (p.astype(np.float64) > float(threshold))).astype(np.uint8)


def threshold(img, bins, n_bins, n_iqr=6.0, thr=0.0, mask=None, max_valid=-1):
    """(strong mask, shells) of one frame, by the histogram form."""
    shells = shells_hist(img, bins, n_bins, n_iqr, mask, max_valid)
    return strong_mask(img, bins, shells, thr, mask, max_valid), shells


def shells_loop(img, bins, n_bins, n_iqr=6.0, mask=None, max_valid=-1):
    """The definition once more as a pixel loop in Python integers (small frames only)."""
    H, W = img.shape
    per = [[] for _ in range(n_bins)]
    for y in range(H):
        for x in range(W):
            b, p = int(bins[y, x]), int(img[y, x])
            if b == NO_BIN or (mask is not None and not mask[y, x]) or (max_valid >= 0 and p > max_valid) or (img.dtype.itemsize == 4 and p >= 1 << 24):
                continue
            per[b].append(p)
    out = np.zeros(n_bins, SHELL_DT)
    for b, v in enumerate(per):
        v.sort()
        _record(out, b, len(v), sum(1 for p in v if p >= VALUES), lambda pos: v[pos - 1], n_iqr)
    return out
