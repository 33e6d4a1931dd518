"""The per-spot constant background (ffs_stream_spot_backgrounds, include/ffs_hip.h) in NumPy, in the histogram form the header states:
the ring of `border` pixels around a bounding box, its valid pixels, 256 one-count bins and a tail, quartiles by 1-based position, the
integer fence.  The checker, never the thing tested; tests/test_spot_background_oracle.py ties it to a sort-based form with float fences."""
import numpy as np

N_BINS = 256
OK, NO_PIXELS, OVERFLOW, RANGE, NO_INLIERS = 0, 1, 2, 3, 4
DT = np.dtype([("n_pixels", "<u4"), ("n_overflow", "<u4"), ("q1", "<i4"), ("median", "<i4"), ("q3", "<i4"), ("n_inliers", "<u4"),
               ("inlier_sum", "<u8"), ("status", "<u4"), ("reserved", "<u4"), ("mean", "<f8")])
INTEGER_FIELDS = ["n_pixels", "n_overflow", "q1", "median", "q3", "n_inliers", "inlier_sum", "status"]


def ring_values(frame, mask, max_valid, box, border):
    """The valid pixels of the ring around box = (x_min, x_max, y_min, y_max), as uint64, in no particular order."""
    H, W = frame.shape
    x_min, x_max, y_min, y_max = (int(v) for v in box)
    X0, X1, Y0, Y1 = max(x_min - border, 0), min(x_max + border, W - 1), max(y_min - border, 0), min(y_max + border, H - 1)
    take = np.ones((Y1 - Y0 + 1, X1 - X0 + 1), bool)
    take[y_min - Y0:y_max - Y0 + 1, x_min - X0:x_max - X0 + 1] = False          # the box itself contributes nothing
    v = frame[Y0:Y1 + 1, X0:X1 + 1].astype(np.uint64)
    if mask is not None:
        take &= mask[Y0:Y1 + 1, X0:X1 + 1] != 0
    if max_valid >= 0:
        take &= v <= max_valid
    if frame.dtype.itemsize == 4:
        take &= v < (1 << 24)
    return v[take]


def histogram(values):
    v = np.asarray(values, np.uint64)
    low = v[v < N_BINS].astype(np.int64)
    return np.bincount(low, minlength=N_BINS).astype(np.uint32), int((v >= N_BINS).sum())


def from_histogram(bins, tail):
    """(n_pixels, n_overflow, q1, median, q3, n_inliers, inlier_sum, status) of 256 bin counts and a tail count: Python integers."""
    bins = np.asarray(bins, np.int64)
    N = int(bins.sum()) + int(tail)
    if N == 0:
        return (0, int(tail), -1, -1, -1, 0, 0, NO_PIXELS)
    if 4 * tail > N:
        return (N, int(tail), -1, -1, -1, 0, 0, OVERFLOW)
    cum = np.cumsum(bins)
    q1, med, q3 = (int(np.searchsorted(cum, p, "left")) for p in ((N + 3) // 4, (N + 1) // 2, (3 * N + 1) // 4))
    assert q1 < N_BINS and med < N_BINS and q3 < N_BINS
    iqr = q3 - q1
    if 2 * q3 + 3 * iqr >= 2 * N_BINS:
        return (N, int(tail), q1, med, q3, 0, 0, RANGE)
    v = np.arange(N_BINS)
    inl = (2 * q1 - 3 * iqr <= 2 * v) & (2 * v <= 2 * q3 + 3 * iqr)
    n_in, s_in = int(bins[inl].sum()), int((bins[inl] * v[inl]).sum())
    if n_in == 0:
        return (N, int(tail), q1, med, q3, 0, 0, NO_INLIERS)
    return (N, int(tail), q1, med, q3, n_in, s_in, OK)


def from_values(values):
    return from_histogram(*histogram(values))


def spot_backgrounds(frame, mask, max_valid, boxes, border):
    """One record (DT) per box of one frame; boxes: rows (x_min, x_max, y_min, y_max)."""
    out = np.zeros(len(boxes), DT)
    for i, box in enumerate(boxes):
        rec = from_values(ring_values(frame, mask, max_valid, box, border))
        for name, val in zip(INTEGER_FIELDS, rec):
            out[name][i] = val
        if rec[-1] == OK:
            out["mean"][i] = float(rec[6]) / float(rec[5])     # (both below 2^53: the same float64 division as the library's)
    return out


def batch_backgrounds(frames, mask, max_valid, reflections_per_frame, border):
    """The batch's records in the order of ffs_stream_batch_arrays: reflections_per_frame[i] is frame i's reflection array (x_min .. y_max)."""
    parts = [spot_backgrounds(f, mask, max_valid, np.stack([r["x_min"], r["x_max"], r["y_min"], r["y_max"]], axis=1) if len(r) else np.zeros((0, 4), int), border)
             for f, r in zip(frames, reflections_per_frame)]
    return np.concatenate(parts) if parts else np.zeros(0, DT)
