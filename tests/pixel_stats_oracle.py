"""The truth of the per-pixel statistics over a run (ffs_ctx_set_pixel_stats): count, sum, sum of squares and maximum per pixel, as exact
integers.

A pixel value p of a frame counts at (x, y) when p <= max_valid (when max_valid >= 0) and -- for 32-bit pixels -- p < 2^24.  The valid-pixel
mask plays no part.  count is uint32, max uint32 (0 where count is 0), the sums uint64 with the wrap of sum_sq written out in uint64
arithmetic.  Frames are folded in one at a time, so a run may be fed in any number of pieces: the state is the tuple the functions return.
"""
import numpy as np


def counted(img, max_valid=-1):
    """The inclusion rule as a boolean array of img's shape."""
    img = np.asarray(img)
    assert img.dtype in (np.dtype(np.uint16), np.dtype(np.uint32))
    ok = np.ones(img.shape, bool)
    if max_valid >= 0:
        ok &= img.astype(np.int64) <= int(max_valid)
    if img.dtype == np.dtype(np.uint32):
        ok &= img < (1 << 24)
    return ok


def empty(H, W):
    """-> (n_frames, count, sum, sum_sq, max) of no frames."""
    return 0, np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint64), np.zeros((H, W), np.uint64), np.zeros((H, W), np.uint32)


def fold(state, frames, max_valid=-1):
    """state with the frames ([B, H, W] or [H, W]) folded in under max_valid: a new tuple, the old one is left as it is."""
    n, count, s, q, mx = state
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    count, s, q, mx = count.copy(), s.copy(), q.copy(), mx.copy()
    for img in frames:
        ok = counted(img, max_valid)
        p = np.where(ok, img, 0).astype(np.uint64)
        count += ok.astype(np.uint32)
        with np.errstate(over="ignore"):
            s += p
            q += p * p          # (p < 2^32: the product is exact in uint64; the additions wrap modulo 2^64)
        mx = np.maximum(mx, p.astype(np.uint32))
    return n + len(frames), count, s, q, mx


def pixel_stats(frames, max_valid=-1):
    frames = np.asarray(frames)
    return fold(empty(*frames.shape[-2:]), frames, max_valid)


def merge(a, b):
    """Two states of the same shape as one (what the driver does with several contexts): counts and sums add, maximum of the maxima."""
    with np.errstate(over="ignore"):
        return a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3], np.maximum(a[4], b[4])


def pixel_stats_loop(frames, max_valid=-1):
    """The same by a plain loop over frames and pixels in Python integers (small frames only)."""
    frames = np.asarray(frames)
    B, H, W = frames.shape
    is32 = frames.dtype == np.dtype(np.uint32)
    count = [[0] * W for _ in range(H)]
    s = [[0] * W for _ in range(H)]
    q = [[0] * W for _ in range(H)]
    mx = [[0] * W for _ in range(H)]
    for f in range(B):
        for y in range(H):
            for x in range(W):
                p = int(frames[f][y][x])
                if max_valid >= 0 and p > max_valid:
                    continue
                if is32 and p >= 1 << 24:
                    continue
                count[y][x] += 1
                s[y][x] += p
                q[y][x] += p * p
                mx[y][x] = max(mx[y][x], p)
    mod = 1 << 64
    return (B, np.array(count, np.uint32).reshape(H, W), np.array([[v % mod for v in r] for r in s], np.uint64).reshape(H, W),
            np.array([[v % mod for v in r] for r in q], np.uint64).reshape(H, W), np.array(mx, np.uint32).reshape(H, W))


def assert_equal(got, want, what=""):
    """array_equal on every plane, and n_frames."""
    assert got[0] == want[0], (what, "n_frames", got[0], want[0])
    for name, a, b, dt in zip(("count", "sum", "sum_sq", "max"), got[1:], want[1:], (np.uint32, np.uint64, np.uint64, np.uint32)):
        assert a.dtype == np.dtype(dt) and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            y, x = bad[0]
            raise AssertionError("%s %s: %d entries differ, first at (x = %d, y = %d): %d, want %d" % (what, name, len(bad), x, y, int(a[y, x]), int(b[y, x])))
