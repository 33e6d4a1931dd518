"""Jungfrau pedestals from dark frames (csrc/jungfrau_pedestal_model.hpp) restated in NumPy and Python integers: the fold of raw words into
per-pixel, per-stage accumulators, the planes (pedestal, rms, ok) and the re-pedestalled calibration.  The truth the kernel, the library's
host function, the driver and the check program are held to, bit for bit.  Also the frames the tests share."""
import numpy as np

MAX_FRAMES = (1 << 32) - 1


def word_counts(raw):
    """Which words count: not the gain code 2, not 0xFFFF, not 0xC000."""
    raw = np.asarray(raw, np.uint16)
    return ~(((raw >> 14) == 2) | (raw == 0xFFFF) | (raw == 0xC000))


def stage(raw):
    """0, 1, 2 for the gain codes 0, 1, 3 (2 for the code 2, whose words do not count)."""
    g = (np.asarray(raw, np.uint16) >> 14).astype(np.intp)
    return np.where(g >= 2, 2, g)


def zeros(H, W):
    """An empty accumulator set: [n_frames, count, sum, sum_sq]."""
    return [0, np.zeros((3, H, W), np.uint32), np.zeros((3, H, W), np.uint64), np.zeros((3, H, W), np.uint64)]


def fold(acc, raw):
    """raw: (H, W) or (n, H, W) words, added into acc in place (and returned)."""
    raw = np.asarray(raw, np.uint16)
    frames = raw.reshape(-1, *raw.shape[-2:])
    assert acc[0] + len(frames) <= MAX_FRAMES
    for fr in frames:
        ok, s, a = word_counts(fr), stage(fr), (fr & 0x3FFF).astype(np.uint64)
        for t in range(3):
            sel = ok & (s == t)
            acc[1][t] += sel.astype(np.uint32)
            acc[2][t] += np.where(sel, a, 0).astype(np.uint64)
            acc[3][t] += np.where(sel, a * a, 0).astype(np.uint64)
        acc[0] += 1
    return acc


def fold_loop(H, W, frames):
    """The same in Python integers, a word at a time: (n_frames, count, sum, sum_sq) as nested lists [stage][pixel]."""
    count = [[0] * (H * W) for _ in range(3)]
    total = [[0] * (H * W) for _ in range(3)]
    total_sq = [[0] * (H * W) for _ in range(3)]
    n = 0
    for fr in frames:
        for k, r in enumerate(np.asarray(fr, np.uint16).reshape(-1).tolist()):
            g, a = r >> 14, r & 0x3FFF
            if g == 2 or r == 0xFFFF or r == 0xC000:
                continue
            s = {0: 0, 1: 1, 3: 2}[g]
            count[s][k] += 1
            total[s][k] += a
            total_sq[s][k] += a * a
        n += 1
    return n, count, total, total_sq


def args_ok(min_frames, max_rms):
    return bool(min_frames >= 1 and np.isfinite(np.float32(max_rms)) and np.float32(max_rms) >= 0)


def planes(count, total, total_sq, min_frames=1, max_rms=0.0):
    """-> (pedestal float32, rms float32, ok bool) of count's shape.  float64 throughout, every operation rounded on its own; the
    integer-to-float64 conversions are NumPy's astype: to nearest, ties to even."""
    assert args_ok(min_frames, max_rms)
    count = np.asarray(count, np.uint32)
    total = np.asarray(total, np.uint64)
    total_sq = np.asarray(total_sq, np.uint64)
    some = count > 0
    c = np.where(some, count, 1).astype(np.float64)
    m = total.astype(np.float64) / c
    q = total_sq.astype(np.float64) / c
    mm = m * m
    v = q - mm
    rms = np.sqrt(np.where(v > 0, v, 0.0)).astype(np.float32)
    ped = m.astype(np.float32)
    max_rms = np.float32(max_rms)
    ok = some & (count >= min_frames) & ((max_rms == 0) | (rms <= max_rms))
    return np.where(some, ped, np.float32(0)).astype(np.float32), np.where(some, rms, np.float32(0)).astype(np.float32), ok


def repedestal(old_pedestal, old_factor, pedestal, ok):
    """-> (pedestal, factor) of the re-pedestalled calibration: the pedestals replaced, a factor kept where ok holds, 0 elsewhere."""
    del old_pedestal
    return np.asarray(pedestal, np.float32).copy(), np.where(ok, np.asarray(old_factor, np.float32), np.float32(0)).astype(np.float32)


def stage_mix_frames(n, H, W, seed):
    """n frames in which every run of eight consecutive pixels sees the three stages, the code 2 and invalid words (where W * H allows),
    the pattern shifting from frame to frame; ADCs over the whole range."""
    rng = np.random.default_rng(seed)
    k = np.arange(H * W)
    out = np.zeros((n, H * W), np.uint16)
    for i in range(n):
        code = np.array([0, 1, 3, 0, 2, 1, 3, 0], np.uint16)[(k + i) % 8]
        raw = (code << 14) | rng.integers(0, 0x4000, H * W).astype(np.uint16)
        sel = (k + 3 * i) % 8 == 3
        raw[sel] = np.where(rng.random(sel.sum()) < 0.5, 0xC000, 0xFFFF)
        out[i] = raw
    return out.reshape(n, H, W)


def uniform_frames(n, H, W, code, seed):
    """n frames wholly in the stage of gain code `code` (0, 1 or 3), ADC 1 .. 16383."""
    rng = np.random.default_rng(seed)
    return ((code << 14) | rng.integers(1, 0x4000, (n, H, W))).astype(np.uint16)
