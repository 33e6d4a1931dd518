"""GPU: the blur of the radial-profile threshold (ffs_ctx_set_radial_blur narrow | wide), held bit for bit to tests/radial_blur_oracle.py
through the C ABI: strong pixels, everything behind them, and every field of every shell record.

Everything is integers, so every comparison is array_equal.  The shapes are test_gpu_radial_threshold.py's -- (517, 41) is one 512-pixel
wave row with a tail (and, for the blurred kernels, two strips of 62 groups and two runs of 32 rows), (1030, 3) three wave rows with fewer
rows than the kernel is high, (8, 1) and (2, 2) frames smaller than either kernel -- and (5, 5).  How one pixel's v is read from outside: a
shell that holds that pixel alone has q1 = median = q3 = v."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import radial_blur_oracle as RB
import radial_oracle as R
import radial_threshold_oracle as RT
from util import assert_frame_matches_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HOST = os.path.join(ROOT, "fast-feedback-service_amd", "host")
NO_BIN = RT.NO_BIN
SHAPES = [(37, 29), (517, 41), (1030, 3), (8, 1), (2, 2), (5, 5)]
FIELDS = ("n_pixels", "n_overflow", "q1", "median", "q3", "cutoff", "status", "reserved")
BLURS = {"none": RB.NONE, "narrow": RB.NARROW, "wide": RB.WIDE}
DTYPES = [np.uint16, np.uint32]
blur_param = pytest.mark.parametrize("blur", ["narrow", "wide"])
dtype_param = pytest.mark.parametrize("dtype", DTYPES, ids=["u16", "u32"])


def _shells(W, H):
    return R.shell_bins(W, H, 16, cx=W * 0.4, cy=H * 0.6)


def _maps(W, H, seed):
    """test_gpu_radial_threshold.py's bin maps."""
    rng = np.random.default_rng(seed)
    every_second = R.shell_bins(W, H, 5).copy()
    every_second.reshape(-1)[1::2] = NO_BIN
    return {
        "shells": (_shells(W, H), 16),
        "random_40": (rng.integers(0, 40, (H, W)).astype(np.uint16), 40),
        "one_bin": (np.zeros((H, W), np.uint16), 1),
        "every_second_none": (every_second, 5),
        "all_none": (np.full((H, W), NO_BIN, np.uint16), 4),
        "random_128": (rng.integers(0, 128, (H, W)).astype(np.uint16), 128),
    }


def _truth(frames, bins, n_bins, blur, mask=None, max_valid=-1, n_iqr=6.0, thr=0.0):
    """The oracle's (strong, shells) of every frame: computed once, shared by the runs that must all equal it."""
    return [RB.threshold(img, bins, n_bins, BLURS.get(blur, blur), n_iqr, thr, mask, max_valid) for img in frames]


def _check(st, res, frames, truth, mask=None, min_spot_size=3):
    """Every frame's results and shell records against the oracle's; -> strong pixels of the batch."""
    total = 0
    ones = np.ones(frames[0].shape, np.uint8)
    for f, img in enumerate(frames):
        strong, shells = truth[f]
        assert_frame_matches_oracle(res[f], img, ones if mask is None else mask, min_spot_size=min_spot_size, strong=strong)
        got = st.radial_thresholds(f)
        assert got.dtype == RT.SHELL_DT and len(got) == len(shells)
        for name in FIELDS:
            assert np.array_equal(got[name], shells[name]), (f, name, got[name], shells[name])
        total += int(strong.sum())
    return total


def _context(ffs, W, H, dtype, bins, n_bins, blur, max_batch=3, mask=None, n_iqr=None, tuning=None, **params):
    ctx = ffs.Context(W, H, dtype, max_batch=max_batch)
    if mask is not None:
        ctx.set_mask(mask)
    if tuning:
        ctx.set_tuning(**tuning)
    ctx.set_radial_bins(bins, n_bins)
    if n_iqr is not None:
        ctx.set_radial_threshold(n_iqr)
    ctx.set_radial_blur(blur)
    ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=1, want_strong_list=1, want_reflections=1, **params)
    return ctx


def _resident(ctx, frames, fill=None):
    """The frames in the library's pitched device layout; the padding beyond W and behind the last row holds `fill` (default: all ones)."""
    import torch
    pitch, fstride = ctx.device_layout()
    B, H, W = frames.shape
    item = frames.dtype.itemsize
    host = np.full((B, fstride // item), np.iinfo(frames.dtype).max if fill is None else fill, frames.dtype)
    host[:, :H * (pitch // item)].reshape(B, H, pitch // item)[:, :, :W] = frames
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).to("cuda:0"), pitch, fstride


# ---- shapes x pixel sizes x kernels x batches of 1 and 3 x maps
@dtype_param
@blur_param
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_maps(ffs, shape, blur, dtype):
    W, H = shape
    frames = RB.fixture_frames(dtype, 3, H, W, _shells(W, H), seed=W * 31 + H)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    ctx.set_radial_blur(blur)
    st = ctx.stream()
    for name, (bins, n_bins) in _maps(W, H, seed=5).items():
        ctx.set_radial_bins(bins, n_bins)
        ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=1, want_strong_list=1, want_reflections=1)
        truth = _truth(frames, bins, n_bins, blur)
        plain = _truth(frames, bins, n_bins, RB.NONE)
        for B in (1, 3):
            res = st.process(frames[:B])
            path = st.last_path()[0]
            assert {"radial_threshold", "radial_blur", "radial"} <= path, (name, path)
            total = _check(st, res, frames[:B], truth[:B])
            if name == "shells" and W * H > 1000:
                assert total >= 20, (name, B, total)
                # the fixture tells the blurred decision from the unblurred one
                assert sum(int((a[0] != b[0]).sum()) for a, b in zip(truth[:B], plain[:B])) >= 10
            if name == "all_none":
                assert total == 0
            for f in range(B):      # the radial profile of the same batch is the raw pixels'
                for a, b in zip(st.radial_profile(f), R.radial_profile(frames[f], bins, n_bins)):
                    assert np.array_equal(a, b), (name, f)


# ---- 1. frame seams in a batch: rows -1, -2, H and H + 1 contribute nothing
@dtype_param
@blur_param
def test_frame_seams_in_a_batch(ffs, blur, dtype):
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    frames = np.full((3, H, W), 3, dtype)
    frames[1, :2] = frames[1, -2:] = 40000       # bright first and last rows between dark neighbours ...
    frames[0, :2] = frames[2, -2:] = 0           # ... and dark ones beside the bright
    frames[0, -2:] = frames[2, :2] = 50000
    truth = _truth(frames, bins, n_bins, blur)
    ctx = _context(ffs, W, H, dtype, bins, n_bins, blur, min_spot_size=1)
    st = ctx.stream()
    assert _check(st, st.process(frames), frames, truth, min_spot_size=1) >= 1
    mem, pitch, fstride = _resident(ctx, frames)
    st.submit_device(mem.data_ptr(), pitch, fstride, 3)
    _check(st, st.wait(), frames, truth, min_spot_size=1)
    # (the oracle blurs frame by frame: a neighbouring frame's bright rows that reached a dark first or last row would show above)
    v, _ = RB.blurred(frames[1], BLURS[blur])
    assert (v[4:-4] == 3).all() and (RB.blurred(frames[0], BLURS[blur])[0][0] == 0).all()
    for order in ([1, 0, 2], [2, 1, 0]):
        _check(st, st.process(frames[order]), frames[order], [truth[i] for i in order], min_spot_size=1)


# ---- 2. pitch padding: anything may lie beyond W
@dtype_param
@blur_param
def test_pitch_padding(ffs, blur, dtype):
    for W, H in ((517, 41), (37, 29), (5, 5)):
        bins, n_bins = _shells(W, H), 16
        frames = RB.fixture_frames(dtype, 3, H, W, bins, seed=77)
        frames[:, :, -2:] = 3                                   # quiet last columns: a padding that leaked in would show
        truth = _truth(frames, bins, n_bins, blur)
        ctx = _context(ffs, W, H, dtype, bins, n_bins, blur)
        st = ctx.stream()
        _check(st, st.process(frames), frames, truth)
        packed = [(r.strong_k.copy(), st.radial_thresholds(f).copy()) for f, r in enumerate(st.process(frames))]
        for fill in (0xFFFF, 0, 1000):
            mem, pitch, fstride = _resident(ctx, frames, fill)
            if W == 517:
                assert pitch // frames.dtype.itemsize > W
            st.submit_device(mem.data_ptr(), pitch, fstride, 3)
            res = st.wait()
            _check(st, res, frames, truth)
            for f, r in enumerate(res):
                assert np.array_equal(r.strong_k, packed[f][0]) and np.array_equal(st.radial_thresholds(f), packed[f][1])


# ---- 3. lane, wave, strip and run seams: one-hot and two-hot frames, every pixel of the footprint read through a shell of its own
SEAM_X = [0, 6, 7, 8, 9, 494, 495, 496, 497, 510, 511, 512, 513, 515, 516]       # lanes; the strip of 62 groups (496); the 512-pixel wave row; W - 2, W - 1
SEAM_Y = [0, 1, 2, 6, 7, 8, 9, 31, 32, 39, 40]                                    # the 8-row tile; the run of 32 rows; H - 2, H - 1


def _footprint(hot, r, W, H):
    return sorted({(y + dy, x + dx) for x, y in hot for dy in range(-r, r + 1) for dx in range(-r, r + 1) if 0 <= y + dy < H and 0 <= x + dx < W})


def _pack(groups, r, per_batch):
    """Batches of at most `per_batch` groups of hot pixels whose footprints (and the pixels they reach) do not meet."""
    batches = []
    for g in groups:
        for b in batches:
            if len(b) < per_batch and all(abs(x - x2) > 4 * r or abs(y - y2) > 4 * r for x, y in g for g2 in b for x2, y2 in g2):
                b.append(g)
                break
        else:
            batches.append([g])
    return batches


def _hot_run(ffs, dtype, blur, groups, value, per_batch, W=517, H=41):
    """Frames of 2 with the hot pixels of one group each at `value`; every pixel of every footprint of the batch sits in a shell of its own,
    so its v is that shell's median (bin 0: everything else).  The records and results equal the oracle's."""
    r = BLURS[blur]
    ctx = _context(ffs, W, H, dtype, np.zeros((H, W), np.uint16), 1, blur, max_batch=per_batch, min_spot_size=1)
    st = ctx.stream()
    seen = 0
    for batch in _pack(groups, r, per_batch):
        bins = np.zeros((H, W), np.uint16)
        n_bins = 1
        for g in batch:
            for y, x in _footprint(g, r, W, H):
                bins[y, x] = n_bins
                n_bins += 1
        assert n_bins <= 128
        frames = np.full((len(batch), H, W), 2, dtype)
        for f, g in enumerate(batch):
            for x, y in g:
                frames[f, y, x] = value
        ctx.set_radial_bins(bins, n_bins)
        truth = _truth(frames, bins, n_bins, blur)
        res = st.process(frames)
        _check(st, res, frames, truth, min_spot_size=1)
        for f, g in enumerate(batch):       # the test sees what it means to see: each footprint pixel's own v, all different from the background's
            v, _ = RB.blurred(frames[f], r)
            got = st.radial_thresholds(f)
            for y, x in _footprint(g, r, W, H):
                b = int(bins[y, x])
                assert v[y, x] > 2 and v[y, x] < 256, (x, y, v[y, x])
                assert got["n_pixels"][b] == 1 and got["status"][b] == RT.OK and got["median"][b] == v[y, x], (g, x, y, got[b], v[y, x])
                seen += 1
    return seen


@dtype_param
@blur_param
def test_one_hot_seams(ffs, blur, dtype):
    # (500: at the image's corner the hot pixel holds 4 / 9 of the narrow kernel's weight, and v stays below 256)
    seen = _hot_run(ffs, dtype, blur, [[(x, y)] for x in SEAM_X for y in SEAM_Y], value=500, per_batch=5)
    assert seen > len(SEAM_X) * len(SEAM_Y) * (2 * BLURS[blur] + 1) ** 2 // 2


@dtype_param
@blur_param
def test_two_hot_seams(ffs, blur, dtype):
    pairs = [[(x, y), (x + 1, y)] for x in (7, 495, 511, 515) for y in (0, 7, 8, 31, 40)]
    pairs += [[(x, y), (x, y + 1)] for x in (0, 8, 496, 512, 516) for y in (0, 7, 31, 39)]
    pairs += [[(x, y), (x + 1, y + 1)] for x in (7, 495, 511) for y in (7, 31)]
    _hot_run(ffs, dtype, blur, pairs, value=300, per_batch=3)


# ---- 4. band seams of the histogram launch; 8. independence of tuning and path
@dtype_param
@blur_param
def test_bands_tuning_and_paths(ffs, blur, dtype):
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    mask = RB.gappy_mask(W, H, 8)
    frames = RB.fixture_frames(dtype, 3, H, W, bins, seed=21)
    truth = _truth(frames, bins, n_bins, blur, mask)
    variants = [{"radthr_bands": b} for b in (1, 2, 5, H)] + [{"sparse_stage": s} for s in (1, 2, 3)]
    variants += [{"radthr_form": f, "radthr_bands": 5} for f in (1, 2)] + [{"dense_mask": 1}, {"window_kernel": 1, "threshold_path": 1}]
    reference = None
    for tuning in [{}] + variants:
        ctx = _context(ffs, W, H, dtype, bins, n_bins, blur, mask=mask, tuning=tuning)
        st = ctx.stream()
        res = st.process(frames)
        assert _check(st, res, frames, truth, mask) >= 20
        assert "radial_blur" in st.last_path()[0], tuning
        now = [(r.strong_k.copy(), st.radial_thresholds(f).copy()) for f, r in enumerate(res)]
        if reference is None:
            reference = now
            mem, pitch, fstride = _resident(ctx, frames)        # resident frames
            st.submit_device(mem.data_ptr(), pitch, fstride, 3)
            _check(st, st.wait(), frames, truth, mask)
            ms_hist, ms_rest = st.bench_threshold(mem.data_ptr(), pitch, fstride, 3, 2)     # the measurement times the blurred forms and leaves the stream usable
            assert 0.0 < ms_hist < 100.0 and 0.0 < ms_rest < 100.0
            _check(st, st.process(frames), frames, truth, mask)
        for (ka, sa), (kb, sb) in zip(reference, now):
            assert np.array_equal(ka, kb) and np.array_equal(sa, sb), tuning
    for want in ((0, 0), (1, 0), (0, 1)):
        ctx = _context(ffs, W, H, dtype, bins, n_bins, blur, mask=mask)
        ctx.set_params(want_strong_mask=want[0], want_strong_list=want[1])
        st = ctx.stream()
        _check(st, st.process(frames), frames, truth, mask)


# ---- 5. both division paths
@dtype_param
@blur_param
def test_division_paths(ffs, blur, dtype):
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    mask = RB.gappy_mask(W, H, 3)
    mask[20:25, 100:105] = 0
    mask[22, 102] = 1                                          # an isolated valid pixel ringed by masked ones: v = p
    mask[8:13, 508:516] = 0
    mask[10, 511] = mask[10, 512] = 1                          # ... and two across the wave row's seam
    frames = RB.fixture_frames(dtype, 2, H, W, bins, seed=11)
    frames[:, 22, 102] = 77
    for img in frames:
        S, Wn, tap = RB.sums(img, BLURS[blur], mask)
        assert int((tap & (Wn == RB.FULL[BLURS[blur]])).sum()) > 1000 and int((tap & (Wn != RB.FULL[BLURS[blur]])).sum()) > 1000
        assert RB.blurred(img, BLURS[blur], mask)[0][22, 102] == 77
    ctx = _context(ffs, W, H, dtype, bins, n_bins, blur, max_batch=2, mask=mask)
    st = ctx.stream()
    total = _check(st, st.process(frames), frames, _truth(frames, bins, n_bins, blur, mask), mask)
    assert total >= 20
    per_scope = []
    truth = _truth(frames, bins, n_bins, blur, mask, max_valid=1000)
    assert (frames > 1000).sum() > 100
    for scope in ("centre", "window"):                          # max_valid with pixels above it, under both scopes: the same results
        ctx.set_max_valid_scope(scope)
        ctx.set_params(max_valid=1000)
        res = st.process(frames)
        t = _check(st, res, frames, truth, mask)
        assert 1 <= t
        per_scope.append([(r.strong_k.copy(), st.radial_thresholds(f).copy()) for f, r in enumerate(res)])
    for (ka, sa), (kb, sb) in zip(*per_scope):
        assert np.array_equal(ka, kb) and np.array_equal(sa, sb)


@dtype_param
@blur_param
def test_decision_ties(ffs, blur, dtype):
    """A one-shell map over a frame of 10 (cutoff 10): a pixel whose S is (cutoff + 1) Wn - 1 is not strong, one at (cutoff + 1) Wn is; at the
    full Wn and at a renormalised one (a corner tap masked)."""
    W, H = 517, 41
    r = BLURS[blur]
    w1 = RB.W1[r]
    wc, full = w1[r] * w1[r], RB.FULL[r]
    bins = np.zeros((H, W), np.uint16)
    mask = np.ones((H, W), np.uint8)
    img = np.full((H, W), 10, dtype)
    spots = {}
    # (x, y) of four targets, the second pair with the corner tap at (x - r, y - r) masked; one pair astride the strip seam at x = 496
    for name, (x, y), renorm, strong in (("full_below", (100, 10), False, 0), ("full_at", (496, 10), False, 1),
                                         ("renorm_below", (300, 30), True, 0), ("renorm_at", (495, 31), True, 1)):
        wn = full - 1 if renorm else full
        target = 11 * wn - 1 + strong
        img[y - r:y + r + 1, x - r:x + r + 1] = 0
        if renorm:
            mask[y - r, x - r] = 0
        pc = (target - 8) // wc
        img[y, x] = pc
        img[y + r, x + r] = target - wc * pc                   # a corner tap of weight 1 carries the remainder
        spots[name] = (x, y, wn, target, strong)
    S, Wn, tap = RB.sums(img, r, mask)
    (strong, shells), = _truth(img[None], bins, 1, blur, mask)
    assert shells["cutoff"][0] == 10 and shells["status"][0] == RT.OK
    for name, (x, y, wn, target, want) in spots.items():
        assert (S[y, x], Wn[y, x]) == (target, wn) and strong[y, x] == want, name
    ctx = _context(ffs, W, H, dtype, bins, 1, blur, max_batch=1, mask=mask, min_spot_size=1)
    st = ctx.stream()
    res = st.process(img[None])
    _check(st, res, img[None], [(strong, shells)], mask, min_spot_size=1)
    for name, (x, y, wn, target, want) in spots.items():
        assert res[0].strong_mask[y, x] == want, name
    # `threshold` just below and at a blurred value: (double)v > threshold
    x, y = spots["full_at"][:2]
    for thr, want in ((10.5, 1), (11.0, 0)):
        ctx.set_params(threshold=thr)
        res = st.process(img[None])
        _check(st, res, img[None], _truth(img[None], bins, 1, blur, mask, thr=thr), mask, min_spot_size=1)
        assert res[0].strong_mask[y, x] == want, thr


# ---- 6. the 32-bit range
def test_32_bit_range(ffs):
    top = (1 << 24) - 1
    for W, H in ((37, 29), (517, 41)):
        bins = np.zeros((H, W), np.uint16)
        img = np.full((H, W), 5, np.uint32)
        for x, y in ((10, 10), (W - 12, H - 12)):
            img[y - 4:y + 5, x - 4:x + 5] = 1 << 24
            img[y - 4:y + 5:2, x - 4:x + 5:3] = 0xFFFFFFFF
            img[y - 3:y + 5:2, x - 4:x + 5:2] = (1 << 24) + 9
            img[y - 2:y + 3, x - 2:x + 3] = top                 # a 5 x 5 block of 2^24 - 1 whose neighbours are no taps
        S, Wn, tap = RB.sums(img, RB.WIDE)
        assert S[10, 10] == 4294967040 and Wn[10, 10] == 256
        for blur in ("wide", "narrow"):
            truth = _truth(img[None], bins, 1, blur)
            v, _ = RB.blurred(img, BLURS[blur])
            assert (v[8:13, 8:13] == top).all() and truth[0][0][8:13, 8:13].all() and not truth[0][0][img >= 1 << 24].any()
            ctx = _context(ffs, W, H, np.uint32, bins, 1, blur, max_batch=1, min_spot_size=1)
            st = ctx.stream()
            res = st.process(img[None])
            _check(st, res, img[None], truth, min_spot_size=1)
            assert st.radial_thresholds(0)["n_overflow"][0] == 50


# ---- 7. the p >= 1 clause
@dtype_param
@blur_param
def test_a_zero_pixel_is_never_strong(ffs, blur, dtype):
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    img = np.full((H, W), 3, dtype)
    zeros, ones = [], []
    for x, y in ((8, 8), (496, 20), (511, 31), (300, 0), (516, 40)):       # blobs at the seams, zero and one-valued pixels beside them
        img[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 5000
        for dx, dy, val in ((-2, 0, 0), (0, -2, 1), (-2, -1, 1), (-2, 1, 0)):
            if 0 <= x + dx < W and 0 <= y + dy < H:
                img[y + dy, x + dx] = val
                (zeros if val == 0 else ones).append((y + dy, x + dx))
    (strong, shells), = truth = _truth(img[None], bins, n_bins, blur)
    v, _ = RB.blurred(img, BLURS[blur])
    assert len(zeros) >= 6 and len(ones) >= 6
    for y, x in zeros:
        assert v[y, x] > shells["cutoff"][bins[y, x]] and strong[y, x] == 0
    for y, x in ones:
        assert strong[y, x] == 1
    ctx = _context(ffs, W, H, dtype, bins, n_bins, blur, max_batch=1, min_spot_size=1)
    st = ctx.stream()
    res = st.process(img[None])
    _check(st, res, img[None], truth, min_spot_size=1)
    for y, x in zeros:
        assert res[0].strong_mask[y, x] == 0
    for y, x in ones:
        assert res[0].strong_mask[y, x] == 1
    assert (img.reshape(-1)[res[0].strong_k] >= 1).all()


# ---- 9. the snapshot: the setting changes between submit and wait, batch after batch on one stream
def test_snapshot_per_batch(ffs):
    from oracle import oracle as O
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    mask = RB.gappy_mask(W, H, 4)
    frames = RB.fixture_frames(np.uint16, 3, H, W, bins, seed=55)
    ctx = ffs.Context(W, H, np.uint16, max_batch=3)
    ctx.set_mask(mask)
    ctx.set_radial_bins(bins, n_bins)
    st = ctx.stream()
    truths = {b: _truth(frames, bins, n_bins, b, mask) for b in ("none", "narrow", "wide")}
    sequence = [("radial", "none"), ("radial", "narrow"), ("radial", "wide"), ("dispersion", "wide"), ("radial", "narrow"), ("radial", "none"),
                ("dispersion", "narrow"), ("radial", "wide"), ("radial", "wide"), ("radial", "none")]

    def apply(algo, blur):
        ctx.set_radial_blur(blur)
        ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE if algo == "radial" else ffs.ALGO_DISPERSION, want_strong_mask=1, want_strong_list=1, want_reflections=1)

    for i, (algo, blur) in enumerate(sequence):
        apply(algo, blur)
        batch = frames if i % 2 == 0 else frames[::-1]
        st.submit(batch)
        apply(*sequence[(i + 1) % len(sequence)])           # the batch in flight keeps what it was submitted with
        res = st.wait()
        path = st.last_path()[0]
        if algo == "radial":
            truth = truths[blur] if i % 2 == 0 else truths[blur][::-1]
            assert _check(st, res, batch, truth, mask) >= 1
            assert "radial_threshold" in path and ("radial_blur" in path) == (blur != "none"), (i, path)
        else:
            for fr, img in zip(res, batch):
                assert_frame_matches_oracle(fr, img, mask)
            assert "radial_threshold" not in path and "radial_blur" not in path, (i, path)
    assert not np.array_equal(truths["none"][0][0], truths["narrow"][0][0]) and not np.array_equal(truths["narrow"][0][0], truths["wide"][0][0])


# ---- 10. a batch that ffs_wait runs again keeps its blur
@blur_param
def test_recovery(ffs, blur):
    """test_gpu_radial_threshold.py's test_recovery under a blur: n_iqr = 0 on noise puts about half of the first frame's pixels above their
    shell's median of v, more than the one launch's forest and the lists hold -- the batch is run again, and that frame then on its own on a
    one-frame stream, which must blur as the batch did.  (240 rows where that test has 80: the blurred noise is smoother, and its strong pixels
    lie in 34 000 runs under the narrow kernel and 26 000 under the wide one, where the unblurred noise has 20 000 in 80 rows.)"""
    W, H = 1030, 240
    bins, n_bins = _shells(W, H), 16
    rng = np.random.default_rng(33)
    quiet = np.full((H, W), 2)
    quiet[5, 5], quiet[40, 700] = 1000, 900
    frames = np.stack([rng.integers(0, 256, (H, W)), quiet]).astype(np.uint16)
    truth = _truth(frames, bins, n_bins, blur, n_iqr=0.0)
    ctx = ffs.Context(W, H, np.uint16, max_batch=2, max_strong_per_frame=28000)
    ctx.set_tuning(chain_runs=2)
    ctx.set_radial_bins(bins, n_bins)
    ctx.set_radial_threshold(0.0)
    ctx.set_radial_blur(blur)
    ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=1, want_strong_list=1, want_reflections=1, min_spot_size=1)
    st = ctx.stream()
    st.submit(frames)
    ctx.set_radial_blur("none")                                 # (the re-run happens inside wait: it must not look at the context)
    res = st.wait()
    path, reruns = st.last_path()
    assert reruns > 0 and "radial_blur" in path, (path, reruns)
    assert res[0].num_strong_pixels > 28000 and res[1].num_strong_pixels == 2 * (2 * BLURS[blur] + 1) ** 2
    _check(st, res, frames, truth, min_spot_size=1)
    assert not np.array_equal(truth[0][0], RB.threshold(frames[0], bins, n_bins, RB.NONE, 0.0)[0])


# ---- 11. refusals
def test_refusals(ffs):
    W, H = 37, 29
    bins, n_bins = _shells(W, H), 16
    frames = RB.fixture_frames(np.uint16, 1, H, W, bins, seed=4)
    ctx = _context(ffs, W, H, np.uint16, bins, n_bins, "narrow", max_batch=1)
    st = ctx.stream()
    truth = _truth(frames, bins, n_bins, "narrow")

    def still_narrow():
        _check(st, st.process(frames), frames, truth)
        assert "radial_blur" in st.last_path()[0]

    still_narrow()
    for bad in (-1, 3, 1024, -2147483648):
        with pytest.raises(ffs.FfsError, match="ffs_ctx_set_radial_blur: blur must be FFS_RADIAL_BLUR_NONE \\(0\\), _NARROW \\(1\\) or _WIDE \\(2\\), got %d" % bad):
            ctx.set_radial_blur(bad)
        still_narrow()
    with pytest.raises(ValueError):
        ctx.set_radial_blur("medium")
    still_narrow()
    # kept across set_params; accepted under any algorithm, where it plays no part
    ctx.set_params(threshold=1.0)
    _check(st, st.process(frames), frames, _truth(frames, bins, n_bins, "narrow", thr=1.0))
    ctx.set_params(algorithm=ffs.ALGO_DISPERSION, threshold=0.0)
    ctx.set_radial_blur(ffs.RADIAL_BLUR_WIDE)
    for fr, img in zip(st.process(frames), frames):
        assert_frame_matches_oracle(fr, img, np.ones((H, W), np.uint8))
    assert "radial_blur" not in st.last_path()[0]
    ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE)
    _check(st, st.process(frames), frames, _truth(frames, bins, n_bins, "wide"))
    ctx.set_radial_blur(ffs.RADIAL_BLUR_NONE)
    res = st.process(frames)
    strong, shells = RT.threshold(frames[0], bins, n_bins)
    _check(st, res, frames, [(strong, shells)])
    assert "radial_blur" not in st.last_path()[0] and "radial_threshold" in st.last_path()[0]


# ---- 12. the driver
def _run(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", out), err, lines


def test_driver(ffs, tmp_path):
    from ffs_amd import synth
    N, SHELLS, N_IQR = 4, 16, 4.0
    exe = tmp_path / "radial_bins_check"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", HOST, os.path.join(ROOT, "tests", "radial_bins_check.cc"), "-o", str(exe)], check=True)
    subprocess.run([str(exe), "dump", str(tmp_path / "map.u16"), "300", "200", str(SHELLS), "0.976", "0.3", "150", "100", "0.75e-4", "0.75e-4"],
                   capture_output=True, text=True, check=True)
    bins = np.fromfile(tmp_path / "map.u16", "<u2").reshape(200, 300)
    common = ["synth:tiny:%d" % N, "--threads", "1", "--batch", "2", "--single-buffer", "--max-valid", "none", "-a", "radial_profile",
              "--radial-bins", str(SHELLS), "--n-iqr", "4"]
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    strong_by_blur = {}
    for blur, size in (("wide", 5), ("narrow", 3)):
        rc, out, err, lines = _run(common + ["--radial-blur", blur], tmp_path)
        assert rc == 0 and not err, (out, err)
        assert "Algorithm: Radial Profile" in out
        assert "Radial-profile threshold: a strong pixel stands above median + 4 x IQR of its shell\n" in out
        assert "Radial blur: %s, a %d x %d kernel over the valid pixels ahead of the threshold\n" % (blur, size, size) in out
        got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
        assert sorted(got) == list(range(N))
        strong_by_blur[blur] = []
        for z in range(N):
            strong, shells = RB.threshold(frames[z], bins, SHELLS, BLURS[blur], N_IQR)
            g = got[z]
            assert g["num_strong_pixels"] == int(strong.sum()) > 0
            assert g["radial_median"] == [int(v) for v in shells["median"]]
            assert g["radial_cutoff"] == [int(v) for v in shells["cutoff"]]
            assert g["radial_status"] == [int(v) for v in shells["status"]]
            assert list(g) == sorted(g)
            strong_by_blur[blur].append(int(strong.sum()))
    rc, out, err, lines = _run(common, tmp_path)                # without the option: no new line, the unblurred numbers
    assert rc == 0 and "Radial blur" not in out
    plain = [json.loads(l) for l in lines]
    assert sorted(g["num_strong_pixels"] for g in plain) != sorted(strong_by_blur["wide"])
