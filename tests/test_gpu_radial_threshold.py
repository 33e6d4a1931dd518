"""GPU: the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE, ffs_ctx_set_radial_threshold, ffs_stream_radial_thresholds), held bit for bit to
tests/radial_threshold_oracle.py.

Everything the algorithm computes is an integer but one product that is defined operation by operation, so every comparison is array_equal.
The shapes are test_gpu_radial.py's: (517, 41) crosses one 512-pixel wave row with a tail and the 8-row tile seam, (1030, 3) three wave
rows with fewer rows than a workgroup has waves, (8, 1) is one lane's load, (2, 2) less than that; no W is a multiple of 8 but 8 itself."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import radial_oracle as R
import radial_threshold_oracle as RT
from util import assert_frame_matches_oracle, assert_reflections_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HOST = os.path.join(ROOT, "fast-feedback-service_amd", "host")
NO_BIN = RT.NO_BIN
SHAPES = [(37, 29), (517, 41), (1030, 3), (8, 1), (2, 2)]
FIELDS = ("n_pixels", "n_overflow", "q1", "median", "q3", "cutoff", "status", "reserved")


def _shells(W, H):
    return R.shell_bins(W, H, 16, cx=W * 0.4, cy=H * 0.6)


def _frames(dtype, B, H, W, seed):
    """Poisson(3) + 20 x (shell mod 5), one shell raised by Poisson(400) so that it lands on OVERFLOW, 1 % bright pixels in 100..60000;
    32-bit frames also get values at and above 2^24.  The shells are the 16 off-centre ones."""
    rng = np.random.default_rng(seed)
    shell = _shells(W, H).astype(np.int64)
    f = rng.poisson(3.0, (B, H, W)).astype(np.int64) + 20 * (shell % 5)[None]
    raised = int(shell[0, W - 1])                                  # the corner's shell
    f += np.where(shell == raised, 1, 0)[None] * rng.poisson(400.0, (B, H, W))
    bright = rng.random((B, H, W)) < 0.01
    counts = np.bincount(shell.reshape(-1), minlength=16)
    counts[raised] = 0
    y, x = np.argwhere(shell == counts.argmax())[0]                 # (small shapes: at least one, in the fullest of the other shells)
    bright[:, y, x] = True
    f[bright] = rng.integers(100, 60000, int(bright.sum()))
    if np.dtype(dtype) == np.dtype(np.uint32):
        top = rng.random((B, H, W)) < 0.01
        f[top] = rng.choice(np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 7, 0xFFFFFFFF], np.int64), int(top.sum()))
    return f.astype(dtype)


def _maps(W, H, seed):
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


def _check(st, res, frames, bins, n_bins, mask=None, max_valid=-1, n_iqr=6.0, thr=0.0, min_spot_size=3):
    """Every frame's results and shell records against the oracle; -> (strong pixels of the batch, the statuses seen)."""
    total, statuses = 0, set()
    ones = np.ones(frames[0].shape, np.uint8)
    for f, img in enumerate(frames):
        strong, shells = RT.threshold(img, bins, n_bins, n_iqr, thr, mask, max_valid)
        assert_frame_matches_oracle(res[f], img, ones if mask is None else mask, min_spot_size=min_spot_size, strong=strong)
        got = st.radial_thresholds(f)
        assert got.dtype == RT.SHELL_DT and len(got) == n_bins
        for name in FIELDS:
            assert np.array_equal(got[name], shells[name]), (f, name, got[name], shells[name])
        total += int(strong.sum())
        statuses |= set(int(s) for s in shells["status"])
    return total, statuses


def _context(ffs, W, H, dtype, bins, n_bins, max_batch=3, mask=None, n_iqr=None, **params):
    ctx = ffs.Context(W, H, dtype, max_batch=max_batch)
    if mask is not None:
        ctx.set_mask(mask)
    ctx.set_radial_bins(bins, n_bins)
    if n_iqr is not None:
        ctx.set_radial_threshold(n_iqr)
    ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=1, want_strong_list=1, want_reflections=1, **params)
    return ctx


# ---- 1. shapes x pixel types x batches of 1 and 3 x maps
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_maps(ffs, shape, dtype):
    W, H = shape
    frames = _frames(dtype, 3, H, W, seed=W * 31 + H)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    st = ctx.stream()
    for name, (bins, n_bins) in _maps(W, H, seed=5).items():
        ctx.set_radial_bins(bins, n_bins)
        ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=1, want_strong_list=1, want_reflections=1)
        for B in (1, 3):
            res = st.process(frames[:B])
            path = st.last_path()[0]
            assert "radial_threshold" in path and "radial" in path, (name, path)
            total, statuses = _check(st, res, frames[:B], bins, n_bins)
            if name == "shells":
                assert total >= 1, (name, B)
                if W * H > 100:
                    assert len(statuses) >= 2, (name, statuses)
            if name == "all_none":
                assert total == 0 and statuses == {RT.EMPTY}
            # the radial profile of the same batch is what it is under any algorithm
            for f in range(B):
                for a, b in zip(st.radial_profile(f), R.radial_profile(frames[f], bins, n_bins)):
                    assert np.array_equal(a, b), (name, f)


# ---- 2. decision ties
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("n_iqr", [0.0, 2.7], ids=["n_iqr_0", "n_iqr_2.7"])
def test_decision_ties(ffs, dtype, n_iqr):
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    rng = np.random.default_rng(12)
    img = (rng.poisson(3.0, (H, W)) + 20 * (bins.astype(np.int64) % 5)).astype(dtype)
    img[bins == 7] = 9                                   # a shell of iqr 0: cutoff = median = 9
    shells = RT.shells_hist(img, bins, n_bins, n_iqr)
    assert (shells["status"] == RT.OK).all() and shells["q3"][7] == shells["q1"][7] == 9 and shells["cutoff"][7] == 9
    # two pixels of every shell planted at the cutoff and at cutoff + 1 (two among hundreds: the quartiles are checked to stay)
    planted = img.copy()
    at = {}
    for b in range(n_bins):
        ys, xs = np.nonzero(bins == b)
        assert len(ys) > 40
        c = int(shells["cutoff"][b])
        planted[ys[3], xs[3]] = c
        planted[ys[11], xs[11]] = c + 1
        at[b] = ((ys[3], xs[3]), (ys[11], xs[11]))
    after = RT.shells_hist(planted, bins, n_bins, n_iqr)
    ctx = _context(ffs, W, H, dtype, bins, n_bins, max_batch=1, n_iqr=n_iqr, min_spot_size=1)
    st = ctx.stream()
    res = st.process(planted[None])
    total, _ = _check(st, res, planted[None], bins, n_bins, n_iqr=n_iqr, min_spot_size=1)
    assert total >= 1
    for b in range(n_bins):
        if after["cutoff"][b] == shells["cutoff"][b]:
            (y0, x0), (y1, x1) = at[b]
            assert res[0].strong_mask[y0, x0] == 0 and res[0].strong_mask[y1, x1] == 1, b
    assert (after["cutoff"] == shells["cutoff"]).sum() >= n_bins // 2
    # `threshold` just below and just above a planted value: (double)p > threshold
    y1, x1 = at[7][1]
    v = int(planted[y1, x1])
    for thr, want in ((v - 0.5, 1), (float(v), 0), (v + 0.5, 0)):
        ctx.set_params(threshold=thr)
        res = st.process(planted[None])
        _check(st, res, planted[None], bins, n_bins, n_iqr=n_iqr, thr=thr, min_spot_size=1)
        assert res[0].strong_mask[y1, x1] == want, thr


# ---- 3. the counting rule
def _gappy_mask(W, H, seed):
    rng = np.random.default_rng(seed)
    m = np.ones((H, W), np.uint8)
    m[:, W // 3:W // 3 + 5] = 0
    m[H // 2:H // 2 + 3, :] = 0
    m[rng.random((H, W)) < 0.03] = 0
    return m


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_inclusion(ffs, dtype):
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    mask = _gappy_mask(W, H, 3)
    frames = _frames(dtype, 2, H, W, seed=11)
    if np.dtype(dtype) == np.dtype(np.uint32):
        frames[0, 5, 5:9] = [(1 << 24) - 1, 1 << 24, (1 << 24) - 1, 1 << 24]
        assert (frames == 1 << 24).any() and (frames == (1 << 24) - 1).any() and (frames > 1 << 24).any()
    ctx = _context(ffs, W, H, dtype, bins, n_bins, max_batch=2, mask=mask)
    st = ctx.stream()
    total, _ = _check(st, st.process(frames), frames, bins, n_bins, mask)
    assert total >= 1
    per_scope = []
    for scope in ("centre", "window"):          # max_valid under both scopes: the same results
        ctx.set_max_valid_scope(scope)
        ctx.set_params(max_valid=1000)
        res = st.process(frames)
        t, _ = _check(st, res, frames, bins, n_bins, mask, max_valid=1000)
        assert 1 <= t < total
        per_scope.append([(r.strong_k.copy(), st.radial_thresholds(f)) for f, r in enumerate(res)])
    for (ka, sa), (kb, sb) in zip(*per_scope):
        assert np.array_equal(ka, kb) and np.array_equal(sa, sb)
    ctx.set_max_valid_scope("centre")
    ctx.set_params(max_valid=-1)
    ctx.apply_resolution_mask(1.0, 0.2, 250.0, 20.0, 75e-6, 75e-6, dmin=15.0, dmax=-1.0)
    now = ctx.get_mask()
    assert 0 < now.sum() < mask.sum()
    _check(st, st.process(frames), frames, bins, n_bins, now)


# ---- 4. seams: one hot pixel at a time
def _one_hot_run(ffs, dtype, W, H, positions, tuning=None):
    bins, n_bins = _shells(W, H), 16
    ctx = _context(ffs, W, H, dtype, bins, n_bins, max_batch=8, min_spot_size=1)
    if tuning:
        ctx.set_tuning(**tuning)
    st = ctx.stream()
    for i in range(0, len(positions), 8):
        chunk = positions[i:i + 8]
        frames = np.full((len(chunk), H, W), 2, dtype)        # every shell: iqr 0, cutoff = median = 2
        for f, (x, y) in enumerate(chunk):
            frames[f, y, x] = 1000
        res = st.process(frames)
        _check(st, res, frames, bins, n_bins, min_spot_size=1)
        for f, (x, y) in enumerate(chunk):
            r = res[f]
            assert r.num_strong_pixels == 1 and list(r.strong_k) == [y * W + x], (x, y)
            assert len(r.boxes) == 1 and tuple(int(r.boxes[k][0]) for k in ("l", "t", "r", "b", "num_pixels")) == (x, y, x, y, 1), (x, y)
            assert r.strong_mask.sum() == 1 and r.strong_mask[y, x] == 1


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_seams_of_the_plane(ffs, dtype):
    W, H = 517, 41
    positions = [(x, 20) for x in range(16, 24)]                       # every bit of a plane byte
    positions += [(W - 1, 3), (127, 9), (128, 9), (300, 7), (300, 8), (5, H - 1), (W - 1, H - 1), (0, 0)]
    _one_hot_run(ffs, dtype, W, H, positions)


@pytest.mark.parametrize("bands", [1, 2, 5])
def test_seams_of_the_histogram_bands(ffs, bands):
    W, H = 517, 41
    rows = -(-H // bands)                                              # ceil(H / bands) rows a band
    edges = sorted({y for b in range(0, H, rows) for y in (b, min(b + rows, H) - 1)})
    _one_hot_run(ffs, np.uint16, W, H, [(100 + 7 * i, y) for i, y in enumerate(edges)], tuning={"radthr_bands": bands})
    # ... and real frames under the same bands, both forms of the table's adds
    bins, n_bins = _shells(W, H), 16
    frames = _frames(np.uint16, 3, H, W, seed=bands)
    for form in (0, 1, 2):
        ctx = _context(ffs, W, H, np.uint16, bins, n_bins)
        ctx.set_tuning(radthr_bands=bands, radthr_form=form)
        st = ctx.stream()
        total, _ = _check(st, st.process(frames), frames, bins, n_bins)
        assert total >= 1


# ---- 5. independence of everything that plays no part
def _resident(ctx, frames):
    import torch
    pitch, fstride = ctx.device_layout()
    B, H, W = frames.shape
    item = frames.dtype.itemsize
    host = np.full((B, fstride // item), np.iinfo(frames.dtype).max, frames.dtype)    # padding of ones: nothing reads it
    host[:, :H * (pitch // item)].reshape(B, H, pitch // item)[:, :, :W] = frames
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).to("cuda:0"), pitch, fstride


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_independence(ffs, dtype):
    from ffs_amd import bslz4
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    mask = _gappy_mask(W, H, 8)
    frames = _frames(dtype, 3, H, W, seed=21)
    if np.dtype(dtype) == np.dtype(np.uint32):
        frames = np.minimum(frames, 0x7FFFFFFF).astype(dtype)
    variants = {"default": {}, "grid_kernels": {"tuning": {"sparse_stage": 1}}, "chain_always": {"tuning": {"sparse_stage": 3}},
                "dense_mask": {"tuning": {"dense_mask": 1}}, "window_kernel_and_path_1": {"tuning": {"window_kernel": 1, "threshold_path": 1}},
                "no_mask_no_list": {"want": (0, 0)}, "mask_only": {"want": (1, 0)}, "list_only": {"want": (0, 1)},
                "gain": {"gain": 2.5}, "gain_map": {"gain_map": True}, "dispersion_settings": {"params": {"kernel_half_x": 5, "nsig_b": 1.0, "min_count": 9}}}
    for name, kw in variants.items():
        ctx = ffs.Context(W, H, dtype, max_batch=3)
        ctx.set_mask(mask)
        ctx.set_tuning(**kw.get("tuning", {}))
        if "gain" in kw:
            ctx.set_gain(kw["gain"])
        if "gain_map" in kw:
            ctx.set_gain_map(np.random.default_rng(2).uniform(0.5, 3.0, (H, W)).astype(np.float32))
        ctx.set_radial_bins(bins, n_bins)
        m, l = kw.get("want", (1, 1))
        ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=m, want_strong_list=l, want_reflections=1, **kw.get("params", {}))
        st = ctx.stream()
        total, _ = _check(st, st.process(frames), frames, bins, n_bins, mask)
        assert total >= 1 and "radial_threshold" in st.last_path()[0], name
        if name == "grid_kernels":
            assert "grid_kernels" in st.last_path()[0]
        if name == "default":       # every way in
            mem, pitch, fstride = _resident(ctx, frames)
            st.submit_device(mem.data_ptr(), pitch, fstride, 3)
            _check(st, st.wait(), frames, bins, n_bins, mask)
            _check(st, st.process_compressed([bslz4.compress(f) for f in frames[::-1]]), frames[::-1], bins, n_bins, mask)
            ms_hist, ms_rest = st.bench_threshold(mem.data_ptr(), pitch, fstride, 3, 2)
            assert 0.0 < ms_hist < 100.0 and 0.0 < ms_rest < 100.0
            _check(st, st.process(frames), frames, bins, n_bins, mask)     # the measurement left the stream usable


# ---- 6. a frame beyond max_strong_per_frame is run again on its own, by the same algorithm
def test_recovery(ffs):
    """n_iqr = 0 on noise: half of the first frame's pixels stand above their shell's median, in more runs than the one launch's run-based
    forest holds (16 384; tuning chain_runs 2 takes it for every frame) -- ffs_wait runs the batch again through the grid-wide kernels --
    and more than the lists hold, so that frame is then run on its own on a one-frame stream, which must threshold by the same map,
    n_iqr and algorithm."""
    W, H = 1030, 80
    bins, n_bins = _shells(W, H), 16
    rng = np.random.default_rng(33)
    quiet = np.full((H, W), 2)
    quiet[5, 5], quiet[40, 700] = 1000, 900
    frames = np.stack([rng.integers(0, 256, (H, W)), quiet]).astype(np.uint16)
    ctx = ffs.Context(W, H, np.uint16, max_batch=2, max_strong_per_frame=28000)
    ctx.set_tuning(chain_runs=2)
    ctx.set_radial_bins(bins, n_bins)
    ctx.set_radial_threshold(0.0)
    ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=1, want_strong_list=1, want_reflections=1, min_spot_size=1)
    st = ctx.stream()
    res = st.process(frames)
    path, reruns = st.last_path()
    assert reruns > 0 and "radial_threshold" in path, (path, reruns)
    assert res[0].num_strong_pixels > 28000 and res[1].num_strong_pixels == 2
    _check(st, res, frames, bins, n_bins, n_iqr=0.0, min_spot_size=1)


# ---- 7. one stream, alternating algorithms: plane, counts and occupancy hygiene
def test_alternating_algorithms_on_one_stream(ffs):
    from oracle import oracle as O
    W, H = 517, 41
    bins, n_bins = _shells(W, H), 16
    mask = _gappy_mask(W, H, 4)
    frames = _frames(np.uint16, 3, H, W, seed=55)
    ctx = ffs.Context(W, H, np.uint16, max_batch=3)
    ctx.set_mask(mask)
    ctx.set_radial_bins(bins, n_bins)
    st = ctx.stream()
    for i, algo in enumerate(("dispersion", "radial", "extended", "radial", "dispersion")):
        batch = frames if i % 2 == 0 else frames[::-1]
        code = {"dispersion": ffs.ALGO_DISPERSION, "radial": ffs.ALGO_RADIAL_PROFILE, "extended": ffs.ALGO_DISPERSION_EXTENDED}[algo]
        ctx.set_params(algorithm=code, want_strong_mask=1, want_strong_list=1, want_reflections=1)
        res = st.process(batch)
        if algo == "radial":
            total, _ = _check(st, res, batch, bins, n_bins, mask)
            assert total >= 1
        else:
            for fr, img in zip(res, batch):
                assert_frame_matches_oracle(fr, img, mask, strong=O.dispersion_extended(img, mask) if algo == "extended" else None)
            assert "radial_threshold" not in st.last_path()[0]
            with pytest.raises(ffs.FfsError, match="did not run the radial_profile algorithm"):
                st.radial_thresholds(0)


# ---- 8. 3D: a stack fed by add_batch from radial batches equals one fed by add_slice with the oracle's lists
def test_stack3d(ffs):
    from oracle import oracle as O
    W, H, NZ = 517, 41, 6
    bins, n_bins = _shells(W, H), 16
    frames = _frames(np.uint16, NZ, H, W, seed=71)
    frames[1:4, 10:13, 50:53] = 5000            # a spot through three frames
    ctx = _context(ffs, W, H, np.uint16, bins, n_bins, max_batch=3, min_spot_size_3d=1)
    st = ctx.stream()
    a, b = ffs.Stack3D(ctx), ffs.Stack3D(ctx)
    for z0 in range(0, NZ, 3):
        st.process(frames[z0:z0 + 3], first_frame_id=z0)
        a.add_batch(st)
    slices = []
    for z, img in enumerate(frames):
        strong, _ = RT.threshold(img, bins, n_bins)
        cc = O.cc2d(strong, img, 3)
        slices.append((cc.k.astype(np.uint32), cc.intensity))
        b.add_slice(z, *slices[-1])
    ra, rb = a.finish(), b.finish()
    assert ra[1:] == rb[1:] and len(ra[0]) >= 1
    assert_reflections_equal(ra[0], rb[0])
    want = O.cc3d(slices, W, H, 1, 2.0)
    assert_reflections_equal(ra[0], want.reflections)
    assert any(r["z_max"] - r["z_min"] >= 2 for r in ra[0])


# ---- 9. refusals, each with its text and the state as it was
def test_refusals(ffs):
    W, H = 37, 29
    bins, n_bins = _shells(W, H), 16
    frames = _frames(np.uint16, 1, H, W, seed=4)
    wide = np.random.default_rng(1).integers(0, 129, (H, W)).astype(np.uint16)
    ctx = ffs.Context(W, H, np.uint16)
    st = ctx.stream()
    with pytest.raises(ffs.FfsError, match="needs a radial bin map"):
        ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE)
    ctx.params.algorithm = ffs.ALGO_DISPERSION
    ctx.set_radial_bins(wide, 129)
    with pytest.raises(ffs.FfsError, match="at most 128 bins"):
        ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE)
    ctx.params.algorithm = ffs.ALGO_DISPERSION
    st.process(frames)                                  # the context still runs the dispersion algorithm
    assert "radial_threshold" not in st.last_path()[0]
    with pytest.raises(ffs.FfsError, match="did not run the radial_profile algorithm"):
        st.radial_thresholds(0)
    ctx.set_radial_bins(bins, n_bins)
    ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE, want_strong_mask=1, want_strong_list=1, want_reflections=1)

    def still_as_it_was(n_iqr=6.0):
        _check(st, st.process(frames), frames, bins, n_bins, n_iqr=n_iqr)

    with pytest.raises(ffs.FfsError, match="which needs the map"):
        ctx.set_radial_bins(None)
    still_as_it_was()
    with pytest.raises(ffs.FfsError, match="takes at most 128 bins, got 129"):
        ctx.set_radial_bins(wide, 129)
    still_as_it_was()
    ctx.set_radial_threshold(2.5)
    for bad in (-1.0, float("nan"), float("inf"), float(1 << 21)):
        with pytest.raises(ffs.FfsError, match="n_iqr must be finite and in 0 .. 2\\^20"):
            ctx.set_radial_threshold(bad)
        still_as_it_was(2.5)
    ctx.set_radial_threshold(float(1 << 20))            # the largest n_iqr is accepted
    still_as_it_was(float(1 << 20))
    with pytest.raises(ffs.FfsError, match="out of range"):
        st.radial_thresholds(1)
    # n_iqr is kept across set_params, and under another algorithm the map may go
    ctx.set_radial_threshold(2.5)
    ctx.set_params(threshold=1.0)
    _check(st, st.process(frames), frames, bins, n_bins, n_iqr=2.5, thr=1.0)
    ctx.set_params(algorithm=ffs.ALGO_DISPERSION)
    ctx.set_radial_bins(None)
    st.process(frames)
    with pytest.raises(ffs.FfsError, match="did not run the radial_profile algorithm"):
        st.radial_thresholds(0)


# ---- 10. the driver
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
    common = ["synth:tiny:%d" % N, "--threads", "1", "--batch", "2", "--single-buffer", "--max-valid", "none"]
    rc, out, err, lines = _run(common + ["-a", "Radial_Profile", "--radial-bins", str(SHELLS), "--n-iqr", "4"], tmp_path)
    assert rc == 0 and not err, (out, err)
    assert "Algorithm: Radial Profile" in out
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    ctx = ffs.Context(300, 200, np.uint16, max_batch=2)
    ctx.set_radial_bins(bins, SHELLS)
    ctx.set_radial_threshold(N_IQR)
    ctx.set_params(algorithm=ffs.ALGO_RADIAL_PROFILE)
    st = ctx.stream()
    for z0 in range(0, N, 2):
        res = st.process(frames[z0:z0 + 2])
        for j, r in enumerate(res):
            g, shells = got[z0 + j], st.radial_thresholds(j)
            assert g["num_strong_pixels"] == r.num_strong_pixels > 0 and g["n_spots_total"] == r.n_spots_total
            assert g["radial_median"] == [int(v) for v in shells["median"]]
            assert g["radial_cutoff"] == [int(v) for v in shells["cutoff"]]
            assert g["radial_status"] == [int(v) for v in shells["status"]]
            assert list(g) == sorted(g)                  # keys in alphabetical order, as before
            want = RT.shells_hist(frames[z0 + j], bins, SHELLS, N_IQR)
            assert np.array_equal(shells["cutoff"], want["cutoff"])
    for extra, message in ((["-a", "radial_profile", "--validate"], "--validate is not available with the radial_profile algorithm"),
                           (["-a", "radial_profile", "--radial-bins", "129"], "at most 128 shells")):
        r = subprocess.run([SPOTFINDER, *common, *extra], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0 and message in r.stdout and "Usage: spotfinder" in r.stdout, r.stdout
