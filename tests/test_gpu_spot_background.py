"""GPU: the per-spot background (ffs_stream_spot_backgrounds), held bit for bit to tests/spot_background_oracle.py.

Every comparison is array_equal on the eight integer fields and on the bit pattern of the float64 mean; the boxes are the reflections the
library returned for the batch.  The shapes are where the kernel can go wrong: (37, 29) has a pitch that is not its width, (517, 41)
crosses a 512-pixel row, (8, 8) is smaller than a border of 16 on every side."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import spot_background_cases as cases
import spot_background_oracle as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
SHAPES = [(37, 29), (517, 41), (8, 8)]


def _check(st, res, frames, mask, max_valid, border):
    """The stream's backgrounds for the batch wait() just returned as `res`, against the oracle on the library's own boxes."""
    got = st.spot_backgrounds(border)
    want = B.batch_backgrounds(frames, mask, max_valid, [r.reflections for r in res], border)
    assert got.dtype == B.DT and len(got) == len(want) == sum(len(r.reflections) for r in res)
    for name in B.INTEGER_FIELDS:
        assert np.array_equal(got[name], want[name]), (name, border, got[name], want[name])
    assert np.array_equal(got["mean"].view(np.uint64), want["mean"].view(np.uint64))
    assert not got["reserved"].any()
    return got


def _raw_rings(frames, res, border):
    """Every ring's pixels of the batch with no validity rule applied, concatenated."""
    parts = [B.ring_values(f.astype(np.uint64), None, -1, (r["x_min"], r["x_max"], r["y_min"], r["y_max"]), border) for f, fr in zip(frames, res) for r in fr.reflections]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint64)


def _batch(dtype, W, H, seed):
    """Three frames with different numbers of spots, the middle one with none; 32-bit: pixels at 2^24 - 1 and at 2^24 sprinkled over them."""
    from util import make_frame
    rng = np.random.default_rng(seed)
    if W * H < 100:
        a = np.full((H, W), 2, dtype)
        a[2:5, 3:6] = 500
        c = rng.poisson(3.0, (H, W)).astype(dtype)
        c[0:2, 0:2] = 700
        c[5:8, 4:8] = 900
    else:
        a = make_frame(W, H, dtype, seed=seed, n_spots=max(W * H // 60, 6))[0]
        c = make_frame(W, H, dtype, seed=seed + 1, n_spots=5)[0]
    frames = np.stack([a, np.full((H, W), 2, dtype), c])
    if np.dtype(dtype).itemsize == 4:
        for f in (frames[0], frames[2]):
            f[rng.random((H, W)) < 0.03] = (1 << 24) - 1
            f[rng.random((H, W)) < 0.03] = 1 << 24
    return frames


def _mask(W, H, seed):
    from util import make_frame
    return make_frame(W, H, np.uint16, seed=seed, masked=True)[1]


# ---- 1. shapes x pixel types x batches of 1 and 3 x borders x masks
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_batches_borders_masks(ffs, shape, dtype):
    W, H = shape
    frames = _batch(dtype, W, H, seed=W + H)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    seen_sizes = set()
    for mask in (None, _mask(W, H, 3)):
        ctx.set_mask(mask)
        for nb in (1, 3):
            res = st.process(frames[:nb])
            counts = [len(r.reflections) for r in res]
            if nb == 3 and mask is None:
                assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0, counts
                assert (counts[0] != counts[2] and sum(counts) > 4) or W * H < 100     # slices of different lengths; more reflections than a workgroup has waves
            for border in (1, 3, 16):
                got = _check(st, res, frames[:nb], mask, -1, border)
                seen_sizes.update(int(v) for v in got["n_pixels"])
            if np.dtype(dtype).itemsize == 4 and nb == 3 and W * H >= 100:
                raw = _raw_rings(frames, res, 3)
                assert (raw == (1 << 24) - 1).any() and (raw == 1 << 24).any()
    assert len(seen_sizes) > 3, seen_sizes


# ---- 2. max_valid below some ring pixels, under both scopes
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_max_valid_leaves_ring_pixels_out(ffs, dtype):
    from util import make_frame
    W, H = 517, 41
    rng = np.random.default_rng(12)
    frames = np.stack([make_frame(W, H, dtype, seed=s, n_spots=60, peak=(30.0, 600.0))[0] for s in (5, 6)])
    frames[rng.random(frames.shape) < 0.04] = 5000
    mask = _mask(W, H, 9)
    ctx = ffs.Context(W, H, dtype, max_batch=2)
    ctx.set_mask(mask)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    res = st.process(frames)
    open_bg = _check(st, res, frames, mask, -1, 3)
    for scope in ("centre", "window"):
        ctx.set_max_valid_scope(scope)
        ctx.set_params(max_valid=1000)
        res = st.process(frames)
        assert sum(len(r.reflections) for r in res) > 4
        assert (_raw_rings(frames, res, 3) > 1000).any()
        _check(st, res, frames, mask, 1000, 3)
    assert open_bg["n_overflow"].any()


# ---- 3. the planted frames
def test_planted_frames(ffs):
    ctx = ffs.Context(cases.W, cases.H, np.uint16)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    seen = set()
    for name, c in cases.cases().items():
        ctx.set_mask(c["mask"])
        res = st.process(c["frame"][None])
        r = res[0].reflections
        boxes = [(int(a), int(b), int(cc), int(d)) for a, b, cc, d in zip(r["x_min"], r["x_max"], r["y_min"], r["y_max"])]
        assert c["box"] in boxes, (name, boxes)
        if c.get("only"):
            assert boxes == [c["box"]], (name, boxes)
        got = _check(st, res, c["frame"][None], c["mask"], -1, 3)
        at = boxes.index(c["box"])
        assert int(got["status"][at]) == c["status"], (name, got[at])
        if "record" in c:
            assert {k: int(got[k][at]) for k in c["record"]} == c["record"], (name, got[at])
            assert got["mean"][at] == (c["record"]["inlier_sum"] / c["record"]["n_inliers"] if c["status"] == 0 else 0.0)
        if "box2" in c:      # each block's strong pixels sit in the other's ring and are fenced out
            at2 = boxes.index(c["box2"])
            assert int(got["status"][at2]) == 0 and got["mean"][at] < 10 and got["mean"][at2] < 10
            assert got["n_inliers"][at] < got["n_pixels"][at] and got["n_inliers"][at2] < got["n_pixels"][at2]
        seen.update(int(s) for s in got["status"])
    assert {0, 1, 2, 3} <= seen, seen


# ---- 4. every way in gives the same arrays
def _resident_padded(ctx, frames):
    """The frames in the context's pitched device layout, the row padding and the tail of every frame filled with ones."""
    import torch
    pitch, fstride = ctx.device_layout()
    n, H, W = frames.shape
    item = frames.dtype.itemsize
    host = np.full((n, fstride // item), np.iinfo(frames.dtype).max, frames.dtype)
    rows = host[:, :H * (pitch // item)].reshape(n, H, pitch // item)
    rows[:, :, :W] = frames
    assert pitch // item > W
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).to("cuda:0"), pitch, fstride


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_every_way_in(ffs, dtype):
    from ffs_amd import bslz4
    W, H = 517, 41
    frames = _batch(dtype, W, H, seed=31)
    mask = _mask(W, H, 4)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    ctx.set_mask(mask)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    res = st.process(frames)
    first = _check(st, res, frames, mask, -1, 3)
    assert len(first) > 4
    mem, pitch, fstride = _resident_padded(ctx, frames)
    st.submit_device(mem.data_ptr(), pitch, fstride, 3)
    res = st.wait()
    assert np.array_equal(_check(st, res, frames, mask, -1, 3), first)
    res = st.process_compressed([bslz4.compress(f) for f in frames])
    assert np.array_equal(_check(st, res, frames, mask, -1, 3), first)


# ---- 5. the tunings that change a batch's path change nothing here
def test_tunings_give_identical_arrays(ffs):
    W, H = 517, 41
    frames = _batch(np.uint16, W, H, seed=41)
    mask = _mask(W, H, 6)

    def run(**tuning):
        ctx = ffs.Context(W, H, np.uint16, max_batch=3)
        ctx.set_mask(mask)
        ctx.set_tuning(**tuning)
        ctx.set_params(want_reflections=1)
        st = ctx.stream()
        res = st.process(frames)
        return _check(st, res, frames, mask, -1, 3), st.last_path()[0]

    default, _ = run()
    assert len(default) > 4
    for tuning in ({"sparse_stage": 1}, {"sparse_stage": 3}, {"threshold_path": 2}):
        got, path = run(**tuning)
        assert np.array_equal(got, default), tuning
        if tuning.get("sparse_stage") == 1:
            assert "grid_kernels" in path


# ---- 6. a batch that ffs_wait ran again: the call sees its final records
def test_after_a_rerun(ffs):
    rng = np.random.default_rng(9)
    W, H = 1000, 300
    base = rng.poisson(2.0, (H, W)).astype(np.uint16)
    for x, y in ((50, 40), (700, 20), (990, 290)):
        base[y:y + 3, x:x + 3] = 500
    fat = base.copy()
    fat[100:130, 200:240] = 3000          # a block whose rim is strong: a band beyond the band plan, a frame beyond the 100 pixels the lists hold
    frames = np.stack([base, fat])
    ctx = ffs.Context(W, H, np.uint16, max_batch=2, max_strong_per_frame=100)
    ctx.set_params(min_spot_size=1, want_reflections=1, max_peak_centroid_separation=100.0)   # (the rim, a ring 40 x 30, stays a reflection)
    st = ctx.stream()
    res = st.process(frames)
    assert st.last_path()[1] >= 1 and res[1].num_strong_pixels > 100
    assert len(res[0].reflections) >= 3 and len(res[1].reflections) >= 4
    assert (res[1].reflections["x_max"] - res[1].reflections["x_min"]).max() == 39
    _check(st, res, frames, None, -1, 3)


# ---- 7. refusals
def test_refusals(ffs):
    W, H = 37, 29
    frames = _batch(np.uint16, W, H, seed=2)
    ctx = ffs.Context(W, H, np.uint16, max_batch=3)
    st = ctx.stream()
    with pytest.raises(ffs.FfsError, match="no batch has been waited for"):
        st.spot_backgrounds(3)
    ctx.set_params(want_reflections=0)
    res = st.process(frames)                               # a batch without want_reflections
    with pytest.raises(ffs.FfsError, match="without want_reflections"):
        st.spot_backgrounds(3)
    ctx.set_params(want_reflections=1)
    st.submit(frames)
    with pytest.raises(ffs.FfsError, match="in flight"):
        st.spot_backgrounds(3)
    res = st.wait()
    for bad in (0, 17, 1 << 20):
        with pytest.raises(ffs.FfsError, match=r"border must be in 1\.\.16"):
            st.spot_backgrounds(bad)
    _check(st, res, frames, None, -1, 3)                   # and the stream is as good as before
    quiet = st.process(np.full((1, H, W), 2, np.uint16))   # a batch with no reflections: an empty array, nothing launched
    got, ms = st.spot_backgrounds(3, want_ms=True)
    assert len(quiet[0].reflections) == 0 and len(got) == 0 and got.dtype == B.DT and ms == 0.0


# ---- 8. sequencing
def test_sequencing_and_teardown(ffs):
    W, H = 37, 29
    fa, fb = _batch(np.uint16, W, H, seed=7), _batch(np.uint16, W, H, seed=8)[::-1]
    ctx = ffs.Context(W, H, np.uint16, max_batch=3)
    ctx.set_params(want_reflections=1)
    st, other = ctx.stream(), ctx.stream()
    res = st.process(fa)
    one = _check(st, res, fa, None, -1, 1)
    three, ms = st.spot_backgrounds(3, want_ms=True)
    assert ms > 0.0 and not np.array_equal(one["n_pixels"], three["n_pixels"])
    assert np.array_equal(_check(st, res, fa, None, -1, 1), one)     # each call its own result, in any order
    view = st.spot_backgrounds(3, copy=False)
    assert np.array_equal(view, three)
    other.submit(fb)                                                  # another stream's batch in flight does not matter
    assert np.array_equal(st.spot_backgrounds(3), three)
    res_other = other.wait()
    _check(other, res_other, fb, None, -1, 3)
    st.submit(fb)
    res = st.wait()
    _check(st, res, fb, None, -1, 3)                                  # follows the new batch
    st.close()
    other.close()
    ctx.close()
    # destroyed in the other order, right after a call
    ctx = ffs.Context(W, H, np.uint16, max_batch=3)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    res = st.process(fa)
    _check(st, res, fa, None, -1, 16)
    ctx.close()
    st.close()


# ---- 9. the driver
def _run(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", out), err, lines


def test_driver_spot_background(ffs, tmp_path):
    from ffs_amd import synth
    N = 4       # (two batches of two images)
    rc, out, err, lines = _run(["synth:tiny:%d" % N, "--threads", "1", "--batch", "2", "--single-buffer", "--max-valid", "none", "--spot-background", "3"], tmp_path)
    assert rc == 0 and not err, (out, err)
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    ctx = ffs.Context(300, 200, np.uint16, max_batch=2)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    n_valid = 0
    for first in (0, 2):
        res = st.process(frames[first:first + 2], first)
        bg = _check(st, res, frames[first:first + 2], None, -1, 3)
        intensity, variance = ffs.spot_intensities(st.last_batch_reflections, bg)
        at = 0
        for k, fr in enumerate(res):
            line = got[first + k]
            n = len(fr.reflections)
            assert n > 0 and list(line) == sorted(line)          # keys in alphabetical order
            ok = bg["status"][at:at + n] == 0
            want_mean = [float(m) if o else None for m, o in zip(bg["mean"][at:at + n], ok)]
            want_int = [float(v) if o else None for v, o in zip(intensity[at:at + n], ok)]
            want_var = [float(v) if o else None for v, o in zip(variance[at:at + n], ok)]
            assert line["spot_background_mean"] == want_mean
            assert line["spot_intensity"] == want_int
            assert line["spot_variance"] == want_var
            assert line["total_intensity"] == sum(v for v in want_int if v is not None)
            n_valid += int(ok.sum())
            at += n
    assert n_valid > 10
