"""GPU: the robust Poisson GLM background (ffs_stream_spot_backgrounds_glm), held bit for bit to `ffs_hosttool spotbgglm` -- the same
header (csrc/spot_background_glm_model.hpp) compiled for the CPU -- on the histograms of the rings that tests/spot_background_oracle.py
extracts for the library's own boxes.  Every comparison is array_equal on the integer fields and on the bit patterns of beta and mean.
The shapes are those of tests/test_gpu_spot_background.py: (37, 29) has a pitch that is not its width, (517, 41) crosses a 512-pixel row,
(8, 8) is smaller than a border of 16 on every side."""
import os
import subprocess

import numpy as np
import pytest

import spot_background_cases as tukey_cases
import spot_background_glm_cases as K
import spot_background_glm_oracle as G
import spot_background_oracle as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTTOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
SHAPES = [(37, 29), (517, 41), (8, 8)]


def host_records(rings):
    """The rings' records from the header on the CPU, as G.DT."""
    out = np.zeros(len(rings), G.DT)
    if not rings:
        return out
    r = subprocess.run([HOSTTOOL, "spotbgglm"], input=K.histogram_text(rings), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(rings)
    for i, line in enumerate(lines):
        t = line.split()
        for name, v in zip(G.INTEGER_FIELDS, t[:5]):
            out[name][i] = int(v)
        out["beta"].view(np.uint64)[i] = int(t[5], 16)
        out["mean"].view(np.uint64)[i] = int(t[6], 16)
    return out


def _rings(frames, mask, max_valid, res, border):
    return [B.ring_values(f, mask, max_valid, (r["x_min"], r["x_max"], r["y_min"], r["y_max"]), border) for f, fr in zip(frames, res) for r in fr.reflections]


def _same(got, want):
    assert got.dtype == G.DT and len(got) == len(want)
    for name in G.INTEGER_FIELDS:
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])
    for name in ("beta", "mean"):
        a, b = got[name].view(np.uint64), want[name].view(np.uint64)
        assert np.array_equal(a, b), (name, got[name][a != b], want[name][a != b], got["n_iter"][a != b])
    assert not got["reserved"].any()


def _check(st, res, frames, mask, max_valid, border):
    """The stream's GLM backgrounds for the batch wait() just returned as `res`, against the header on the CPU for the library's own boxes."""
    got = st.spot_backgrounds_glm(border)
    assert len(got) == sum(len(r.reflections) for r in res)
    _same(got, host_records(_rings(frames, mask, max_valid, res, border)))
    assert (got["mean"][got["status"] != 0] == 0.0).all() and (got["median"][np.isin(got["status"], (1, 2, 5))] == -1).all()
    return got


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


# ---- 1. shapes x pixel types x batches of 1 and 3 (an empty middle frame) x borders x masks; more reflections than a workgroup has waves
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_batches_borders_masks(ffs, shape, dtype):
    W, H = shape
    frames = _batch(dtype, W, H, seed=W + H)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    statuses, sizes = set(), set()
    for mask in (None, _mask(W, H, 3)):
        ctx.set_mask(mask)
        for nb in (1, 3):
            res = st.process(frames[:nb])
            counts = [len(r.reflections) for r in res]
            if nb == 3 and mask is None:
                assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0, counts
                assert sum(counts) > 4 or W * H < 100
            for border in (1, 3, 16):
                got = _check(st, res, frames[:nb], mask, -1, border)
                statuses.update(int(s) for s in got["status"])
                sizes.update(int(v) for v in got["n_pixels"])
            if np.dtype(dtype).itemsize == 4 and nb == 3 and W * H >= 100:
                raw = np.concatenate(_rings(frames.astype(np.uint64), None, -1, res, 3))
                assert (raw == (1 << 24) - 1).any() and (raw == 1 << 24).any()
    assert 0 in statuses and len(sizes) > 3, (statuses, sizes)


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
        assert (np.concatenate(_rings(frames.astype(np.uint64), None, -1, res, 3)) > 1000).any()
        _check(st, res, frames, mask, 1000, 3)
    assert open_bg["n_overflow"].any()


# ---- 3. the planted frames: each situation on the device
def _boxes(res):
    r = res[0].reflections
    return [(int(a), int(b), int(cc), int(d)) for a, b, cc, d in zip(r["x_min"], r["x_max"], r["y_min"], r["y_max"])]


def test_planted_frames(ffs):
    seen = {}
    for name, c in K.planted_frames().items():
        Hf, Wf = c["frame"].shape
        ctx = ffs.Context(Wf, Hf, np.uint16)
        ctx.set_params(want_reflections=1)
        ctx.set_mask(c["mask"])
        st = ctx.stream()
        res = st.process(c["frame"][None])
        boxes = _boxes(res)
        assert c["box"] in boxes, (name, boxes)
        got = _check(st, res, c["frame"][None], c["mask"], -1, c["border"])
        rec = got[boxes.index(c["box"])]
        assert int(rec["status"]) == c["status"] and int(rec["n_pixels"]) == c["n_pixels"], (name, rec)
        if "n_iter" in c:
            assert int(rec["n_iter"]) == c["n_iter"], (name, rec)
        if "n_iter_at_least" in c:
            assert int(rec["n_iter"]) >= c["n_iter_at_least"], (name, rec)
        if "mean" in c:
            assert rec["mean"] == c["mean"], (name, rec)
        seen[name] = rec
        st.close()
        ctx.close()
    assert seen["all_zero_ring"]["beta"] == -np.inf
    assert 150.0 < seen["poisson_200"]["mean"] < 250.0 and 0.0 < seen["poisson_0_05"]["mean"] < 0.3
    assert seen["ring_of_9"]["median"] == -1 and seen["ring_of_10"]["mean"] > 0.0


def test_overflow_boundary_and_the_tukey_frames(ffs):
    """The planted frames of the Tukey model: 18 of 72 ring pixels in the tail is still fitted (4 * 18 = 72), 19 is refused; a ring with no
    valid pixel is status 1; and the rings whose fence reaches the end of the histogram (Tukey's status 3) get a GLM estimate."""
    ctx = ffs.Context(tukey_cases.W, tukey_cases.H, np.uint16)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    by_name = {}
    for name, c in tukey_cases.cases().items():
        ctx.set_mask(c["mask"])
        res = st.process(c["frame"][None])
        boxes = _boxes(res)
        assert c["box"] in boxes, (name, boxes)
        got = _check(st, res, c["frame"][None], c["mask"], -1, 3)
        tukey = st.spot_backgrounds(3)
        at = boxes.index(c["box"])
        assert int(tukey["status"][at]) == c["status"]
        by_name[name] = got[at]
    assert (int(by_name["tie_18_of_72"]["status"]), int(by_name["tie_18_of_72"]["n_overflow"])) == (0, 18) and by_name["tie_18_of_72"]["mean"] > 2.0
    assert (int(by_name["tie_19_of_72"]["status"]), int(by_name["tie_19_of_72"]["n_overflow"])) == (2, 19)
    assert int(by_name["island_in_the_mask"]["status"]) == 1 and int(by_name["above_the_bins"]["status"]) == 2
    assert int(by_name["two_levels"]["status"]) == 0 and by_name["two_levels"]["mean"] > 0.0      # (Tukey: status 3)


# ---- 4. both models on one batch: each its own buffer, neither disturbs the other
def test_both_models_on_one_batch(ffs):
    W, H = 517, 41
    frames = _batch(np.uint16, W, H, seed=31)
    ctx = ffs.Context(W, H, np.uint16, max_batch=3)
    ctx.set_params(want_reflections=1)
    st = ctx.stream()
    res = st.process(frames)
    want_tukey = B.batch_backgrounds(frames, None, -1, [r.reflections for r in res], 3)
    want_glm = host_records(_rings(frames, None, -1, res, 3))
    assert len(want_glm) > 4
    tukey_view = st.spot_backgrounds(3, copy=False)
    tukey_first = tukey_view.copy()
    glm_view, ms = st.spot_backgrounds_glm(3, copy=False, want_ms=True)
    assert ms > 0.0
    _same(glm_view, want_glm)
    assert np.array_equal(tukey_view, tukey_first)                   # the Tukey pointer is still valid after the GLM call, its records unchanged
    for name in B.INTEGER_FIELDS:
        assert np.array_equal(tukey_view[name], want_tukey[name]), name
    again = st.spot_backgrounds(3, copy=False)                       # and the GLM pointer after another Tukey call
    assert np.array_equal(again, tukey_first)
    _same(glm_view, want_glm)
    assert np.array_equal(st.spot_backgrounds_glm(1)["n_pixels"], st.spot_backgrounds(1)["n_pixels"])
    assert np.array_equal(st.spot_backgrounds_glm(3), glm_view)
    intensity, variance = ffs.spot_intensities_glm(st.last_batch_reflections, glm_view)
    ok = glm_view["status"] == 0
    assert ok.any() and np.isfinite(intensity[ok]).all() and (variance[ok] > 0).all() and np.isnan(intensity[~ok]).all()


# ---- 5. the refusals of the shared preconditions name this entry point
def test_refusals(ffs):
    W, H = 37, 29
    frames = _batch(np.uint16, W, H, seed=2)
    ctx = ffs.Context(W, H, np.uint16, max_batch=3)
    st = ctx.stream()
    with pytest.raises(ffs.FfsError, match="ffs_stream_spot_backgrounds_glm: no batch has been waited for"):
        st.spot_backgrounds_glm(3)
    ctx.set_params(want_reflections=0)
    st.process(frames)                                     # a batch without want_reflections
    with pytest.raises(ffs.FfsError, match="ffs_stream_spot_backgrounds_glm: the last batch was submitted without want_reflections"):
        st.spot_backgrounds_glm(3)
    ctx.set_params(want_reflections=1)
    st.submit(frames)
    with pytest.raises(ffs.FfsError, match="ffs_stream_spot_backgrounds_glm: a batch is in flight"):
        st.spot_backgrounds_glm(3)
    res = st.wait()
    for bad in (0, 17, 1 << 20):
        with pytest.raises(ffs.FfsError, match=r"ffs_stream_spot_backgrounds_glm: border must be in 1\.\.16"):
            st.spot_backgrounds_glm(bad)
    with pytest.raises(ffs.FfsError, match=r"ffs_stream_spot_backgrounds: border must be in 1\.\.16"):
        st.spot_backgrounds(0)                             # (and the Tukey entry still names itself)
    _check(st, res, frames, None, -1, 3)                   # the stream is as good as before
    quiet = st.process(np.full((1, H, W), 2, np.uint16))   # a batch with no reflections: an empty array, nothing launched
    got, ms = st.spot_backgrounds_glm(3, want_ms=True)
    assert len(quiet[0].reflections) == 0 and len(got) == 0 and got.dtype == G.DT and ms == 0.0
    ctx.close()                                            # destroyed right after a call, context first
    st.close()
