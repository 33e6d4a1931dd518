"""GPU: the detector gain (ffs_ctx_set_gain; DIALS spotfinder.threshold.dispersion.gain).  Every comparison is exact equality --
all pixels, boxes and reflections -- with tests/gain_oracle.py, the NumPy float64 restatement of the reference's gain arithmetic
that tests/test_gain_oracle.py ties to the committed oracle; at gain 1.0 and by powers of two also with the committed oracle itself.
The standard algorithm through the general-window kernel and through the gather of threshold_path 2, the extended algorithm
(flavour 0) with its debug planes, the per-batch snapshot through re-runs and encoded submits, and the driver's --gain."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gain_oracle as G
import tie_windows as T
import window_ties as WT
from oracle import oracle as O
from util import assert_frame_matches_oracle, make_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
WINDOWS = [(3, 3), (2, 5), (7, 1)]
GAINS = [7.0, 2.5, 0.3]


def _disp(kx, ky, min_count=2):
    return O.DispParams(kx, ky, min_count, 0.0, 6.0, 3.0)


def _ctx(ffs, W, H, dtype, gain, kx=3, ky=3, max_batch=1, tuning=None, mask=None, max_strong_per_frame=0, **kw):
    ctx = ffs.Context(W, H, dtype, max_batch=max_batch, max_strong_per_frame=max_strong_per_frame)
    if tuning:
        ctx.set_tuning(**tuning)
    kw.setdefault("want_strong_mask", 1)
    kw.setdefault("want_strong_list", 1)
    ctx.set_params(want_reflections=1, kernel_half_x=kx, kernel_half_y=ky, **kw)
    if gain is not None:
        ctx.set_gain(gain)
    if mask is not None:
        ctx.set_mask(mask)
    return ctx


# the shared frames: computed once, read-only (530 x 97 crosses k_window's 496-px strip edge and its two row bands)
_ADU = {}


def _adu_frame(dtype, gain, masked=True, seed=1):
    key = (np.dtype(dtype).name, gain, masked, seed)
    if key not in _ADU:
        photons, mask = G.photon_frame(seed, masked=masked)
        img = G.adu(photons, gain, dtype)
        img.setflags(write=False)
        mask.setflags(write=False)
        _ADU[key] = (img, mask)
    return _ADU[key]


# ---- 1. the standard algorithm on frames in ADU
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("kx,ky", WINDOWS, ids=["3x3", "2x5", "7x1"])
def test_adu_frames(ffs, kx, ky, gain, dtype):
    for masked in (True, False):
        img, mask = _adu_frame(dtype, gain, masked)
        H, W = img.shape
        want = G.dispersion_gain(img, mask, gain, kx, ky)
        assert want.sum() > 0 and not np.array_equal(want, O.dispersion(img, mask, _disp(kx, ky)))   # (the gain matters on this frame)
        ctx = _ctx(ffs, W, H, dtype, gain, kx, ky, mask=mask)
        st = ctx.stream()
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
        assert "window" in st.last_path()[0]


# ---- 2. ties: gain 1.0 against the compiled oracle
@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5), (5, 5)], ids=["3x3", "2x5", "5x5"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_tie_cells_at_gain_1(ffs, kx, ky, dtype):
    prm = T.Params(min_count=(2 * kx + 1) * (2 * ky + 1) // 2)
    img, mask, cells = WT.frame(kx, ky, dtype, prm)
    H, W = img.shape
    want = O.dispersion(img, mask, _disp(kx, ky, prm.min_count))
    for c in cells:
        assert bool(want[c.row, c.col]) == c.exact
    for tuning in ({}, {"sparse_stage": 1}):
        ctx = _ctx(ffs, W, H, dtype, 1.0, kx, ky, tuning=tuning, mask=mask, min_count=prm.min_count)
        st = ctx.stream()
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
        assert "window" in st.last_path()[0]


# ---- 3. bound to the committed oracle: frame x 4 at gain 4 is the frame at gain 1, exactly (tests/test_gain_oracle.py)
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", WINDOWS, ids=["3x3", "2x5", "7x1"])
def test_frame_times_4_at_gain_4_is_the_committed_oracle(ffs, kx, ky, dtype):
    for seed in (1, 2):
        photons, mask = G.photon_frame(seed)
        want = O.dispersion(photons.astype(dtype), mask, _disp(kx, ky))
        img = (photons * 4).astype(dtype)
        assert want.sum() > 100
        ctx = _ctx(ffs, img.shape[1], img.shape[0], dtype, 4.0, kx, ky, mask=mask)
        assert_frame_matches_oracle(ctx.stream().process(img[None])[0], img, mask, strong=want)


# ---- 4. the cross-check path of `spotfinder --validate`
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5)], ids=["3x3", "2x5"])
def test_threshold_path_2(ffs, kx, ky, dtype):
    img, mask = _adu_frame(dtype, 2.5)
    H, W = img.shape
    want = G.dispersion_gain(img, mask, 2.5, kx, ky)
    assert want.sum() > 0 and not np.array_equal(want, O.dispersion(img, mask, _disp(kx, ky)))
    ctx = _ctx(ffs, W, H, dtype, 2.5, kx, ky, tuning={"threshold_path": 2}, mask=mask)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" not in st.last_path()[0]


# ---- 5. the default is untouched; the gain is a per-batch snapshot, kept across set_params
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_gain_0_is_the_default_path(ffs, dtype):
    img, mask = _adu_frame(dtype, 2.5)
    H, W = img.shape
    want = O.dispersion(img, mask)
    never = _ctx(ffs, W, H, dtype, None, mask=mask)
    st = never.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" not in st.last_path()[0]
    back = _ctx(ffs, W, H, dtype, 3.0, mask=mask)
    st = back.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=G.dispersion_gain(img, mask, 3.0))
    assert "window" in st.last_path()[0]
    back.set_gain(0)
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" not in st.last_path()[0]


def test_gain_survives_set_params_and_is_taken_at_submit(ffs):
    img, mask = _adu_frame(np.uint16, 2.5)
    H, W = img.shape
    frames = np.stack([img, np.ascontiguousarray(img[::-1])])
    masks = np.ones((H, W), np.uint8)
    ctx = _ctx(ffs, W, H, np.uint16, 2.5, max_batch=2)
    a, b, c = ctx.stream(), ctx.stream(), ctx.stream()
    a.submit(frames)
    ctx.set_gain(0)
    b.submit(frames)
    ctx.set_gain(7.0)
    ctx.set_params(min_spot_size=3)   # the gain is kept across ffs_ctx_set_params
    c.submit(frames)
    ctx.set_gain(0)
    for fr, f in zip(a.wait(), frames):
        assert_frame_matches_oracle(fr, f, masks, strong=G.dispersion_gain(f, masks, 2.5))
    for fr, f in zip(b.wait(), frames):
        assert_frame_matches_oracle(fr, f, masks, strong=O.dispersion(f, masks))
    for fr, f in zip(c.wait(), frames):
        assert_frame_matches_oracle(fr, f, masks, strong=G.dispersion_gain(f, masks, 7.0))
    assert "window" in a.last_path()[0] and "window" not in b.last_path()[0] and "window" in c.last_path()[0]


# ---- 6. with the window scope of max_valid
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5)], ids=["3x3", "2x5"])
def test_with_max_valid_window_scope(ffs, kx, ky, dtype):
    img, mask = _adu_frame(dtype, 2.5)
    H, W = img.shape
    over, max_valid = (65535, 60000) if dtype == np.uint16 else ((1 << 24) - 1, 1_000_000)
    img = img.copy()
    ys, xs = np.nonzero(G.dispersion_gain(img, mask, 2.5, kx, ky))
    pick = np.random.default_rng(5).choice(len(ys), 12, replace=False)
    img[ys[pick], np.minimum(xs[pick] + 2, W - 1)] = over   # overloads two columns to the right of strong pixels
    mask2 = (mask & (img <= max_valid)).astype(np.uint8)
    want = G.dispersion_gain(img, mask2, 2.5, kx, ky)
    centre = G.dispersion_gain(img, mask, 2.5, kx, ky, max_valid=max_valid)
    assert want.sum() > 0 and not np.array_equal(want, centre)
    assert not np.array_equal(want, O.dispersion(img, mask2, _disp(kx, ky)))
    ctx = _ctx(ffs, W, H, dtype, 2.5, kx, ky, mask=mask, max_valid=max_valid)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=centre)   # the centre scope first
    ctx.set_max_valid_scope("window")
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" in st.last_path()[0]


# ---- 7. the extended algorithm, flavour 0
_EXT = {}


def _ext_case(dtype, gain):
    key = (np.dtype(dtype).name, gain)
    if key not in _EXT:
        photons, mask = G.blob_photons(5)
        img = G.adu(photons.astype(np.int64), gain, dtype)
        want = G.dispersion_extended_gain(img, mask, gain)
        _EXT[key] = (img, mask, want)
    return _EXT[key]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("tuning", [{}, {"ext_first_pass": 0}, {"ext_erode": 0}, {"ext_fused": 1}], ids=["default", "first0", "erode0", "fused"])
def test_extended_flavour_0(ffs, dtype, tuning):
    img, mask, (strong, first, eroded) = _ext_case(dtype, 2.5)
    H, W = img.shape
    assert eroded.sum() > 100 and strong.sum() > 100
    assert not np.array_equal(strong, O.dispersion_extended(img, mask))   # (the gain matters here)
    ctx = _ctx(ffs, W, H, dtype, 2.5, tuning=tuning, mask=mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED)
    st = ctx.stream()
    fr = st.process(img[None])[0]
    d = np.argwhere(st.debug_bitplane(0, 1) != first)
    assert d.size == 0, f"first pass: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"
    d = np.argwhere(st.debug_bitplane(0, 2) != eroded)
    assert d.size == 0, f"erosion: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"
    assert_frame_matches_oracle(fr, img, mask, strong=strong)
    assert "extended" in st.last_path()[0]
    # gain 0 again on the same stream: what the committed oracle says
    ctx.set_gain(0)
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=O.dispersion_extended(img, mask))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_extended_530x97_and_gain_1(ffs, dtype):
    """The base shape (k_ext_first's 56-px strips, its 64-row band) with max_valid set; and gain 1.0 against the committed oracle."""
    rng = np.random.default_rng(3)
    W, H = 530, 97
    from util import _blob_frame
    photons = _blob_frame(W, H, 8, 12).astype(np.int64)
    mask = (rng.random((H, W)) > 0.01).astype(np.uint8)
    for gain, max_valid in ((2.5, 9000), (1.0, 3500)):
        img = G.adu(photons, gain, dtype)
        strong, first, eroded = G.dispersion_extended_gain(img, mask, gain, max_valid=max_valid)
        assert eroded.sum() > 50 and strong.sum() > 0
        if gain == 1.0:
            for g, w in zip((strong, first, eroded), O.dispersion_extended(img, mask, None, 0, float(max_valid), debug=True)):
                assert np.array_equal(g, w)
        ctx = _ctx(ffs, W, H, dtype, gain, mask=mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED, max_valid=max_valid)
        st = ctx.stream()
        fr = st.process(img[None])[0]
        assert np.array_equal(st.debug_bitplane(0, 1), first) and np.array_equal(st.debug_bitplane(0, 2), eroded)
        assert_frame_matches_oracle(fr, img, mask, strong=strong)


@pytest.mark.parametrize("scope", ["centre", "window"])
def test_extended_u32_pixels_at_and_above_2_24(ffs, scope):
    """32-bit pixels at 2^24 - 1, 2^24 and above it, as neighbours and as centres: under the centre scope the GAIN kernels' neighbour
    limit is 2^24, the oracle's own rule (standalone.cc:78,90); under the window scope max_valid lies above it and changes nothing
    but the centre guard.  At gain 1.0 the restatement is held to the committed oracle on the same kind of frame."""
    photons, mask = G.blob_photons(7)
    rng = np.random.default_rng(11)
    big = rng.random(photons.shape) < 0.01
    max_valid = -1 if scope == "centre" else (1 << 24) + 3
    for gain in (2.5, 1.0):
        img = G.adu(photons.astype(np.int64), gain, np.uint32)
        # (gain 1.0 without 2^24 - 1: windows that hold it have m*y and x*x beyond 2^53, where the gain form's a = m*y - x*x and the
        # photon form's m*y - x*x - x*(m - 1) round differently, and the compiled oracle's float64 table is no longer exact either)
        img[big] = rng.choice([(1 << 24) - 1, 1 << 24, (1 << 24) + 7] if gain != 1.0 else [1 << 24, (1 << 24) + 7], size=big.sum())
        mask_f = mask if scope == "centre" else (mask & (img <= max_valid)).astype(np.uint8)   # (the window scope: masked for the frame)
        strong, first, eroded = G.dispersion_extended_gain(img, mask_f, gain, max_valid=max_valid)
        assert eroded.sum() > 100 and strong.sum() > 100 and (strong & (img >= (1 << 24))).sum() > 0   # (centres at or above 2^24 among them)
        if gain == 1.0:
            for g, w in zip((strong, first, eroded), O.dispersion_extended(img, mask_f, None, 0, float(max_valid), debug=True)):
                assert np.array_equal(g, w)
        ctx = _ctx(ffs, img.shape[1], img.shape[0], np.uint32, gain, mask=mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED, max_valid=max_valid)
        ctx.set_max_valid_scope(scope)
        st = ctx.stream()
        fr = st.process(img[None])[0]
        assert np.array_equal(st.debug_bitplane(0, 1), first) and np.array_equal(st.debug_bitplane(0, 2), eroded)
        assert_frame_matches_oracle(fr, img, mask, strong=strong)


# ---- 8. refusals leave the state as it was
def test_refusals(ffs):
    img, mask = _adu_frame(np.uint16, 2.5)
    H, W = img.shape
    ctx = _ctx(ffs, W, H, np.uint16, 2.5, mask=mask)
    st = ctx.stream()
    for bad in (-1.0, -0.0001, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ffs.FfsError, match="ffs_ctx_set_gain"):
            ctx.set_gain(bad)
    want = G.dispersion_gain(img, mask, 2.5)
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)   # still 2.5
    # a gain and the device flavour of the extended algorithm, whichever call comes second
    with pytest.raises(ffs.FfsError, match="gain"):
        ctx.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=1)
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)   # still the standard algorithm at 2.5
    ctx.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=0)      # flavour 0 is fine
    photons, bmask = G.blob_photons(2, 64, 64, masked=False)
    ctx2 = ffs.Context(64, 64, np.uint16)
    ctx2.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=1, want_strong_mask=1)
    with pytest.raises(ffs.FfsError, match="extended_flavour 1"):
        ctx2.set_gain(2.5)
    ctx2.set_gain(0)   # off is always accepted
    # (still flavour 1 without a gain: the refused call changed nothing)
    assert_frame_matches_oracle(ctx2.stream().process(photons[None])[0], photons, bmask, strong=O.dispersion_extended(photons, bmask, None, 1))


# ---- 9. clipping: frames narrower or shorter than the window, the kernel's strip edge
@pytest.mark.parametrize("W,H", [(1, 1), (9, 5), (62 * 8 + 1, 4), (1, 40)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_clipping(ffs, W, H, dtype):
    rng = np.random.default_rng(W * 1000 + H)
    photons = rng.poisson(2.0, size=(H, W)).astype(np.int64)
    hot = rng.random((H, W)) < 0.05
    photons[hot] = rng.integers(50, 3000, size=hot.sum())
    img = G.adu(photons, 2.5, dtype)
    img[rng.random((H, W)) < 0.01] = 65535 if dtype == np.uint16 else (1 << 24) + 5
    mask = (rng.random((H, W)) > 0.1).astype(np.uint8)
    ctx = _ctx(ffs, W, H, dtype, 2.5, mask=mask)
    st = ctx.stream()
    for kx, ky in ((3, 3), (5, 5)):
        ctx.set_params(kernel_half_x=kx, kernel_half_y=ky)
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=G.dispersion_gain(img, mask, 2.5, kx, ky))
        assert "window" in st.last_path()[0]


# ---- 10. outputs on and off, batches of three frames on three streams in flight
@pytest.mark.parametrize("want_mask,want_list", [(0, 0), (0, 1), (1, 0)])
def test_three_streams_in_flight(ffs, want_mask, want_list):
    W, H, B = 700, 130, 3
    frames = np.stack([G.adu(G.photon_frame(40 + i, W, H)[0], 2.5, np.uint16) for i in range(3 * B)])
    mask = make_frame(W, H, np.uint16, seed=40, masked=True)[1]
    ctx = _ctx(ffs, W, H, np.uint16, 2.5, max_batch=B, mask=mask, want_strong_mask=want_mask, want_strong_list=want_list)
    streams = [ctx.stream() for _ in range(3)]
    for i, st in enumerate(streams):
        st.submit(frames[i * B:(i + 1) * B], first_frame_id=i * B)
    for i, st in enumerate(streams):
        res = st.wait()
        for fr, img in zip(res, frames[i * B:(i + 1) * B]):
            assert_frame_matches_oracle(fr, img, mask, strong=G.dispersion_gain(img, mask, 2.5))
        assert (res[0].strong_mask is not None) == bool(want_mask)
        assert (res[0].strong_k is not None) == bool(want_list)
        assert "window" in st.last_path()[0]


# ---- 11. the re-runs inside ffs_wait keep the batch's gain
def test_overflow_rerun_keeps_the_gain(ffs):
    """A frame with more strong pixels than the stream's lists is run again inside ffs_wait, on a one-frame stream: under the gain
    its batch was submitted with, whatever the context says by then."""
    W, H = 300, 200
    photons = T.dense_frame((H, W), np.uint16).astype(np.int64) // 2   # Poisson(300) with 1 % of the pixels near 20300, halved
    sel = np.random.default_rng(8).random((H, W)) < 0.02
    photons[sel] += 40                                                   # weak peaks: strong only for who takes ADU for photons
    img = G.adu(photons, 2.5, np.uint16)
    mask = np.ones((H, W), np.uint8)
    want = G.dispersion_gain(img, mask, 2.5)
    assert want.sum() > 500 and not np.array_equal(want, O.dispersion(img, mask))
    other = G.adu(G.photon_frame(3, W, H)[0], 2.5, np.uint16)
    frames = np.stack([img, other])
    ctx = _ctx(ffs, W, H, np.uint16, 2.5, max_batch=2, max_strong_per_frame=500)
    st = ctx.stream()
    st.submit(frames)
    ctx.set_gain(0)   # the context moves on; the batch in flight and its re-run keep the gain
    res = st.wait()
    assert_frame_matches_oracle(res[0], img, mask, strong=want)
    assert_frame_matches_oracle(res[1], other, mask, strong=G.dispersion_gain(other, mask, 2.5))
    # The stream's lists hold 500 entries: a complete list of more (held to the oracle entry by entry above) can only have come from
    # the frame's re-run on the one-frame stream, which rerun_overflow_frames enqueues with the batch's own snapshot.
    assert res[0].num_strong_pixels == int(want.sum()) > 500 and len(res[0].strong_k) == int(want.sum())


def test_batch_rerun_keeps_the_gain(ffs):
    """A frame of isolated strong pixels with more runs than the run-based one-launch sparse stage holds (tuning chain_runs = 2)
    raises its flag: ffs_wait runs the WHOLE batch again (`reruns` > 0), threshold stage included -- under the batch's gain."""
    rng = np.random.default_rng(4)
    W, H = 640, 480
    photons = rng.poisson(1.0, (H, W)).astype(np.int64)
    photons[rng.random((H, W)) < 0.09] += 60                      # ~27 k isolated strong pixels
    img = G.adu(photons, 2.5, np.uint16)
    mask = np.ones((H, W), np.uint8)
    want = G.dispersion_gain(img, mask, 2.5)
    assert want.sum() > 20000 and not np.array_equal(want, O.dispersion(img, mask))
    ctx = _ctx(ffs, W, H, np.uint16, 2.5, max_strong_per_frame=60000, tuning={"chain_runs": 2}, want_strong_mask=0, min_spot_size=1)
    st = ctx.stream()
    st.submit(img[None])
    ctx.set_gain(0)
    res = st.wait()
    path, reruns = st.last_path()
    assert_frame_matches_oracle(res[0], img, mask, min_spot_size=1, strong=want)
    assert reruns > 0 and "window" in path, (path, reruns)


# ---- 12. an encoded submit enqueues from a helper thread, with the snapshot taken at the submit call
def test_encoded_submit_keeps_the_gain(ffs):
    from ffs_amd import bslz4
    img, mask = _adu_frame(np.uint16, 2.5)
    H, W = img.shape
    frames = [np.ascontiguousarray(img), np.ascontiguousarray(img[::-1])]
    ctx = _ctx(ffs, W, H, np.uint16, 2.5, max_batch=2, mask=mask)
    st = ctx.stream()
    st.submit_compressed([bslz4.compress(f) for f in frames])
    ctx.set_gain(0)
    res = st.wait()
    for fr, f in zip(res, frames):
        assert_frame_matches_oracle(fr, f, mask, strong=G.dispersion_gain(f, mask, 2.5))
    assert "window" in st.last_path()[0]


# ---- 13. the driver
def _run(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", out), err, lines


@pytest.mark.parametrize("algo", ["dispersion", "dispersion_extended"])
def test_driver_gain(ffs, tmp_path, algo):
    from ffs_amd import synth
    N = 4
    rc, out, err, lines = _run(["synth:tiny:%d" % N, "--threads", "2", "--batch", "2", "--gain", "2.5", "-a", algo, "--max-valid", "none",
                                "--validate"], tmp_path)
    assert rc == 0 and not err, (out, err)
    assert "Detector gain: 2.5" in out
    matches = re.findall(r"Image\s+(\d+): Compared: Match (\d+) px", out)
    assert sorted(int(a) for a, _ in matches) == list(range(N)) and "Mismatch" not in out
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    mask = np.ones((200, 300), np.uint8)
    differs = False
    for i, img in enumerate(frames):
        if algo == "dispersion":
            want, plain = G.dispersion_gain(img, mask, 2.5), O.dispersion(img, mask)
        else:
            want, plain = G.dispersion_extended_gain(img, mask, 2.5)[0], O.dispersion_extended(img, mask)
        cc = O.cc2d(want, img, 3)
        assert got[i]["num_strong_pixels"] == cc.num_strong_pixels == int(want.sum())
        assert got[i]["n_spots_total"] == len(cc.boxes)
        differs |= not np.array_equal(want, plain)
    assert differs
