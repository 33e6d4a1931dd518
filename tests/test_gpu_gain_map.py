"""GPU: the per-pixel gain map (ffs_ctx_set_gain_map; DIALS spotfinder.lookup.gain_map).  Every comparison is exact equality -- all
pixels, boxes and reflections -- with tests/gain_map_oracle.py, the NumPy float64 restatement of the reference's gain arithmetic with
the gain array read at the window's centre, which tests/test_gain_map_oracle.py ties to tests/gain_oracle.py and a pixel loop.  The
standard algorithm through the general-window kernel and through the gather of threshold_path 2, the extended algorithm (flavour 0)
with its debug planes, batches in flight, the re-runs inside ffs_wait, an encoded submit, the map as a property of the context with
its refusals, and the driver's --gain-map.  Section by section after tests/test_gpu_gain.py."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gain_map_oracle as M
import gain_oracle as G
import tie_windows as T
import window_ties as WT
from oracle import oracle as O
from util import assert_frame_matches_oracle, make_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
WINDOWS = [(3, 3), (2, 5), (7, 1)]


def _disp(kx, ky, min_count=2):
    return O.DispParams(kx, ky, min_count, 0.0, 6.0, 3.0)


def _ctx(ffs, W, H, dtype, gain_map, kx=3, ky=3, max_batch=1, tuning=None, mask=None, max_strong_per_frame=0, **kw):
    ctx = ffs.Context(W, H, dtype, max_batch=max_batch, max_strong_per_frame=max_strong_per_frame)
    if tuning:
        ctx.set_tuning(**tuning)
    kw.setdefault("want_strong_mask", 1)
    kw.setdefault("want_strong_list", 1)
    ctx.set_params(want_reflections=1, kernel_half_x=kx, kernel_half_y=ky, **kw)
    if gain_map is not None:
        ctx.set_gain_map(gain_map)
    if mask is not None:
        ctx.set_mask(mask)
    return ctx


# the shared maps and frames: computed once, read-only (530 x 97 crosses k_window's 496-px strip edge and its two row bands; the module
# map's boundary at x = 500 sits 4 px from that edge)
_MAPS, _FRAMES = {}, {}


def _map(name, W=530, H=97):
    key = (name, W, H)
    if key not in _MAPS:
        g = M.module_map(W, H) if name == "module" else M.random_map(1, W, H) if name == "random" else M.random_map(2, W, H)
        g.setflags(write=False)
        _MAPS[key] = g
    return _MAPS[key]


def _frame(dtype, name, masked=True, seed=1):
    """The photon frame of the gain tests as a detector with this map delivers it."""
    key = (np.dtype(dtype).name, name, masked, seed)
    if key not in _FRAMES:
        photons, mask = G.photon_frame(seed, masked=masked)
        img = M.adu_under_map(photons, _map(name), dtype)
        img.setflags(write=False)
        mask.setflags(write=False)
        _FRAMES[key] = (img, mask)
    return _FRAMES[key]


# ---- 1. the standard algorithm
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("name", ["module", "random"])
@pytest.mark.parametrize("kx,ky", WINDOWS, ids=["3x3", "2x5", "7x1"])
def test_adu_frames(ffs, kx, ky, name, dtype):
    gmap = _map(name)
    for masked in (True, False):
        img, mask = _frame(dtype, name, masked)
        H, W = img.shape
        want = M.dispersion_gain_map(img, mask, gmap, kx, ky)
        scalar = G.dispersion_gain(img, mask, float(gmap.mean(dtype=np.float64)), kx, ky)
        assert want.sum() > 0 and not np.array_equal(want, scalar)   # (the map matters on this frame)
        ctx = _ctx(ffs, W, H, dtype, gmap, kx, ky, mask=mask)
        st = ctx.stream()
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
        assert "window" in st.last_path()[0]


# ---- 2. a constant map is the scalar gain, bit for bit
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", WINDOWS, ids=["3x3", "2x5", "7x1"])
def test_constant_map_against_the_scalar(ffs, kx, ky, dtype):
    photons, mask = G.photon_frame(1)
    img = G.adu(photons, 2.5, dtype)
    H, W = img.shape
    want = G.dispersion_gain(img, mask, 2.5, kx, ky)
    assert want.sum() > 100
    by_map = _ctx(ffs, W, H, dtype, np.full((H, W), 2.5, np.float32), kx, ky, mask=mask)
    scalar = _ctx(ffs, W, H, dtype, None, kx, ky, mask=mask)
    scalar.set_gain(2.5)
    a, b = by_map.stream().process(img[None])[0], scalar.stream().process(img[None])[0]
    assert_frame_matches_oracle(a, img, mask, strong=want)
    assert_frame_matches_oracle(b, img, mask, strong=want)
    assert np.array_equal(a.strong_mask, b.strong_mask) and np.array_equal(a.strong_k, b.strong_k)


# ---- 3. ties: an all-ones map against the compiled oracle
@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5), (5, 5)], ids=["3x3", "2x5", "5x5"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_tie_cells_under_an_all_ones_map(ffs, kx, ky, dtype):
    prm = T.Params(min_count=(2 * kx + 1) * (2 * ky + 1) // 2)
    img, mask, cells = WT.frame(kx, ky, dtype, prm)
    H, W = img.shape
    want = O.dispersion(img, mask, _disp(kx, ky, prm.min_count))
    for c in cells:
        assert bool(want[c.row, c.col]) == c.exact
    ctx = _ctx(ffs, W, H, dtype, np.ones((H, W), np.float32), kx, ky, mask=mask, min_count=prm.min_count)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" in st.last_path()[0]


# ---- 4. the cross-check path of `spotfinder --validate`
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5)], ids=["3x3", "2x5"])
def test_threshold_path_2(ffs, kx, ky, dtype):
    gmap = _map("module")
    img, mask = _frame(dtype, "module")
    H, W = img.shape
    want = M.dispersion_gain_map(img, mask, gmap, kx, ky)
    assert want.sum() > 0
    ctx = _ctx(ffs, W, H, dtype, gmap, kx, ky, tuning={"threshold_path": 2}, mask=mask)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" not in st.last_path()[0]


# ---- 5. the extended algorithm, flavour 0
_EXT = {}


def _ext_case(dtype):
    key = np.dtype(dtype).name
    if key not in _EXT:
        photons, mask = G.blob_photons(5)
        gmap = _map("module", 300, 200)
        img = M.adu_under_map(photons.astype(np.int64), gmap, dtype)
        _EXT[key] = (img, mask, gmap, M.dispersion_extended_gain_map(img, mask, gmap))
    return _EXT[key]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("tuning", [{}, {"ext_first_pass": 0}, {"ext_erode": 0}, {"ext_fused": 1}], ids=["default", "first0", "erode0", "fused"])
def test_extended_flavour_0(ffs, dtype, tuning):
    img, mask, gmap, (strong, first, eroded) = _ext_case(dtype)
    H, W = img.shape
    assert eroded.sum() > 100 and strong.sum() > 100
    scalar = G.dispersion_extended_gain(img, mask, float(gmap.mean(dtype=np.float64)))
    assert not np.array_equal(strong, scalar[0]) and not np.array_equal(first, scalar[1])   # (the map matters here, in both passes)
    ctx = _ctx(ffs, W, H, dtype, gmap, tuning=tuning, mask=mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED)
    st = ctx.stream()
    fr = st.process(img[None])[0]
    d = np.argwhere(st.debug_bitplane(0, 1) != first)
    assert d.size == 0, f"first pass: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"
    d = np.argwhere(st.debug_bitplane(0, 2) != eroded)
    assert d.size == 0, f"erosion: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"
    assert_frame_matches_oracle(fr, img, mask, strong=strong)
    assert "extended" in st.last_path()[0]
    # no map again on the same stream: what the committed oracle says
    ctx.set_gain_map(None)
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=O.dispersion_extended(img, mask))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_extended_530x97_with_max_valid(ffs, dtype):
    """The base shape (k_ext_first's 56-px strips, its 64-row band) with max_valid set."""
    rng = np.random.default_rng(3)
    W, H = 530, 97
    from util import _blob_frame
    photons = _blob_frame(W, H, 8, 12).astype(np.int64)
    mask = (rng.random((H, W)) > 0.01).astype(np.uint8)
    for name, max_valid in (("module", 9000),):
        gmap = _map(name)
        img = M.adu_under_map(photons, gmap, dtype)
        strong, first, eroded = M.dispersion_extended_gain_map(img, mask, gmap, max_valid=max_valid)
        assert eroded.sum() > 50 and strong.sum() > 0
        assert not np.array_equal(strong, M.dispersion_extended_gain_map(img, mask, gmap)[0])   # (max_valid matters)
        ctx = _ctx(ffs, W, H, dtype, gmap, mask=mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED, max_valid=max_valid)
        st = ctx.stream()
        fr = st.process(img[None])[0]
        assert np.array_equal(st.debug_bitplane(0, 1), first) and np.array_equal(st.debug_bitplane(0, 2), eroded)
        assert_frame_matches_oracle(fr, img, mask, strong=strong)


@pytest.mark.parametrize("scope", ["centre", "window"])
def test_extended_u32_pixels_at_and_above_2_24(ffs, scope):
    """32-bit pixels at 2^24 - 1, 2^24 and above it, as neighbours and as centres, as in the scalar gain's test of this name."""
    photons, mask = G.blob_photons(7)
    rng = np.random.default_rng(11)
    big = rng.random(photons.shape) < 0.01
    max_valid = -1 if scope == "centre" else (1 << 24) + 3
    gmap = _map("module", 300, 200)
    img = M.adu_under_map(photons.astype(np.int64), gmap, np.uint32)
    img[big] = rng.choice([(1 << 24) - 1, 1 << 24, (1 << 24) + 7], size=big.sum())
    mask_f = mask if scope == "centre" else (mask & (img <= max_valid)).astype(np.uint8)   # (the window scope: masked for the frame)
    strong, first, eroded = M.dispersion_extended_gain_map(img, mask_f, gmap, max_valid=max_valid)
    assert eroded.sum() > 100 and strong.sum() > 100 and (strong & (img >= (1 << 24))).sum() > 0   # (centres at or above 2^24 among them)
    ctx = _ctx(ffs, img.shape[1], img.shape[0], np.uint32, gmap, mask=mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED, max_valid=max_valid)
    ctx.set_max_valid_scope(scope)
    st = ctx.stream()
    fr = st.process(img[None])[0]
    assert np.array_equal(st.debug_bitplane(0, 1), first) and np.array_equal(st.debug_bitplane(0, 2), eroded)
    assert_frame_matches_oracle(fr, img, mask, strong=strong)


# ---- 6. with the window scope of max_valid
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5)], ids=["3x3", "2x5"])
def test_with_max_valid_window_scope(ffs, kx, ky, dtype):
    gmap = _map("module")
    img, mask = _frame(dtype, "module")
    H, W = img.shape
    over, max_valid = (65535, 60000) if dtype == np.uint16 else ((1 << 24) - 1, 1_000_000)
    img = img.copy()
    ys, xs = np.nonzero(M.dispersion_gain_map(img, mask, gmap, kx, ky))
    pick = np.random.default_rng(5).choice(len(ys), 12, replace=False)
    img[ys[pick], np.minimum(xs[pick] + 2, W - 1)] = over   # overloads two columns to the right of strong pixels
    mask2 = (mask & (img <= max_valid)).astype(np.uint8)
    want = M.dispersion_gain_map(img, mask2, gmap, kx, ky)
    centre = M.dispersion_gain_map(img, mask, gmap, kx, ky, max_valid=max_valid)
    assert want.sum() > 0 and not np.array_equal(want, centre)
    ctx = _ctx(ffs, W, H, dtype, gmap, kx, ky, mask=mask, max_valid=max_valid)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=centre)   # the centre scope first
    ctx.set_max_valid_scope("window")
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" in st.last_path()[0]


# ---- 7. clipping: frames narrower or shorter than the window, the kernel's strip edge
@pytest.mark.parametrize("W,H", [(1, 1), (9, 5), (62 * 8 + 1, 4), (1, 40)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_clipping(ffs, W, H, dtype):
    rng = np.random.default_rng(W * 1000 + H)
    photons = rng.poisson(2.0, size=(H, W)).astype(np.int64)
    hot = rng.random((H, W)) < 0.05
    photons[hot] = rng.integers(50, 3000, size=hot.sum())
    gmap = M.random_map(W + H, W, H)
    img = M.adu_under_map(photons, gmap, dtype)
    img[rng.random((H, W)) < 0.01] = 65535 if dtype == np.uint16 else (1 << 24) + 5
    mask = (rng.random((H, W)) > 0.1).astype(np.uint8)
    ctx = _ctx(ffs, W, H, dtype, gmap, mask=mask)
    st = ctx.stream()
    for kx, ky in ((3, 3), (5, 5)):
        ctx.set_params(kernel_half_x=kx, kernel_half_y=ky)
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=M.dispersion_gain_map(img, mask, gmap, kx, ky))
        assert "window" in st.last_path()[0]


# ---- 8. outputs on and off, batches of three frames on three streams in flight
@pytest.mark.parametrize("want_mask,want_list", [(0, 0), (0, 1), (1, 0)])
def test_three_streams_in_flight(ffs, want_mask, want_list):
    W, H, B = 700, 130, 3
    gmap = _map("module", W, H)
    frames = np.stack([M.adu_under_map(G.photon_frame(40 + i, W, H)[0], gmap, np.uint16) for i in range(3 * B)])
    mask = make_frame(W, H, np.uint16, seed=40, masked=True)[1]
    ctx = _ctx(ffs, W, H, np.uint16, gmap, max_batch=B, mask=mask, want_strong_mask=want_mask, want_strong_list=want_list)
    streams = [ctx.stream() for _ in range(3)]
    for i, st in enumerate(streams):
        st.submit(frames[i * B:(i + 1) * B], first_frame_id=i * B)
    for i, st in enumerate(streams):
        res = st.wait()
        for fr, img in zip(res, frames[i * B:(i + 1) * B]):
            assert_frame_matches_oracle(fr, img, mask, strong=M.dispersion_gain_map(img, mask, gmap))
        assert (res[0].strong_mask is not None) == bool(want_mask)
        assert (res[0].strong_k is not None) == bool(want_list)
        assert "window" in st.last_path()[0]


# ---- 9. the re-runs inside ffs_wait compute with the map
def test_overflow_rerun_keeps_the_map(ffs):
    """A frame with more strong pixels than the stream's lists is run again inside ffs_wait, on a one-frame stream of the same
    context: under the map."""
    W, H = 300, 200
    gmap = _map("module", W, H)
    photons = T.dense_frame((H, W), np.uint16).astype(np.int64) // 8   # Poisson(300) with 1 % of the pixels near 20300, an eighth of it
    sel = np.random.default_rng(8).random((H, W)) < 0.02
    photons[sel] += 40
    img = M.adu_under_map(photons, gmap, np.uint16)
    mask = np.ones((H, W), np.uint8)
    want = M.dispersion_gain_map(img, mask, gmap)
    assert want.sum() > 500 and not np.array_equal(want, G.dispersion_gain(img, mask, float(gmap.mean(dtype=np.float64))))
    other = M.adu_under_map(G.photon_frame(3, W, H)[0], gmap, np.uint16)
    frames = np.stack([img, other])
    ctx = _ctx(ffs, W, H, np.uint16, gmap, max_batch=2, max_strong_per_frame=500)
    st = ctx.stream()
    st.submit(frames)
    res = st.wait()
    assert_frame_matches_oracle(res[0], img, mask, strong=want)
    assert_frame_matches_oracle(res[1], other, mask, strong=M.dispersion_gain_map(other, mask, gmap))
    # The stream's lists hold 500 entries: a complete list of more (held to the oracle entry by entry above) can only have come from
    # the frame's re-run on the one-frame stream.
    assert res[0].num_strong_pixels == int(want.sum()) > 500 and len(res[0].strong_k) == int(want.sum())


def test_batch_rerun_keeps_the_map(ffs):
    """A frame of isolated strong pixels with more runs than the run-based one-launch sparse stage holds (tuning chain_runs = 2)
    raises its flag: ffs_wait runs the WHOLE batch again (`reruns` > 0), threshold stage included -- under the map, even when the
    caller has dropped it in between (NULL frees nothing a batch could still read)."""
    rng = np.random.default_rng(4)
    W, H = 640, 480
    gmap = _map("module", W, H)
    photons = rng.poisson(1.0, (H, W)).astype(np.int64)
    photons[rng.random((H, W)) < 0.09] += 60                      # ~27 k isolated strong pixels
    img = M.adu_under_map(photons, gmap, np.uint16)
    mask = np.ones((H, W), np.uint8)
    want = M.dispersion_gain_map(img, mask, gmap)
    assert want.sum() > 20000 and not np.array_equal(want, G.dispersion_gain(img, mask, float(gmap.mean(dtype=np.float64))))
    ctx = _ctx(ffs, W, H, np.uint16, gmap, max_strong_per_frame=60000, tuning={"chain_runs": 2}, want_strong_mask=0, min_spot_size=1)
    st = ctx.stream()
    st.submit(img[None])
    ctx.set_gain_map(None)
    res = st.wait()
    path, reruns = st.last_path()
    assert_frame_matches_oracle(res[0], img, mask, min_spot_size=1, strong=want)
    assert reruns > 0 and "window" in path, (path, reruns)


# ---- 10. an encoded submit enqueues from a helper thread
def test_encoded_submit(ffs):
    from ffs_amd import bslz4
    gmap = _map("module")
    img, mask = _frame(np.uint16, "module")
    H, W = img.shape
    frames = [np.ascontiguousarray(img), np.ascontiguousarray(img[::-1])]
    ctx = _ctx(ffs, W, H, np.uint16, gmap, max_batch=2, mask=mask)
    st = ctx.stream()
    st.submit_compressed([bslz4.compress(f) for f in frames])
    res = st.wait()
    for fr, f in zip(res, frames):
        assert_frame_matches_oracle(fr, f, mask, strong=M.dispersion_gain_map(f, mask, gmap))
    assert "window" in st.last_path()[0]


# ---- 11. the map is a property of the context
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_state(ffs, dtype):
    gmap, second = _map("module"), _map("random2")
    img, mask = _frame(dtype, "module")
    H, W = img.shape
    ctx = _ctx(ffs, W, H, dtype, gmap, mask=mask)
    st = ctx.stream()
    want = M.dispersion_gain_map(img, mask, gmap)
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    ctx.set_params(min_spot_size=3)                  # kept across ffs_ctx_set_params
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" in st.last_path()[0]
    want2 = M.dispersion_gain_map(img, mask, second)
    assert not np.array_equal(want, want2)
    ctx.set_gain_map(second)                         # a second, different map takes effect for the next batch
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want2)
    ctx.set_gain_map(None)                           # back on the default path, with the committed oracle's results
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=O.dispersion(img, mask))
    assert "window" not in st.last_path()[0]
    ctx.set_gain_map(gmap)                           # ... and the first map again, into the buffer of the first set
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)


# ---- 12. refusals leave the state as it was
def test_refusals(ffs):
    gmap = _map("module")
    img, mask = _frame(np.uint16, "module")
    H, W = img.shape
    ctx = _ctx(ffs, W, H, np.uint16, gmap, mask=mask)
    st = ctx.stream()
    want = M.dispersion_gain_map(img, mask, gmap)

    def still_the_map():
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
        assert "window" in st.last_path()[0]

    for bad in (0.0, -2.5, float("nan"), float("inf"), 2.0 ** -61, 2.0 ** 61):
        g = np.array(_map("random"))
        g[5, 7] = bad
        with pytest.raises(ffs.FfsError, match=rf"ffs_ctx_set_gain_map: entry {5 * W + 7} "):
            ctx.set_gain_map(g)
        still_the_map()
    for edge in (2.0 ** -60, 2.0 ** 60):                   # the ends of the range are inside it
        other = ffs.Context(16, 8, np.uint16)
        other.set_gain_map(np.full((8, 16), edge, np.float32))
    # the scalar while a map is set ...
    with pytest.raises(ffs.FfsError, match="ffs_ctx_set_gain: a gain map is set"):
        ctx.set_gain(2.5)
    ctx.set_gain(0)                                        # (off is always accepted)
    still_the_map()
    # ... and a map while gain 2.5 is set
    sc = _ctx(ffs, W, H, np.uint16, None, mask=mask)
    sc.set_gain(2.5)
    with pytest.raises(ffs.FfsError, match="ffs_ctx_set_gain_map: a scalar gain is set"):
        sc.set_gain_map(gmap)
    sc.set_gain_map(None)                                  # (no map is always accepted)
    sst = sc.stream()
    assert_frame_matches_oracle(sst.process(img[None])[0], img, mask, strong=G.dispersion_gain(img, mask, 2.5))
    # a map and the device flavour of the extended algorithm, whichever call comes second
    with pytest.raises(ffs.FfsError, match="gain map"):
        ctx.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=1)
    ctx.params.algorithm, ctx.params.extended_flavour = ffs.ALGO_DISPERSION, 0   # (the binding's copy; the context never took them)
    still_the_map()
    photons, bmask = G.blob_photons(2, 64, 64, masked=False)
    ctx2 = ffs.Context(64, 64, np.uint16)
    ctx2.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=1, want_strong_mask=1)
    with pytest.raises(ffs.FfsError, match="extended_flavour 1"):
        ctx2.set_gain_map(np.full((64, 64), 2.5, np.float32))
    ctx2.set_gain_map(None)
    # (still flavour 1 without a gain: the refused call changed nothing)
    assert_frame_matches_oracle(ctx2.stream().process(photons[None])[0], photons, bmask, strong=O.dispersion_extended(photons, bmask, None, 1))
    # a wrong array shape is refused in the binding
    for shape in ((W, H), (H, W - 1), (H * W,), (1, H, W)):
        with pytest.raises(ValueError, match="gain map must have shape"):
            ctx.set_gain_map(np.ones(shape, np.float32))
    still_the_map()
    # while a batch is in flight: refused; the batch is the old map's
    st.submit(img[None])
    with pytest.raises(ffs.FfsError, match="in flight"):
        ctx.set_gain_map(_map("random"))
    assert_frame_matches_oracle(st.wait()[0], img, mask, strong=want)
    still_the_map()
    ctx.set_gain_map(_map("random"))                       # (accepted once nothing is in flight)
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=M.dispersion_gain_map(img, mask, _map("random")))


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
def test_driver_gain_map(ffs, tmp_path, algo):
    from ffs_amd import synth
    N = 4
    gmap = np.empty((200, 300), np.float32)   # two vertical stripes
    gmap[:, :150], gmap[:, 150:] = 4.0, 0.5
    gmap.astype("<f4").tofile(tmp_path / "gain.f32")
    common = ["synth:tiny:%d" % N, "--threads", "2", "--batch", "2", "-a", algo, "--max-valid", "none", "--validate"]
    rc, out, err, lines = _run(common + ["--gain-map", str(tmp_path / "gain.f32")], tmp_path)
    assert rc == 0 and not err, (out, err)
    assert re.search(r"Detector gain map: \S*gain\.f32 \(0\.5 \.\. 4\)", out), out
    matches = re.findall(r"Image\s+(\d+): Compared: Match (\d+) px", out)
    assert sorted(int(a) for a, _ in matches) == list(range(N)) and "Mismatch" not in out
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    rc0, out0, err0, lines0 = _run(common, tmp_path)
    assert rc0 == 0 and not err0 and "Detector gain map" not in out0
    plain = {json.loads(l)["file-number"]: json.loads(l) for l in lines0}
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    mask = np.ones((200, 300), np.uint8)
    differs = False
    for i, img in enumerate(frames):
        want = M.dispersion_gain_map(img, mask, gmap) if algo == "dispersion" else M.dispersion_extended_gain_map(img, mask, gmap)[0]
        cc = O.cc2d(want, img, 3)
        assert got[i]["num_strong_pixels"] == cc.num_strong_pixels == int(want.sum())
        assert got[i]["n_spots_total"] == len(cc.boxes)
        differs |= got[i]["num_strong_pixels"] != plain[i]["num_strong_pixels"]
    assert differs
