"""GPU: the tie frames of tests/tie_windows.py through every route that decides a pixel -- 16- and 32-bit pixels, the three
threshold paths, wave logs and bit plane, rows_ahead 2 / 3 / 4, the byte-mask kernel and the run without lists, an overflowing
bright-window list, the extended algorithm's first pass and final test -- under every parameter set of tie_windows.PARAM_SETS.
Everything the C ABI returns is compared with the oracle bit for bit; the cells make sure the windows under test sit at,
and one step either side of, each conservative margin of the kernels."""
import numpy as np
import pytest

import tie_windows as T
from ffs_amd import bslz4
from oracle import oracle as O
from util import assert_frame_matches_oracle, oracle_frame

pytestmark = pytest.mark.gpu

DTYPES = {"u16": np.uint16, "u32": np.uint32}


def _standard_oracle(tf, img=None):
    img = tf.image if img is None else img
    strong = O.dispersion(img, tf.mask, tf.params.disp())
    if tf.params.max_valid >= 0:
        strong = strong & (img <= tf.params.max_valid)          # thresholding.cu:208-215
    return strong


def _check_cells(strong, tf):
    """The cells' own expected decisions (exact arithmetic) against what the oracle said: the frame still holds its ties."""
    mv = tf.params.max_valid
    for c in tf.cells:
        want = c.exact and not (mv >= 0 and c.p > mv)
        assert bool(strong[c.row, c.col]) == want, (c.family, c.side, c.m, c.x, c.y, c.p)


def _run(ffs, tf, tuning, want_mask=1, want_list=1, frames=None):
    H, W = tf.image.shape
    frames = tf.image[None] if frames is None else frames
    ctx = ffs.Context(W, H, tf.image.dtype, max_batch=len(frames))
    ctx.set_tuning(**tuning)
    ctx.set_mask(tf.mask)
    ctx.set_params(want_strong_mask=want_mask, want_strong_list=want_list, want_reflections=1, **tf.params.ctx_params())
    st = ctx.stream()
    return ctx, st, st.process(frames)


# (name, tuning, want_strong_mask, want_strong_list): a covering set of the routes, not their product
ROUTES_U16 = [
    ("default", {}, 1, 1),
    ("plane", {"strong_log": 0}, 1, 1),
    ("path1", {"threshold_path": 1}, 1, 1),
    ("path2", {"threshold_path": 2}, 1, 1),
    ("rows2", {"rows_ahead": 2}, 1, 1),
    ("rows4_plane", {"rows_ahead": 4, "strong_log": 0}, 1, 1),
    ("no_byte_mask", {}, 0, 1),
    ("no_lists", {}, 0, 0),
    ("no_lists_plane", {"strong_log": 0}, 0, 0),
    ("bright_overflow", {"strong_log": 0, "bright_cap": 2}, 1, 1),
]
ROUTES_U32 = [
    ("default", {}, 1, 1),
    ("path1", {"threshold_path": 1}, 1, 1),
    ("path2", {"threshold_path": 2}, 1, 1),
    ("rows2", {"rows_ahead": 2}, 1, 1),
    ("no_lists", {}, 0, 0),
    ("bright_overflow", {"bright_cap": 2}, 1, 1),
]


@pytest.mark.parametrize("dt,route", [("u16", r) for r in ROUTES_U16] + [("u32", r) for r in ROUTES_U32],
                         ids=lambda v: v if isinstance(v, str) else v[0])
def test_routes_default_params(ffs, dt, route):
    _, tuning, want_mask, want_list = route
    tf = T.frame(np.dtype(DTYPES[dt]).name)
    strong = _standard_oracle(tf)
    _check_cells(strong, tf)
    _, st, res = _run(ffs, tf, tuning, want_mask, want_list)
    assert_frame_matches_oracle(res[0], tf.image, tf.mask, strong=strong)
    path, reruns = st.last_path()
    if "bright_cap" in tuning:
        assert reruns >= 1, (path, reruns)       # the list overflowed and the batch went round again
    # (a whole tie frame overflows the 16-bit kernel's wave logs: the batch goes round again through the plane -- that route is
    # tested here; test_wave_logs sends the same cells in sparse frames through the logs)


# the wave-log routes of the 16-bit standard path, on the tie frame's cells spread over a batch of sparse frames
ROUTES_LOGS = [
    ("default", {}, 1, 1),
    ("rows2", {"rows_ahead": 2}, 1, 1),
    ("rows4", {"rows_ahead": 4}, 1, 1),
    ("no_byte_mask", {}, 0, 1),
    ("no_lists", {}, 0, 0),
]


@pytest.mark.parametrize("route", ROUTES_LOGS, ids=lambda v: v[0])
@pytest.mark.parametrize("name", ["default", "nsig_2.5_1.5", "threshold_41"])
def test_wave_logs(ffs, route, name):
    _, tuning, want_mask, want_list = route
    tf = T.frame("uint16", T.PARAM_SETS[name])
    frames, cells = tf.split(16)
    _, st, res = _run(ffs, tf, tuning, want_mask, want_list, frames=frames)
    path, reruns = st.last_path()
    assert "wave_logs" in path, (path, reruns)
    if want_list:
        assert reruns == 0, (path, reruns)   # (without lists the sparse stage's bands may send a batch round again: their own route)
    for fr, img, own in zip(res, frames, cells):
        strong = _standard_oracle(tf, img)
        for c in own:
            assert bool(strong[c.row, c.col]) == c.exact, (c.family, c.side)
        assert_frame_matches_oracle(fr, img, tf.mask, strong=strong)


@pytest.mark.parametrize("name", [n for n in T.PARAM_SETS if n != "default"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("route", [("default", {}), ("plane_path1", {"strong_log": 0, "threshold_path": 1}),
                                   ("path2", {"threshold_path": 2})], ids=lambda v: v[0])
def test_param_sets(ffs, name, dt, route):
    tf = T.frame(np.dtype(DTYPES[dt]).name, T.PARAM_SETS[name])
    strong = _standard_oracle(tf)
    _check_cells(strong, tf)
    _, _, res = _run(ffs, tf, route[1])
    assert_frame_matches_oracle(res[0], tf.image, tf.mask, strong=strong)


@pytest.mark.parametrize("name", ["default", "mincount3_maxvalid", "nsig_2.5_1.5", "nsig_b33", "threshold_41"])
@pytest.mark.parametrize("dt,first_pass", [("u16", 2), ("u16", 0), ("u32", 0)])
@pytest.mark.parametrize("flavour", [0, 1])
def test_extended(ffs, name, dt, first_pass, flavour):
    """The first-pass plane (where the drain's float32 sure / maybe band decides) and the final strong plane (family j: the
    flat-background ties of src >= mean + nsig_s sqrt(mean))."""
    prm = T.PARAM_SETS[name]
    tf = T.frame(np.dtype(DTYPES[dt]).name, prm)
    H, W = tf.image.shape
    ctx = ffs.Context(W, H, tf.image.dtype, max_batch=1)
    ctx.set_tuning(ext_first_pass=first_pass)
    ctx.set_mask(tf.mask)
    ctx.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=flavour, want_strong_mask=1, want_strong_list=1,
                   want_reflections=1, **prm.ctx_params())
    st = ctx.stream()
    fr = st.process(tf.image[None])[0]
    strong, first, eroded = O.dispersion_extended(tf.image, tf.mask, prm.disp(), flavour=flavour,
                                                  max_valid=float(prm.max_valid), debug=True)
    for c in tf.cells:
        assert bool(first[c.row, c.col]) == c.first_exact, (c.family, c.side)
    for r, col, fam, side, want in tf.ext_cells:
        assert bool(strong[r, col]) == want, (fam, side, r, col)
    d = np.argwhere(st.debug_bitplane(0, 1) != first)
    assert d.size == 0, f"first pass: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"
    assert np.array_equal(st.debug_bitplane(0, 2), eroded)
    assert np.array_equal(st.debug_bitplane(0, 0), strong)
    assert_frame_matches_oracle(fr, tf.image, tf.mask, strong=strong)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("at", [0, 1, 2])
@pytest.mark.parametrize("route", [("default", {}), ("plane", {"strong_log": 0})], ids=lambda v: v[0])
def test_batches(ffs, dt, at, route):
    """The tie frame first, in the middle and last of a batch of three beside a dense and an empty frame."""
    tf = T.frame(np.dtype(DTYPES[dt]).name)
    others = [T.dense_frame(tf.image.shape, tf.image.dtype), np.zeros_like(tf.image)]
    frames = np.stack(others[:at] + [tf.image] + others[at:])
    _, _, res = _run(ffs, tf, route[1], frames=frames)
    for fr, img in zip(res, frames):
        assert_frame_matches_oracle(fr, img, tf.mask, strong=_standard_oracle(tf, img))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_compressed_batch(ffs, dt):
    tf = T.frame(np.dtype(DTYPES[dt]).name)
    frames = [np.zeros_like(tf.image), tf.image, T.dense_frame(tf.image.shape, tf.image.dtype)]
    H, W = tf.image.shape
    ctx = ffs.Context(W, H, tf.image.dtype, max_batch=3)
    ctx.set_mask(tf.mask)
    ctx.set_params(want_strong_mask=1, want_strong_list=1, want_reflections=1, **tf.params.ctx_params())
    st = ctx.stream()
    res = st.process_compressed([bslz4.compress(f) for f in frames])
    for fr, img in zip(res, frames):
        assert_frame_matches_oracle(fr, img, tf.mask, precomputed=oracle_frame(img, tf.mask, strong=_standard_oracle(tf, img)))
