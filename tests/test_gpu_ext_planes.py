"""GPU: the extended algorithm's erosion and final pass on the planes of tests/ext_planes.py -- frames whose signal region is dense
enough for the dense-tile branch of exact_tile, with its edges on every bit, on the seam of k_ext_erode_strips' 62-word strips, on
the row seams of the bands and tiles, in the columns where the quad path falls back, and with 0, 1 and 2 background pixels in a
window (tests/test_ext_planes.py holds the fixtures to that, on the CPU).  Every stage against the oracle, bit-exact, as
test_gpu_extended.test_every_stage_matches_oracle does for blob frames."""
import numpy as np
import pytest

import ext_planes as X
import gain_map_oracle as GM
import gain_oracle as G
from oracle import oracle as O
from util import assert_frame_matches_oracle, oracle_frame

pytestmark = pytest.mark.gpu

_WANT = {}


def _threshold(W):
    """Frames wider than 1024 run at half the noise range: at threshold 0, flavour 0 makes every signal-region pixel with fewer
    than two background pixels strong -- solid slabs of up to 2000 x 40 strong pixels, and the union-find has no path compression
    (nobody has measured the 2D sparse stage on such a slab, so this is a precaution, not a measured limit).
    The threshold enters the final test only: D and E stay as the census saw them.  Narrow frames keep threshold 0 and their slabs."""
    return X.WIDE_THRESHOLD if W > 1024 else 0.0


def want(kind, dtype, W, H, flavour):
    """(img, mask, (strong, first, eroded), what oracle_frame returns), from the oracle, once per process."""
    key = (kind, np.dtype(dtype).name, W, H, flavour)
    if key not in _WANT:
        img, mask, _ = X.fixture(kind, dtype, W, H)
        p = O.DispParams()
        O.lib().ffs_oracle_default_disp_params(O.C.byref(p))
        p.threshold = _threshold(W)
        planes = O.dispersion_extended(img, mask, p, flavour=flavour, debug=True)
        _WANT[key] = (img, mask, planes, oracle_frame(img, mask, strong=planes[0]))
    return _WANT[key]


def _context(ffs, dtype, W, H, flavour, max_batch=1, **tuning):
    ctx = ffs.Context(W, H, dtype, max_batch=max_batch, max_strong_per_frame=W * H)
    if tuning:
        ctx.set_tuning(**tuning)
    ctx.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=flavour, threshold=_threshold(W),
                   want_strong_mask=1, want_strong_list=1, want_reflections=1)
    return ctx


def _assert_plane(got, wanted, name, where=""):
    d = np.argwhere(got != wanted)
    assert d.size == 0, f"{name}{where}: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"


def _assert_frame(st, f, fr, img, mask, planes, precomputed, where=""):
    strong, first, eroded = planes
    _assert_plane(st.debug_bitplane(f, 1), first, "first pass", where)
    _assert_plane(st.debug_bitplane(f, 2), eroded, "erosion", where)
    _assert_plane(st.debug_bitplane(f, 0), strong, "strong plane", where)
    assert_frame_matches_oracle(fr, img, mask, precomputed=precomputed)


VARIANTS = {
    "default": dict(ext_first_pass=2, ext_erode=1),    # the streaming first pass, strips of 32 rows
    "erode0": dict(ext_first_pass=2, ext_erode=0),     # a lane per word column
    "erode2": dict(ext_first_pass=2, ext_erode=2),     # strips of 16 rows
    "fused": dict(ext_first_pass=2, ext_erode=1, ext_fused=1),   # the erosion in the final pass's tiles (an 18-row LDS window); 16-bit pixels
    "first0": dict(ext_first_pass=0, ext_erode=1),     # the one-pixel-per-lane first pass (what 32-bit pixels always take)
}


@pytest.mark.parametrize("shape", X.SHAPES, ids=X.shape_id)
@pytest.mark.parametrize("kind", ["dense", "islands"])
@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_planes(ffs, shape, kind, flavour, variant):
    dtype, W, H = shape
    if variant in ("fused", "first0") and np.dtype(dtype) == np.uint32:
        pytest.skip("32-bit pixels have one first-pass kernel and no fused erosion")
    img, mask, planes, pre = want(kind, dtype, W, H, flavour)
    ctx = _context(ffs, dtype, W, H, flavour, **VARIANTS[variant])
    ctx.set_mask(mask)
    st = ctx.stream()
    fr = st.process(img)[0]
    _assert_frame(st, 0, fr, img, mask, planes, pre)
    assert "extended" in st.last_path()[0]


@pytest.mark.parametrize("flavour,tuning", [(fl, dict(ext_erode=e, ext_e_sparse=s)) for fl in (0, 1) for e, s in ((1, 1), (2, 1), (1, 0), (0, 0))]
                         + [(0, dict(ext_fused=1))],
                         ids=lambda v: "-".join("%s%d" % kv for kv in v.items()) if isinstance(v, dict) else "flavour%d" % v)
def test_successive_batches_wide(ffs, flavour, tuning):
    """test_gpu_extended.test_planes_of_successive_batches at a width with a strip seam, the contents alternating between "almost
    every word set" and "almost every word zero": what an erosion that stores its non-zero words only, over a plane cleared behind
    the batch before, can get wrong.  One mask for the stream (the dense fixture's; the islands keep their image)."""
    dtype, W, H = np.uint16, 2080, 40
    mask = X.fixture("dense", dtype, W, H)[1]
    key = ("batches", flavour)
    if key not in _WANT:
        p = O.DispParams()
        O.lib().ffs_oracle_default_disp_params(O.C.byref(p))
        p.threshold = _threshold(W)
        frames = {}
        for kind in ("dense", "islands", "empty"):
            img = X.fixture(kind, dtype, W, H)[0]
            planes = O.dispersion_extended(img, mask, p, flavour=flavour, debug=True)
            frames[kind] = (img, planes, oracle_frame(img, mask, strong=planes[0]))
        _WANT[key] = frames
    frames = _WANT[key]
    assert frames["dense"][1][2].mean() > 0.8 and 0 < frames["islands"][1][2].mean() < 0.15 and not frames["empty"][1][1].any()
    ctx = _context(ffs, dtype, W, H, flavour, max_batch=3, **tuning)
    ctx.set_mask(mask)
    st = ctx.stream()
    for batch in (["dense", "islands"], ["empty"], ["islands", "dense", "islands"], ["dense"], ["empty", "islands"]):
        res = st.process(np.stack([frames[k][0] for k in batch]))
        assert "extended" in st.last_path()[0]
        for f, kind in enumerate(batch):
            img, planes, pre = frames[kind]
            _assert_frame(st, f, res[f], img, mask, planes, pre, where=f" (batch {batch}, frame {f})")


PREDICATE_SHAPES = [(np.uint16, 128, 24), (np.uint32, 128, 24), (np.uint32, 330, 40)]


@pytest.mark.parametrize("shape", PREDICATE_SHAPES, ids=X.shape_id)
@pytest.mark.parametrize("predicate", ["max_valid_window", "gain", "gain_map"])
def test_predicate_variants_dense(ffs, shape, predicate):
    """The TRUSTED and GAIN instantiations of ext_final_strong / ext_final_strong4 and of the first pass, on the dense fixtures and
    at the right edge (they have only seen blob frames).  Flavour 0 (the gain forms have no other).  max_valid at three quarters of
    the noise range masks a quarter of the pixels for the frame, so that variant's signal region is thin: what it holds to the
    fixture is the first pass (every pixel a candidate) and the windows at the frame's edges."""
    dtype, W, H = shape
    img, mask, _ = X.fixture("dense", dtype, W, H)
    ctx = _context(ffs, dtype, W, H, 0)
    ctx.set_mask(mask)
    if predicate == "max_valid_window":
        max_valid = 3 * X.NOISE_MAX[np.dtype(dtype).itemsize] // 4
        ctx.set_params(max_valid=max_valid)
        ctx.set_max_valid_scope("window")
        strong, first, eroded = O.dispersion_extended(img, (mask & (img <= max_valid)).astype(np.uint8), None, 0, float(max_valid), debug=True)
        assert not np.array_equal(strong, O.dispersion_extended(img, mask, None, 0, float(max_valid)))   # (the scope matters here)
    elif predicate == "gain":
        ctx.set_gain(2.5)
        strong, first, eroded = G.dispersion_extended_gain(img, mask, 2.5)
        assert eroded.mean() > 0.5
    else:
        gmap = np.broadcast_to((0.25 * 4.0 ** (np.arange(W) % 7)).astype(np.float32), (H, W))   # 0.25 .. 1024: differs from column to column
        ctx.set_gain_map(gmap)
        strong, first, eroded = GM.dispersion_extended_gain_map(img, mask, gmap)
        assert eroded.mean() > 0.5
    assert strong.sum() > 0 and not np.array_equal(strong, O.dispersion_extended(img, mask))
    st = ctx.stream()
    fr = st.process(img)[0]
    _assert_plane(st.debug_bitplane(0, 1), first, "first pass")
    _assert_plane(st.debug_bitplane(0, 2), eroded, "erosion")
    _assert_plane(st.debug_bitplane(0, 0), strong, "strong plane")
    assert_frame_matches_oracle(fr, img, mask, strong=strong)
    assert "extended" in st.last_path()[0]
