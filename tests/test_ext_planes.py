"""CPU: the fixtures of tests/ext_planes.py.  First the independent restatement (erode, background_counts, final) against the
oracle, bit for bit, on every fixture and both flavours; then the census -- conditions the fixtures must meet so that the GPU
tests reach the code they are built for (the dense-tile branch, the strip seam, the quad path's fall-back, m2 = 0 / 1 / 2, ...).
The conditions are measured against nothing and asserted on the oracle's planes alone: a fixture that drifts off its target fails
here, not silently on the GPU."""
import numpy as np
import pytest

import ext_planes as X
from oracle import oracle as O

KINDS = ["dense", "islands"]
_PLANES = {}


def planes(kind, shape, flavour):
    """(img, mask, strong, first, eroded) from the oracle, once per process (threshold as the GPU tests pass it)."""
    key = (kind, X.shape_id(shape), flavour)
    if key not in _PLANES:
        dtype, W, H = shape
        img, mask, _ = X.fixture(kind, dtype, W, H)
        p = O.DispParams()
        O.lib().ffs_oracle_default_disp_params(O.C.byref(p))
        p.threshold = threshold_of(W)
        _PLANES[key] = (img, mask) + O.dispersion_extended(img, mask, p, flavour=flavour, debug=True)
    return _PLANES[key]


def threshold_of(W):
    return X.WIDE_THRESHOLD if W > 1024 else 0.0


def _census(kind, shape, flavour):
    img, mask, _, first, eroded = planes(kind, shape, flavour)
    return X.census(img, mask, first, eroded, flavour)


both_flavours = pytest.mark.parametrize("flavour", [0, 1])
every_shape = pytest.mark.parametrize("shape", X.SHAPES, ids=X.shape_id)
every_kind = pytest.mark.parametrize("kind", KINDS)


# ---- the restatement against the oracle ----------------------------------------------------------------------------------

@every_shape
@every_kind
@both_flavours
def test_restatement_equals_oracle(kind, shape, flavour):
    img, mask, strong, first, eroded = planes(kind, shape, flavour)
    E = X.erode(first, mask, flavour)
    d = np.argwhere(E != eroded.astype(bool))
    assert d.size == 0, f"erosion: {len(d)} differences, first at (y,x)={d[:5].tolist()}"
    m2, x2 = X.background_counts(E, mask, img)
    S = X.final(img, m2, x2, E, flavour, 3.0, threshold_of(shape[1]))
    d = np.argwhere(S != strong.astype(bool))
    assert d.size == 0, f"final pass: {len(d)} differences, first at (y,x)={d[:5].tolist()}"
    assert strong.sum() > 0


def test_restatement_of_the_empty_frame():
    img, mask, _ = X.fixture("empty", np.uint16, 2080, 40)
    for flavour in (0, 1):
        strong, first, eroded = O.dispersion_extended(img, mask, flavour=flavour, debug=True)
        assert not first.any() and not eroded.any() and not strong.any()
        assert not X.erode(first, mask, flavour).any()


def test_generators_are_deterministic_and_in_range():
    for kind in KINDS:
        for dtype, W, H in X.SHAPES:
            gen = getattr(X, kind)
            img, mask, note = gen(dtype, W, H, 0)
            img2, mask2, _ = gen(dtype, W, H, 0)
            assert np.array_equal(img, img2) and np.array_equal(mask, mask2) and isinstance(note, str)
            assert img.shape == mask.shape == (H, W) and img.dtype == np.dtype(dtype) and mask.dtype == np.uint8
            assert not np.array_equal(img, gen(dtype, W, H, 1)[0])
            if np.dtype(dtype).itemsize == 4:
                assert 3 <= (img >= X.BIG).sum() <= 12            # a handful at and above 2^24
                assert ((img >= X.BIG) & (mask != 0)).sum() >= 3
            else:
                assert img.max() <= 60000
            assert (mask == 0).all(0).sum() == 1                   # one whole masked column


# ---- the census ------------------------------------------------------------------------------------------------------------

WIDE16 = [s for s in X.SHAPES if s[1] > 1024]
SEAMED = [s for s in X.SHAPES if s[1] > X.SEAM]


@pytest.mark.parametrize("shape", WIDE16, ids=X.shape_id)
@both_flavours
def test_dense_tiles_16bit(shape, flavour):
    """MODE 2 / 3 take the dense-tile branch when a tile holds more than LIST_CAP groups of four.  Every whole tile does; a last
    tile of a single row (H = 33, 17) holds at most W / 4 <= 520 groups and cannot."""
    c = _census("dense", shape, flavour)
    assert shape[1] // 4 * X.TILE_ROWS > X.LIST_CAP
    for rows, groups in zip(c["tile_rows"], c["tile_groups"]):
        if rows == X.TILE_ROWS:
            assert groups > X.LIST_CAP, c["tile_groups"]
    assert sum(r == X.TILE_ROWS for r in c["tile_rows"]) >= 2
    # (both lists' tails: the short tile takes the usual branch beside them)
    if c["tile_rows"][-1] < X.TILE_ROWS:
        assert 1 <= c["tile_groups"][-1] <= X.LIST_CAP


@both_flavours
def test_dense_tiles_32bit(flavour):
    """MODE 1: an entry per pixel of the signal region."""
    c = _census("dense", (np.uint32, 330, 40), flavour)
    assert c["tile_rows"] == [X.TILE_ROWS] * 5
    assert all(n > X.LIST_CAP for n in c["tile_pixels"]), c["tile_pixels"]


@every_shape
@both_flavours
def test_islands_are_sparse(shape, flavour):
    c = _census("islands", shape, flavour)
    entries = c["tile_pixels"] if np.dtype(shape[0]).itemsize == 4 else c["tile_groups"]
    assert any(1 <= n <= X.LIST_CAP for n in entries), entries
    assert c["zero_words_in_live_rows"] >= 1


@both_flavours
def test_edges_at_every_bit_position(flavour):
    c = _census("dense", (np.uint16, 2080, 40), flavour)
    every = set(range(32))
    assert c["E_rise"] == every and c["E_fall"] == every
    assert c["D_rise"] == every and c["D_fall"] == every


@pytest.mark.parametrize("shape", SEAMED, ids=X.shape_id)
@every_kind
@both_flavours
def test_strip_seam(kind, shape, flavour):
    """E differs between x = 1983 and x = 1984 in both directions.  One exception that no frame can avoid: at W = 1985 under
    flavour 0, x = 1984 is the last column, its clipped 5x5 is a subset of that of x = 1983, and a masked pixel at 1984 erodes 1983
    too -- so E cannot be 1 at 1983 and 0 at 1984 there (flavour 1 skips the masked pixel and can)."""
    c = _census(kind, shape, flavour)
    assert c["seam_E_rise"] >= 1
    if not (shape[1] == X.SEAM + 1 and flavour == 0):
        assert c["seam_E_fall"] >= 1
    assert c["E_at_seam_column"] >= 1 and c["seam_E_pixels"] >= 10
    if kind == "dense":
        assert c["seam_D_rise"] >= 1
    # Pixels at 1982 / 1983 that only columns from 1984 on erode, and pixels at 1984 / 1985 that only columns up to 1983 erode: the
    # words that lanes 63 and 0 of k_ext_erode_strips carry.  Flavour 0 has the masked singles at 1984 and 1983 for both; under
    # flavour 1 only holes of D erode, and the second seam patch (D's hole at 1983) needs a second slot of rows: H >= 33.
    # `islands` has a noise patch for each below its island across the seam, from rows 24 and 32.
    H = shape[2]
    if flavour == 0 or kind == "dense" or H >= 33:
        assert c["seam_carry_lane63"] >= 1
    if flavour == 0 or (kind == "dense" and H >= 33) or H >= 40:
        assert c["seam_carry_lane0"] >= 1


@pytest.mark.parametrize("shape", [(np.uint16, 2048, 24), (np.uint16, 128, 24), (np.uint16, 125, 24)], ids=X.shape_id)
@every_kind
@both_flavours
def test_quad_path_guard(kind, shape, flavour):
    """Groups with x < 8 or x + 12 > pitch_px leave the quad path for ext_final_strong, whose 12-pixel row is clamped at the right."""
    c = _census(kind, shape, flavour)
    assert c["E_left"] >= 50 and c["E_right"] >= 50, (c["E_left"], c["E_right"])


@every_shape
@every_kind
@both_flavours
def test_clipped_windows(kind, shape, flavour):
    c = _census(kind, shape, flavour)
    assert c["E_top"] >= 50 and c["E_bottom"] >= 50, (c["E_top"], c["E_bottom"])


@pytest.mark.parametrize("shape", [s for s in X.SHAPES if s[1] >= 300], ids=X.shape_id)
@both_flavours
def test_background_counts(shape, flavour):
    """m2 = 0 (flavour 1: never strong), m2 = 1 (the mean is 0, not x2 / 1), m2 = 2 (the first real mean) and the usual case."""
    c = _census("dense", shape, flavour)
    assert min(c["m2_0"], c["m2_1"], c["m2_2"]) >= 10, (c["m2_0"], c["m2_1"], c["m2_2"])
    assert c["m2_3plus"] >= 1000


@every_shape
@every_kind
@both_flavours
def test_flavours_differ(kind, shape, flavour):
    assert _census(kind, shape, flavour)["flavours_differ"] >= 100


@every_shape
@both_flavours
def test_row_seams(shape, flavour):
    """E changes across the seams of the 8-row tiles and the 16- and 32-row bands."""
    H = shape[2]
    c = _census("dense", shape, flavour)
    for y in (8, 16, 32):
        if y < H:
            assert y in c["rows_E_changes"], (y, sorted(c["rows_E_changes"]))
    img, mask, _, first, _ = planes("dense", shape, flavour)
    # ... and a hole of D (valid pixels, not the masked ones) lies across each of them
    hole = ~first.astype(bool) & (mask != 0)
    for y in (8, 16, 32):
        if y < H:
            assert (hole[y - 1] & hole[y]).any(), y
