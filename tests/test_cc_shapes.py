"""CPU: the voxel sets of tests/cc_shapes.py -- the oracle's 3D connected components (its own union-find) against the
independent sparse-graph formulation on every topology fixture, and against hand-known answers on every numeric one.
This pins the truth tests/test_gpu_stack3d_shapes.py holds the kernels to."""
from fractions import Fraction

import numpy as np
import pytest

import cc_shapes as S
from oracle import oracle as O


def _topology(name):
    W, H, slices, note = S.TOPOLOGY[name]()
    assert note == name
    return W, H, slices


@pytest.mark.parametrize("name", sorted(S.TOPOLOGY))
def test_fixture_respects_the_limits(name):
    W, H, slices = _topology(name)
    x, y, z, inten = S.vertex_arrays(W, slices)
    assert len(x) <= 65536
    assert (inten >= 1).all()
    for k, i in slices:
        assert k.dtype == np.uint64 and i.dtype == np.uint32 and len(k) == len(i)
        assert (np.diff(k.astype(np.int64)) > 0).all() and (len(k) == 0 or int(k[-1]) < W * H)


@pytest.mark.parametrize("name", sorted(S.TOPOLOGY))
def test_oracle_matches_the_graph_formulation(name):
    W, H, slices = _topology(name)
    r = O.cc3d(slices, W, H, 1, 0.0)                       # filters off: every component comes out, in label order
    sig = O.cc3d_signals(slices, W, H, 1, 0.0)
    _, lab = S._helix_components(S.volume_of(W, H, slices))
    n = int(lab.max()) + 1 if len(lab) else 0
    assert r.n_calculated == n == len(r.reflections)
    assert np.array_equal(sig, lab)                        # the label of every voxel
    x, y, z, _ = S.vertex_arrays(W, slices)
    for f, v in (("x", x), ("y", y), ("z", z)):
        lo = np.full(n, np.iinfo(np.int64).max); hi = np.full(n, -1)
        np.minimum.at(lo, lab, v); np.maximum.at(hi, lab, v)
        assert np.array_equal(r.reflections[f + "_min"], lo), f
        assert np.array_equal(r.reflections[f + "_max"], hi), f
    assert np.array_equal(r.reflections["num_pixels"], np.bincount(lab, minlength=n))


def test_topology_fixtures_are_what_they_claim():
    """Component counts and the label orders the fixtures were built for, by the graph formulation alone."""
    def labels(name):
        W, H, slices = _topology(name)
        return slices, S._helix_components(S.volume_of(W, H, slices))[1]

    for name in ("late_join", "late_join_last_row"):
        slices, lab = labels(name)
        assert lab.max() == 1
        n0 = len(slices[0][0])
        first = lab[:n0]                                   # slice 0: arm, the third, ..., arm
        assert first[0] == 0 and first[-1] == 0 and (first[1:-1] == 1).all() and n0 >= 4
        # without the last slice the arms are apart
        W, H, _ = _topology(name)
        assert S._helix_components(S.volume_of(W, H, slices[:-1]))[1].max() == 2
    if True:
        W, H, slices = _topology("late_join_last_row")
        assert int(slices[-1][0][-1]) // W == H - 1        # the bridge runs through the last row of the last slice
    assert labels("z_staircase")[1].max() == 0
    assert labels("z_diagonal")[1].max() == 11
    assert labels("serpentine")[1].max() == 0
    slices, lab = labels("row_wrap_3d")
    # slice 0: 1 + 3 * 2; slices 1-2: 8 singles; slice 3: 2; slice 4: 2; slice 5: 2
    assert lab.max() + 1 == 7 + 8 + 2 + 2 + 2
    assert labels("empty_between")[1].max() + 1 == 4
    slices, lab = labels("empty_first_last")
    assert lab.max() + 1 == 2 and len(slices[0][0]) == 0 and len(slices[-1][0]) == 0
    assert labels("twin_slices")[1].max() + 1 == 2
    assert len(labels("only_empty")[1]) == 0 and len(labels("no_slices")[1]) == 0
    slices, lab = labels("checker_3d")
    assert len(lab) == 2048 and lab.max() + 1 == 2048 and [len(k) for k, _ in slices] == [512] * 4
    slices, lab = labels("solid")
    assert len(lab) == 48 * 40 * 6 and lab.max() == 0
    W, H, slices = _topology("empty_first_last")
    assert O.cc3d(slices, W, H, 1, 0.0).reflections["z_min"].min() == 1   # z ranks start at 1


def test_chunk_edges_cover_every_root_combination():
    """Entry counts as asked, and for the two entries a thread of k_finalize_roots3d handles every combination of root /
    non-root at the first and at the last thread of a chunk -- also with a component that spans the chunk boundary."""
    seen = set()
    for total in S.CHUNK_TOTALS:
        W, H, slices, _ = S.chunk_edges(total)
        root, lab = S.root_flags(W, H, slices)
        assert len(root) == total
        for b in range(S.ROOT_CHUNK, total + 1, S.ROOT_CHUNK):
            spans = b < total and lab[b] == lab[b - 1]
            seen.add(("last", bool(root[b - 2]), bool(root[b - 1]), bool(spans)))
            if b + 1 < total:
                seen.add(("first", bool(root[b]), bool(root[b + 1]), bool(spans)))
            elif b < total:
                seen.add(("first-alone", bool(root[b]), bool(spans)))
        seen.add(("end", total % 2, bool(root[total - 1])))
    for r0 in (False, True):
        for r1 in (False, True):
            assert ("last", r0, r1, True) in seen and ("last", r0, r1, False) in seen, (r0, r1)
            assert ("first", r0, r1, not r0) in seen, (r0, r1)       # a non-root at a chunk's start spans the boundary
    assert {("first-alone", True, False), ("first-alone", False, True)} <= seen
    assert {("end", 1, True), ("end", 1, False), ("end", 0, True), ("end", 0, False)} <= seen


# ---- numerics --------------------------------------------------------------------------------------------------------

def test_peak_ties_smallest_zyx_wins():
    W, H, slices, _ = S.peak_ties()
    r = O.cc3d(slices, W, H, 1, 0.0).reflections
    got = [tuple(int(r[f][i]) for f in ("peak_x", "peak_y", "peak_z", "peak_intensity", "num_pixels")) for i in range(len(r))]
    assert got == S.PEAK_TIES_EXPECTED


TWO = np.float32(2.0)
BELOW_TWO = np.nextafter(np.float32(2.0), np.float32(0.0))


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_separation_on_the_threshold(axis):
    W, H, slices, _ = S.line5(axis)
    r = O.cc3d(slices, W, H, 1, 0.0)
    assert r.n_calculated == 1
    a = r.reflections[0]
    want_peak = {"x": (17, 9, 0), "y": (17, 9, 0), "z": (17, 9, 0)}[axis]
    assert (a["peak_x"], a["peak_y"], a["peak_z"], a["peak_intensity"]) == want_peak + (3,)
    com = {"x": (19.5, 9.5, 0.5), "y": (17.5, 11.5, 0.5), "z": (17.5, 9.5, 2.5)}[axis]
    assert (a["com_x"], a["com_y"], a["com_z"]) == com
    assert a["peak_centroid_distance"] == TWO and a["sum_intensity"] == 9
    kept = O.cc3d(slices, W, H, 1, float(TWO))
    assert (len(kept.reflections), kept.n_filtered_sep) == (1, 0)          # strict >: kept at the threshold
    cut = O.cc3d(slices, W, H, 1, float(BELOW_TWO))
    assert (len(cut.reflections), cut.n_filtered_sep, cut.n_filtered_size) == (0, 1, 0)


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_size_on_the_threshold(axis):
    W, H, slices, _ = S.line5(axis)
    for min_size, kept in ((5, 1), (6, 0), (0, 1)):
        r = O.cc3d(slices, W, H, min_size, 0.0)
        assert (len(r.reflections), r.n_filtered_size, r.n_filtered_sep) == (kept, 1 - kept, 0), min_size


def test_too_small_and_too_spread_counts_under_size():
    W, H, slices, _ = S.small_and_spread()
    a = O.cc3d(slices, W, H, 1, 0.0).reflections[0]
    assert a["num_pixels"] == 7 and a["peak_x"] == 30 and a["peak_centroid_distance"] == np.float32(3.0)
    r = O.cc3d(slices, W, H, 8, 2.0)
    assert (len(r.reflections), r.n_filtered_size, r.n_filtered_sep) == (0, 1, 0)
    r = O.cc3d(slices, W, H, 7, 2.0)
    assert (len(r.reflections), r.n_filtered_size, r.n_filtered_sep) == (0, 0, 1)


def test_wide_sums_are_exact():
    W, H, slices, _ = S.wide_sums()
    k, inten = slices[0]
    xs = [int(v) % W for v in k]
    sx = sum((2 * x + 1) * int(i) for x, i in zip(xs, inten))
    assert sx.bit_length() == 53                            # inside the domain where the reference is order-independent
    r = O.cc3d(slices, W, H, 1, 0.0)
    assert r.n_calculated == 1
    a = r.reflections[0]
    tot = sum(int(i) for i in inten)
    assert a["sum_intensity"] == tot == 64 * (2 ** 32 - 1)
    cx = Fraction(sx, 2 * tot)                              # exact rational centroid
    assert cx == Fraction(10208) and a["com_x"] == np.float32(10208.0)
    assert a["com_y"] == np.float32(S.WIDE_ROW + 0.5) and a["com_z"] == np.float32(0.5)
    assert (a["x_min"], a["x_max"], a["num_pixels"], a["peak_x"]) == (S.WIDE_X0, W - 1, 64, S.WIDE_X0)


# ---- delivery --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["late_join", "z_staircase"])
def test_rendered_frames_threshold_back_to_the_voxel_set(name):
    """One-pixel lines of a bright value on a quiet background: the dispersion threshold returns exactly the lines."""
    W, H, slices = _topology(name)
    frames = S.render(W, H, slices)
    mask = np.ones((H, W), np.uint8)
    for img, (k, _) in zip(frames, slices):
        assert np.array_equal(np.flatnonzero(O.dispersion(img, mask)), k.astype(np.int64))
