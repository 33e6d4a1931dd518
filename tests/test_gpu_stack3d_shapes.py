"""GPU: the 3D connected components of a rotation sweep (ffs_stack3d.hip, kernels_stack3d.hpp, k_union<true>) on the
voxel sets of tests/cc_shapes.py, handed to the kernels as they are by Stack3D.add_slice and held to O.cc3d bit for
bit.  tests/test_cc_shapes.py pins that truth without the oracle's own union-find."""
import numpy as np
import pytest

import cc_shapes as S
from oracle import oracle as O
from util import assert_reflections_equal

pytestmark = pytest.mark.gpu

OFF = (1, 0.0)             # min_spot_size_3d, max_peak_centroid_separation: every component comes out
DEFAULTS = (3, 2.0)
TWO = float(np.float32(2.0))
BELOW_TWO = float(np.nextafter(np.float32(2.0), np.float32(0.0)))


def _context(ffs, W, H, filters, **kw):
    ctx = ffs.Context(W, H, np.uint16, **kw)
    ctx.set_params(min_spot_size_3d=filters[0], max_peak_centroid_separation=filters[1])
    return ctx


def _feed(stack, slices, ids=None, order=None):
    ids = list(range(len(slices))) if ids is None else ids
    for j in (range(len(slices)) if order is None else order):
        stack.add_slice(ids[j], slices[j][0], slices[j][1])


def _result(stack):
    refl, n_calc, fs, fp = stack.finish()
    return refl, (n_calc, fs, fp), stack.signals()


def _assert_same_result(a, b):
    assert a[1] == b[1]
    assert_reflections_equal(a[0], b[0])
    for f in ("x", "y", "z", "intensity", "reflection"):
        np.testing.assert_array_equal(a[2][f], b[2][f], err_msg=f)


def _assert_oracle(stack, W, H, slices, filters):
    """finish() and signals() against O.cc3d on `slices` (z order), tol = 0."""
    got = _result(stack)
    refl, counts, sig = got
    want = O.cc3d(slices, W, H, *filters)
    assert counts == (want.n_calculated, want.n_filtered_size, want.n_filtered_sep), "(n_calculated, n_filtered_size, n_filtered_sep)"
    assert_reflections_equal(refl, want.reflections)
    np.testing.assert_array_equal(sig["reflection"], O.cc3d_signals(slices, W, H, *filters), err_msg="signals: reflection")
    x, y, z, inten = S.vertex_arrays(W, slices)
    for f, v in (("x", x), ("y", y), ("z", z), ("intensity", inten)):
        np.testing.assert_array_equal(sig[f], v, err_msg="signals: " + f)
    return got


def _run(ffs, fixture, filters, ids=None, order=None):
    W, H, slices, _ = fixture
    ctx = _context(ffs, W, H, filters)
    stack = ffs.Stack3D(ctx)
    _feed(stack, slices, ids, order)
    got = _assert_oracle(stack, W, H, slices, filters)
    stack.close()
    ctx.close()
    return got


# ---- topology --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["filters_off", "defaults", "shuffled"])
@pytest.mark.parametrize("name", sorted(S.TOPOLOGY))
def test_topology(ffs, name, mode):
    fixture = S.TOPOLOGY[name]()
    n = len(fixture[2])
    order = None
    if mode == "shuffled":                                  # arrival order is not z order
        order = list(np.random.default_rng(len(name)).permutation(n))
        if n > 1 and order == sorted(order):
            order = order[::-1]
    _run(ffs, fixture, DEFAULTS if mode == "defaults" else OFF, order=order)


def test_frame_ids_with_a_gap_are_neighbours(ffs):
    """z is the rank of the frame id: slices 7 and 19 are adjacent, their blobs are joined."""
    refl, counts, _ = _run(ffs, S.twin_slices(), OFF, ids=[7, 19])
    assert counts[0] == 2 and list(refl["z_max"] - refl["z_min"]) == [1, 1]


def test_checkerboard_is_all_roots_and_block_is_one(ffs):
    _, counts, _ = _run(ffs, S.checker_3d(), OFF)
    assert counts == (2048, 0, 0)
    refl, counts, _ = _run(ffs, S.solid(), OFF)
    assert counts == (1, 0, 0) and refl["num_pixels"][0] == 48 * 40 * 6


# ---- numerics --------------------------------------------------------------------------------------------------------

def test_peak_ties(ffs):
    refl, _, _ = _run(ffs, S.peak_ties(), OFF)
    got = [tuple(int(refl[f][i]) for f in ("peak_x", "peak_y", "peak_z", "peak_intensity", "num_pixels")) for i in range(len(refl))]
    assert got == S.PEAK_TIES_EXPECTED


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_separation_on_the_threshold(ffs, axis):
    """Peak and centroid exactly 2.0 apart: kept at 2.0 (the filter is a strict >), filtered one ulp below, kept at 0 (off)."""
    fixture = S.line5(axis)
    for sep, want in ((TWO, (1, 0, 0)), (BELOW_TWO, (1, 0, 1)), (0.0, (1, 0, 0))):
        refl, counts, sig = _run(ffs, fixture, (1, sep))
        assert counts == want, sep
        assert len(refl) == 1 - want[2] and (sig["reflection"] == (-1 if want[2] else 0)).all()
        if len(refl):
            assert refl["peak_centroid_distance"][0] == np.float32(2.0)


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_size_on_the_threshold(ffs, axis):
    fixture = S.line5(axis)
    for min_size, want in ((5, (1, 0, 0)), (6, (1, 1, 0)), (0, (1, 0, 0))):
        refl, counts, _ = _run(ffs, fixture, (min_size, 0.0))
        assert counts == want and len(refl) == 1 - want[1], min_size


def test_too_small_and_too_spread_counts_under_size(ffs):
    fixture = S.small_and_spread()
    assert _run(ffs, fixture, (8, 2.0))[1] == (1, 1, 0)
    assert _run(ffs, fixture, (7, 2.0))[1] == (1, 0, 1)


def test_wide_sums(ffs):
    """sum (2x+1) I of 53 bits: the centroid is exact, com_x = float32 10208.0, sum_intensity = 64 (2^32 - 1)."""
    fixture = S.wide_sums()
    refl, counts, _ = _run(ffs, fixture, OFF)
    assert counts == (1, 0, 0)
    assert refl["com_x"][0] == np.float32(10208.0) and refl["sum_intensity"][0] == 64 * (2 ** 32 - 1)
    assert _run(ffs, fixture, DEFAULTS)[1] == (1, 0, 1)       # 32 pixels from its peak


# ---- bookkeeping -----------------------------------------------------------------------------------------------------

def test_frame_added_twice_the_later_list_counts(ffs):
    W, H, s, _ = S.late_join()
    other = S.z_staircase()[2]
    ctx = _context(ffs, W, H, OFF)
    stack = ffs.Stack3D(ctx)
    stack.add_slice(0, *s[0])
    stack.add_slice(1, *other[3])                           # replaced below
    stack.add_slice(2, *s[2])
    stack.add_slice(1, *s[1])
    stack.add_slice(3, *s[3])
    stack.add_slice(3, *other[5])                           # replaces
    _assert_oracle(stack, W, H, [s[0], s[1], s[2], other[5]], OFF)
    stack.close(); ctx.close()


def test_frame_ids_are_ordered_as_int64(ffs):
    W, H, s, _ = S.z_staircase()
    ctx = _context(ffs, W, H, OFF)
    stack = ffs.Stack3D(ctx)
    stack.add_slice(2 ** 40, *s[2])
    stack.add_slice(0, *s[1])
    stack.add_slice(-5, *s[0])
    _, counts, _ = _assert_oracle(stack, W, H, s[:3], OFF)
    assert counts[0] == 1                                   # (ordered as unsigned: slices 1, 2, 0 -- two components)
    stack.close(); ctx.close()


def test_finish_twice_and_add_after_finish(ffs):
    W, H, s, _ = S.z_staircase()
    ctx = _context(ffs, W, H, OFF)
    stack = ffs.Stack3D(ctx)
    _feed(stack, s[1:6], ids=[11, 12, 13, 14, 15])
    first = _assert_oracle(stack, W, H, s[1:6], OFF)
    _assert_same_result(_result(stack), first)              # finish() again: identical
    stack.add_slice(3, *s[0])                               # sorts first: every z rank shifts by one
    third = _assert_oracle(stack, W, H, s[0:6], OFF)
    assert third[2]["z"].min() == 0 and third[0]["z_max"][0] == 5 and third[0]["num_pixels"][0] == 12
    stack.close(); ctx.close()


def test_pooled_stack_leaks_nothing(ffs):
    """A closed stack goes back to its context with its grown buffers; the next Stack3D takes it over."""
    W, H, big, _ = S.solid()
    ctx = _context(ffs, W, H, OFF)
    stack = ffs.Stack3D(ctx)
    _feed(stack, big)
    _assert_oracle(stack, W, H, big, OFF)
    stack.close()
    W2, H2, s, _ = S.late_join()
    assert (W2, H2) == (W, H)
    stack = ffs.Stack3D(ctx)
    assert stack.finish()[1:] == (0, 0, 0) and len(stack.signals()["x"]) == 0     # empty before anything is added
    _feed(stack, s)
    _assert_oracle(stack, W, H, s, OFF)
    stack.close(); ctx.close()


def test_max_total_strong_refuses_and_keeps_what_it_had(ffs):
    W, H, s, _ = S.late_join()
    n = [len(k) for k, _ in s]
    cap = n[0] + n[1] + n[2] + 1                            # the fourth slice (>= 2 entries) does not fit
    assert n[3] >= 2
    ctx = _context(ffs, W, H, OFF)
    stack = ffs.Stack3D(ctx, max_total_strong=cap)
    _feed(stack, s[:3])
    with pytest.raises(ffs.FfsError) as e:
        stack.add_slice(3, *s[3])
    assert e.value.code == -4 and "too many strong pixels" in str(e.value)        # FFS_ERR_OVERFLOW
    _assert_oracle(stack, W, H, s[:3], OFF)
    stack.close(); ctx.close()


# ---- delivery: the same voxel sets through the threshold and ffs_stack3d_add_batch ------------------------------------

BRIGHT = 1000


def _rendered(name):
    W, H, slices, _ = S.TOPOLOGY[name]()
    designed = [(k, np.full(len(k), BRIGHT, np.uint32)) for k, _ in slices]
    return W, H, S.render(W, H, slices, bright=BRIGHT), designed


def _by_add_slice(ffs, W, H, designed):
    return _run(ffs, (W, H, designed, ""), DEFAULTS)


def _process_into(stack, stream, frames, z0, designed):
    res = stream.process(frames[z0:z0 + stream.ctx.max_batch], first_frame_id=z0)
    for j, r in enumerate(res):                             # the fixture is what it claims to be
        np.testing.assert_array_equal(r.strong_k.astype(np.uint64), designed[z0 + j][0])
        np.testing.assert_array_equal(r.strong_intensity, designed[z0 + j][1])
    stack.add_batch(stream)


@pytest.mark.parametrize("name", ["late_join", "z_staircase"])
def test_delivery_by_add_batch(ffs, name):
    W, H, frames, designed = _rendered(name)
    mask = np.ones((H, W), np.uint8)
    for img, (k, _) in zip(frames, designed):               # the oracle's threshold gives the designed lists
        np.testing.assert_array_equal(np.flatnonzero(O.dispersion(img, mask)), k.astype(np.int64))
    want = _by_add_slice(ffs, W, H, designed)
    ctx = _context(ffs, W, H, DEFAULTS, max_batch=5)
    ctx.set_params(want_strong_list=1)
    stream = ctx.stream()
    stack = ffs.Stack3D(ctx)
    for z0 in range(0, len(frames), 5):
        _process_into(stack, stream, frames, z0, designed)
    _assert_same_result(_assert_oracle(stack, W, H, designed, DEFAULTS), want)
    stack.close(); stream.close(); ctx.close()


def _sweep_context(ffs, W, H):
    ctx = ffs.Context(W, H, np.uint16, max_batch=3, max_strong_per_frame=600)
    ctx.set_params(want_strong_list=1, min_spot_size_3d=4)
    return ctx


def _add_batch_of(stack, stream, frames, first_frame_id):
    res = stream.process(frames, first_frame_id=first_frame_id)
    stack.add_batch(stream)
    return [(r.strong_k.copy(), r.strong_intensity.copy()) for r in res]


def test_local_batches_with_overflow_frames_across_the_slot_ring(ffs):
    """One stream, one context, nine batches of three: the ninth add_batch takes slot 0 of the stack's eight slice tables again.
    Frames 4 (the middle of its batch) and 26 (the last of the ninth) hold ~50 % strong pixels, far beyond the lists' 600 entries
    (as test_gpu_parity.py::test_stack3d_takes_an_overflowing_frame_from_the_second_context makes them): their lists go up from the
    host to the places the batch's placement gives them, between and behind the frames the append kernel copies."""
    from ffs_amd import synth
    W, H, NZ = 200, 120, 27
    frames = synth.frames(synth.sweep_params(seed=91, n_frames=NZ, n_spots=30, width=W, height=H), range(NZ)).copy()
    rng = np.random.default_rng(5)
    for z in (4, 26):
        frames[z][rng.random((H, W)) < 0.5] += 400
    ctx = _sweep_context(ffs, W, H)
    stream = ctx.stream()
    stack = ffs.Stack3D(ctx)
    slices = []
    for z0 in range(0, NZ, 3):
        slices += _add_batch_of(stack, stream, frames[z0:z0 + 3], z0)
    assert len(slices[4][0]) > 5000 and len(slices[26][0]) > 5000 and len(slices[5][0]) < 600 and len(slices[25][0]) < 600
    refl, n_calc, fs, fp = stack.finish()
    want = O.cc3d(slices, W, H, 4, 2.0)
    assert (n_calc, fs, fp) == (want.n_calculated, want.n_filtered_size, want.n_filtered_sep)
    assert_reflections_equal(refl, want.reflections)
    stack.close(); stream.close(); ctx.close()


def test_frame_ids_delivered_twice_by_add_batch(ffs):
    """Ids 0-2, then ids 1-3 from other frames: the later lists count for 1 and 2, and the first batch's lists for them stay in
    the arrival buffers, dead -- the held slices' arrival offsets are not the running sum of their lengths."""
    from ffs_amd import synth
    W, H = 200, 120
    frames = synth.frames(synth.sweep_params(seed=91, n_frames=6, n_spots=30, width=W, height=H), range(6))
    ctx = _sweep_context(ffs, W, H)
    stream = ctx.stream()
    stack = ffs.Stack3D(ctx)
    first = _add_batch_of(stack, stream, frames[0:3], 0)
    later = _add_batch_of(stack, stream, frames[3:6], 1)
    assert all(len(k) > 0 for k, _ in first + later)
    _assert_oracle(stack, W, H, [first[0]] + later, (4, 2.0))
    stack.close(); stream.close(); ctx.close()


@pytest.mark.parametrize("transport", ["peer", "rccl"])
@pytest.mark.parametrize("name", ["late_join", "z_staircase"])
def test_delivery_from_a_second_context(ffs, name, transport, monkeypatch):
    """Batches alternate between two contexts on the one GPU; the second context's lists cross into the first one's
    stack by device copies and by RCCL (as test_gpu_parity.py::test_stack3d_fed_from_two_contexts)."""
    monkeypatch.setenv("FFS_GATHER", transport)
    used = ffs.multi_init([0, 0], transport)
    assert used == ("rccl" if transport == "rccl" else "none")
    W, H, frames, designed = _rendered(name)
    want = _by_add_slice(ffs, W, H, designed)
    ctxs = [_context(ffs, W, H, DEFAULTS, max_batch=2) for _ in range(2)]
    for c in ctxs:
        c.set_params(want_strong_list=1)
    streams = [c.stream() for c in ctxs]
    stack = ffs.Stack3D(ctxs[0])
    for b, z0 in enumerate(range(0, len(frames), 2)):
        _process_into(stack, streams[b % 2], frames, z0, designed)
    _assert_same_result(_assert_oracle(stack, W, H, designed, DEFAULTS), want)
    stack.close()
    for st, c in zip(streams, ctxs):
        st.close()
        c.close()
