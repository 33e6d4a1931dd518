"""GPU: index assignment for many settings at once (ffs_ctx_index_assign) through the C ABI, byte for byte against tests/assign_oracle.py: the
records, hkl and lsq of two lattices under the settings from their own basis vectors plus the true cell, the cell doubled and the cell
halved; duplicate groups of 1 to 200 placed by hand; the corners of the arithmetic; the shapes; the passes under a small workspace; the
same call twice; a call while batches are in flight; index_correct on the doubled cell."""
import numpy as np
import pytest

import assign_cases as AC
import assign_oracle as AO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ffs):
    return ffs.Context(64, 48, np.uint16, max_batch=2)


def assert_equals_oracle(ffs, ctx, c, **kw):
    recs, hkl, lsq = ctx.index_assign(c["rlp"], c["phi"], c["A"], selected=c["selected"], tolerance=c["tolerance"], want_hkl=True, want_lsq=True, **kw)
    want = AC.expected(c)
    assert recs.dtype == AO.ASSIGNMENT_DT
    if recs.tobytes() != want[0].tobytes():
        bad = [k for k in range(len(recs)) if recs[k].tobytes() != want[0][k].tobytes()]
        k = bad[0]
        raise AssertionError((c["name"], "records", len(bad), k, [(f, recs[k][f], want[0][k][f]) for f in ("status", "n_accepted", "n_indexed", "n_out_of_range", "sum_lsq_q40")],
                              np.flatnonzero(recs[k]["absent0"] != want[0][k]["absent0"])[:5]))
    if hkl.tobytes() != want[1].tobytes():
        bad = np.argwhere(np.any(hkl != want[1], axis=2))
        raise AssertionError((c["name"], "hkl", len(bad), bad[:5], hkl[tuple(bad[0])], want[1][tuple(bad[0])]))
    assert lsq.tobytes() == want[2].tobytes(), (c["name"], "lsq", np.argwhere(lsq != want[2])[:5])
    return recs, hkl, lsq


@pytest.mark.parametrize("name,n_settings,total", (("small-disturbed", None, 709), ("triclinic-disturbed", 200, 4093)))
def test_the_lattices_under_their_own_settings(ffs, ctx, name, n_settings, total):
    c = AC.lattice(name, n_settings)
    recs, hkl, _ = assert_equals_oracle(ffs, ctx, c)
    k = c["n_own"]
    assert len(c["rlp"]) == total and len(c["A"]) == k + 3 and (n_settings is None or k == n_settings)
    # an oracle and a kernel that share a wrong convention cannot pass: the true setting explains the lattice
    assert recs[k]["n_indexed"] >= 0.9 * total and recs[k]["n_accepted"] > recs[k]["n_indexed"]
    assert recs[k + 1]["absent0"][0] > 0.99 * recs[k + 1]["n_indexed"] and ffs.index_absence_detect(recs[k + 1]) == 0 and ffs.index_absence_detect(recs[k]) == -1
    assert recs[k + 2]["n_accepted"] < 0.2 * total


def test_index_correct_halves_the_doubled_cell_three_times(ffs, ctx):
    c = AC.lattice("small-disturbed")
    k = c["n_own"]
    A, rec, hkl, rounds = ctx.index_correct(c["rlp"], c["phi"], c["A"][k + 1])
    want_A, want_rec, want_hkl, want_rounds = AO.correct(c["rlp"], c["phi"], c["A"][k + 1])
    volume = abs(np.linalg.det(c["axes"]))
    assert rounds == want_rounds == 3 and abs(1.0 / abs(np.linalg.det(A.reshape(3, 3))) - volume) <= 1e-9 * volume
    assert A.tobytes() == want_A.tobytes() and rec.tobytes() == want_rec.tobytes() and hkl.tobytes() == want_hkl.tobytes()


@pytest.mark.parametrize("name", [c["name"] for c in AC.built_groups() + AC.corners()])
def test_built_groups_and_the_corners_of_the_arithmetic(ffs, ctx, name):
    c = next(x for x in AC.built_groups() + AC.corners() if x["name"] == name)
    recs, hkl, lsq = assert_equals_oracle(ffs, ctx, c)
    if name == "built-groups":
        assert recs[0]["n_accepted"] - recs[0]["n_indexed"] > 600   # the groups of 64, 65 and 200 lose most of their members
    if name == "singular-among-good":
        assert recs["status"].tolist() == [0, 1, 1, 0, 1, 0, 1] and np.all(lsq[1] == -1.0) and not hkl[1].any() and recs[3]["n_out_of_range"] > 0
    if name == "range-edge":
        assert recs[0]["n_out_of_range"] == 3 and [524288, 1, 0] in hkl[0].tolist() and [-524288, 1, 0] in hkl[0].tolist()


_SHAPES = {}


def shape_case(n, m):
    if (n, m) not in _SHAPES:
        rlp, phi, A = AC.shaped(n)
        A = np.concatenate([A[:max(m - 3, 0)], A[len(A) - min(m, 3):]]) if m else A[:0]
        _SHAPES[(n, m)] = AC.case(f"shape-{n}-{m}", rlp, phi, A)
    return _SHAPES[(n, m)]


@pytest.mark.parametrize("m", (0, 1, 65))
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 4097))
def test_the_shapes(ffs, ctx, n, m):
    c = shape_case(n, m)
    assert c["rlp"].shape == (n, 3) and c["A"].shape == (m, 9)
    recs, hkl, lsq = assert_equals_oracle(ffs, ctx, c)
    assert recs.shape == (m,) and hkl.shape == (m, n, 3) and lsq.shape == (m, n)
    if n == 4097 and m == 65:
        assert recs[-3]["n_indexed"] > 3900 and recs[-3]["n_accepted"] - recs[-3]["n_indexed"] >= 4   # the spots added twice meet their twins


def test_the_passes_under_a_small_workspace_give_the_default_s_bytes(ffs, ctx):
    c = AC.lattice("small-disturbed")
    n = len(c["rlp"])
    one = 16 * n + 16 * 2048 + 4 + 20 * n   # csrc/assign_plan.hpp: one setting of 709 spots with hkl and lsq
    few = dict(c, A=c["A"][-12:], name="small-few")
    whole = assert_equals_oracle(ffs, ctx, few)
    for room in (one, 2 * one + 1, 5 * one, 12 * one):   # 12, 6, 3 (the last one short) and 1 passes
        again = assert_equals_oracle(ffs, ctx, few, workspace_bytes=room)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again)), room
    with pytest.raises(ffs.FfsError) as e:
        ctx.index_assign(c["rlp"], c["phi"], few["A"], want_hkl=True, want_lsq=True, workspace_bytes=one - 1)
    assert e.value.code == -3 and "one setting of 709 spots needs" in str(e.value), str(e.value)
    recs = ctx.index_assign(c["rlp"], c["phi"], few["A"], workspace_bytes=one - 20 * n)   # without hkl and lsq a setting is smaller
    assert recs.tobytes() == whole[0].tobytes()


def test_the_same_call_twice_and_the_wanted_outputs_on_and_off(ffs):
    c = AC.built_groups()[0]
    ctx = ffs.Context(64, 48, np.uint16, max_batch=1)
    assert set(ctx.index_assign(np.zeros((0, 3)), np.zeros(0), np.zeros((0, 9)), want_ms=True)[1].values()) == {0.0}
    a = assert_equals_oracle(ffs, ctx, c)
    b = assert_equals_oracle(ffs, ctx, c)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    recs = ctx.index_assign(c["rlp"], c["phi"], c["A"])
    recs_h, hkl = ctx.index_assign(c["rlp"], c["phi"], c["A"], want_hkl=True)
    recs_l, lsq, ms = ctx.index_assign(c["rlp"], c["phi"], c["A"], want_lsq=True, want_ms=True)
    assert recs.tobytes() == recs_h.tobytes() == recs_l.tobytes() == a[0].tobytes() and hkl.tobytes() == a[1].tobytes() and lsq.tobytes() == a[2].tobytes()
    assert list(ms) == list(ffs.INDEX_ASSIGN_LAUNCH_SPANS) and all(v > 0.0 for v in ms.values())


def test_a_call_while_batches_are_in_flight(ffs):
    from ffs_amd import synth
    W, H = 300, 200
    frames = synth.frames(synth.params(W, H, np.uint16, seed=5, background=2.0, n_spots=30), range(4))
    c = ffs.Context(W, H, np.uint16, max_batch=4)
    c.set_params(want_reflections=1)
    case = AC.lattice("small-disturbed")
    few = dict(case, A=case["A"][-12:], name="small-few")
    st, st2 = c.stream(), c.stream()
    before = st2.process(frames)
    st.submit(frames)
    assert_equals_oracle(ffs, c, few)
    after = st.wait()
    assert sum(r.num_strong_pixels for r in after) > 0
    for a, b in zip(before, after):
        assert a.num_strong_pixels == b.num_strong_pixels and a.boxes.tobytes() == b.boxes.tobytes() and a.reflections.tobytes() == b.reflections.tobytes()


def refused(ffs, call, *needles):
    with pytest.raises(ffs.FfsError) as e:
        call()
    assert e.value.code == -1 and all(n in str(e.value) for n in needles), str(e.value)


def test_every_refusal_through_the_live_context(ffs, ctx):
    rlp, phi, A = np.array([[0.1, 0.02, -0.03], [0.0, 0.2, 0.1]]), np.array([0.1, 0.2]), np.eye(3).reshape(1, 9)
    for bad in (0.0, -0.3, 0.51, np.inf, np.nan):
        refused(ffs, lambda: ctx.index_assign(rlp, phi, A, tolerance=bad), "ffs_ctx_index_assign", "tolerance must be in (0, 0.5]")
    refused(ffs, lambda: ctx.index_assign(np.where(np.arange(6).reshape(2, 3) == 4, np.nan, rlp), phi, A), "rlp", "not finite")
    refused(ffs, lambda: ctx.index_assign(rlp, [0.1, np.inf], A), "phi", "not finite")
    refused(ffs, lambda: ctx.index_assign(rlp, phi, A * np.nan), "A has an entry", "not finite")
    refused(ffs, lambda: ctx.index_assign(rlp, phi, np.tile(A, (4097, 1))), "n_candidates must be at most 4096")
    import ctypes as C
    lib = ffs.load_library()
    out = np.full(472, 7, np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.ffs_ctx_index_assign(ctx._h, None, p(phi), None, 2, p(A), 1, 0.3, 0, p(out), None, None) == -1 and b"NULL" in lib.ffs_last_error(ctx._h)
    assert lib.ffs_ctx_index_assign(ctx._h, p(rlp), p(phi), None, 2, None, 1, 0.3, 0, p(out), None, None) == -1 and b"NULL" in lib.ffs_last_error(ctx._h)
    assert lib.ffs_ctx_index_assign(ctx._h, p(rlp), p(phi), None, 2, p(A), 1, 0.3, 0, None, None, None) == -1 and b"NULL" in lib.ffs_last_error(ctx._h)
    assert lib.ffs_ctx_index_assign(ctx._h, p(rlp), p(phi), None, (1 << 20) + 1, p(A), 1, 0.3, 0, p(out), None, None) == -1 and b"1048577" in lib.ffs_last_error(ctx._h)
    assert np.all(out == 7), "a refused call writes nothing"
    assert lib.ffs_ctx_index_assign_launch_ms(ctx._h, None) == -1 and b"NULL" in lib.ffs_last_error(ctx._h)
    recs = ctx.index_assign(rlp, phi, A)   # the refused calls changed nothing
    assert recs.tobytes() == AO.assign_many(rlp, phi, A)[0].tobytes()
