"""GPU: the indexer's basis-vector search (ffs_ctx_index_grid, ffs_ctx_index_peaks and the host-only ffs_index_* entries) through the C ABI,
bit for bit against tests/index_oracle.py: the power grid, `used`, the statistics, the peaks and the candidate vectors for every case of
tests/index_cases.py at n_points 16, 32 and 64 (the smallest sizes that still have every stage and the slab path, one instantiation each)
and one lattice at 128; at 256 one lattice against `ffs_hosttool indexbasis`, the CPU twin compiled from the same header (the test hashes
the 134 MB it copies out); the same call twice; a call at another n_points on one context; batches in flight while index calls run."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import index_cases as K
import index_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTTOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
CASES = {c["name"]: c for c in K.cases()}
SIZES = (16, 32, 64)
_oracle = {}


def expected(name, n_points):
    """The oracle's chain for a case at a grid size, computed once."""
    if (name, n_points) not in _oracle:
        c = CASES[name]
        _oracle[(name, n_points)] = O.chain(c["g"], c["xyz"], c["max_cell"], n_points, c["dmin"])
    return _oracle[(name, n_points)]


@pytest.fixture(scope="module")
def ctx(ffs):
    return ffs.Context(64, 48, np.uint16, max_batch=2)


def stats_bytes(stats):
    st = np.zeros((), O.STATS_DT)
    for k in O.STATS_DT.names:
        st[k] = stats[k]
    return st.tobytes()


def run_chain(ffs, ctx, c, n_points):
    """the chain through the ABI, step by step: a dict like the oracle's"""
    rlp, s1, mm = ffs.index_rlp(c["g"], c["xyz"])
    dmin, b_iso = ffs.index_defaults(rlp, c["max_cell"], n_points, c["dmin"])
    cell, weight = ffs.index_map(rlp, dmin, b_iso, n_points)
    used, power = ctx.index_grid(rlp, dmin, b_iso, n_points, want_power=True)
    peaks, stats = ctx.index_peaks(O.RMSD_CUTOFF)
    return dict(rlp=rlp, s1=s1, xyz_mm=mm, dmin=dmin, b_iso=b_iso, cell=cell, weight=weight, used=used, power=power, peaks=peaks, stats=stats,
                vectors=ffs.index_basis_vectors(peaks, n_points, dmin, c["max_cell"]))


def assert_chain_equal(got, want, what):
    assert (got["dmin"], got["b_iso"]) == (want["dmin"], want["b_iso"]), what
    for k in ("rlp", "s1", "xyz_mm", "cell", "weight", "used"):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (what, k)
    if got["power"].tobytes() != want["power"].tobytes():
        bad = np.flatnonzero(got["power"] != want["power"])
        raise AssertionError((what, "power grid", len(bad), bad[:5], got["power"][bad[:5]], want["power"][bad[:5]]))
    assert stats_bytes(got["stats"]) == want["stats"].tobytes(), (what, got["stats"], want["stats"])
    assert got["peaks"].tobytes() == want["peaks"].tobytes(), (what, "peaks", len(got["peaks"]), len(want["peaks"]))
    assert got["vectors"].tobytes() == want["vectors"].tobytes(), (what, "vectors", got["vectors"], want["vectors"])


@pytest.mark.parametrize("n_points", SIZES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_equals_the_oracle_bit_for_bit(ffs, ctx, name, n_points):
    assert_chain_equal(run_chain(ffs, ctx, CASES[name], n_points), expected(name, n_points), (name, n_points))


def test_a_lattice_at_128(ffs, ctx):
    got, want = run_chain(ffs, ctx, CASES["small-disturbed"], 128), expected("small-disturbed", 128)
    assert_chain_equal(got, want, "small-disturbed at 128")
    assert len(got["peaks"]) > 20 and len(got["vectors"]) >= 3


def test_the_convenience_call_runs_the_chain(ffs, ctx):
    c = CASES["triclinic-disturbed"]
    assert ctx.index_basis(c["xyz"], c["g"], c["max_cell"], n_points=64).tobytes() == expected("triclinic-disturbed", 64)["vectors"].tobytes()


def test_at_256_the_grid_and_the_records_are_the_host_tools(ffs, ctx, tmp_path):
    c = CASES["triclinic-disturbed"]
    centres, prefix = str(tmp_path / "c.centres"), str(tmp_path / "twin")
    c["xyz"].astype("<f8").tofile(centres)
    g = c["g"]
    run = subprocess.run([HOSTTOOL, "indexbasis", "centres=" + centres, "distance=150.0", "beam_x=1231.4", "beam_y=1263.7", "pixel_x=0.172", "pixel_y=0.172",
                          "wavelength=1.0", "osc_start=0.0", "osc_width=0.25", f"max-cell={c['max_cell']!r}", "npoints=256", "out=" + prefix], capture_output=True, text=True)
    assert run.returncode == 0 and "Candidate basis vectors:" in run.stdout, (run.stdout[-500:], run.stderr[-500:])
    assert np.array_equal(g["d_matrix"], K.geometry(0.172, 150.0, (1231.4, 1263.7))["d_matrix"])
    rlp, _, _ = ffs.index_rlp(g, c["xyz"])
    dmin, b_iso = ffs.index_defaults(rlp, c["max_cell"], 256)
    used, power, ms = ctx.index_grid(rlp, dmin, b_iso, 256, want_power=True, want_ms=True)
    assert ms > 0.0 and used.sum() > 3000
    assert hashlib.sha256(power.tobytes()).hexdigest() == open(prefix + ".grid_sha256").read().strip()
    peaks, stats = ctx.index_peaks(O.RMSD_CUTOFF)
    assert len(peaks) > 100 and peaks.tobytes() == open(prefix + ".peaks", "rb").read()
    vectors = ffs.index_basis_vectors(peaks, 256, dmin, c["max_cell"])
    assert len(vectors) >= 3 and vectors.tobytes() == open(prefix + ".basis_vectors", "rb").read()


def test_two_calls_give_identical_bytes_and_another_size_works_on_the_same_context(ffs):
    c = CASES["orthogonal-disturbed"]
    ctx = ffs.Context(64, 48, np.uint16, max_batch=1)
    a = run_chain(ffs, ctx, c, 64)
    b = run_chain(ffs, ctx, c, 64)
    assert a["power"].tobytes() == b["power"].tobytes() and a["peaks"].tobytes() == b["peaks"].tobytes() and a["stats"] == b["stats"]
    assert_chain_equal(run_chain(ffs, ctx, c, 32), expected("orthogonal-disturbed", 32), "32 after 64")
    assert_chain_equal(run_chain(ffs, ctx, c, 64), expected("orthogonal-disturbed", 64), "64 after 32")
    # the peaks of the resident grid again, at another cutoff and at the first
    loose, _ = ctx.index_peaks(5.0)
    again, _ = ctx.index_peaks(O.RMSD_CUTOFF)
    assert len(loose) != len(a["peaks"]) and again.tobytes() == a["peaks"].tobytes()
    want, _ = O.peaks(a["power"], 64, 5.0)
    assert loose.tobytes() == want.tobytes()


def test_the_launch_times_by_stage_add_up_to_the_calls(ffs):
    c = CASES["triclinic-disturbed"]
    ctx = ffs.Context(64, 48, np.uint16, max_batch=1)
    assert set(ctx.index_launch_ms().values()) == {0.0}, "zeros before the first call"
    rlp, _, _ = ffs.index_rlp(c["g"], c["xyz"])
    dmin, b_iso = ffs.index_defaults(rlp, c["max_cell"], 64)
    _, grid_ms = ctx.index_grid(rlp, dmin, b_iso, 64, want_ms=True)
    spans = ctx.index_launch_ms()
    assert list(spans) == list(ffs.INDEX_LAUNCH_SPANS)
    grid = [spans[k] for k in ffs.INDEX_LAUNCH_SPANS[:5]]
    assert all(v > 0.0 for v in grid) and all(spans[k] == 0.0 for k in ffs.INDEX_LAUNCH_SPANS[5:])
    assert abs(sum(grid) - grid_ms) <= 0.01 * grid_ms + 0.002   # (consecutive intervals between events of one stream; float32 milliseconds)
    peaks, _, peaks_ms = ctx.index_peaks(want_ms=True)
    spans = ctx.index_launch_ms()
    rest = [spans[k] for k in ffs.INDEX_LAUNCH_SPANS[5:]]
    assert len(peaks) > 0 and all(v > 0.0 for v in rest) and [spans[k] for k in ffs.INDEX_LAUNCH_SPANS[:5]] == grid
    assert abs(sum(rest) - peaks_ms) <= 0.01 * peaks_ms + 0.002
    lib = ffs.load_library()
    assert lib.ffs_ctx_index_launch_ms(ctx._h, None) == -1 and b"NULL" in lib.ffs_last_error(ctx._h)


def test_index_calls_while_batches_are_in_flight(ffs):
    from ffs_amd import synth
    W, H = 300, 200
    frames = synth.frames(synth.params(W, H, np.uint16, seed=5, background=2.0, n_spots=30), range(4))
    c = ffs.Context(W, H, np.uint16, max_batch=4)
    c.set_params(want_reflections=1)
    case = CASES["small-disturbed"]
    want = expected("small-disturbed", 32)
    st, st2 = c.stream(), c.stream()
    before = st2.process(frames)
    st.submit(frames)
    busy = run_chain(ffs, c, case, 32)
    after = st.wait()
    assert_chain_equal(busy, want, "while a batch is in flight")
    assert sum(r.num_strong_pixels for r in after) > 0
    for a, b in zip(before, after):
        assert a.num_strong_pixels == b.num_strong_pixels and a.boxes.tobytes() == b.boxes.tobytes() and a.reflections.tobytes() == b.reflections.tobytes()


def refused(ffs, call, *needles):
    with pytest.raises(ffs.FfsError) as e:
        call()
    assert e.value.code == -1 and all(n in str(e.value) for n in needles), str(e.value)


def test_every_refusal_through_the_live_context(ffs):
    ctx = ffs.Context(64, 48, np.uint16, max_batch=1)
    rlp = np.array([[0.1, 0.02, -0.03], [0.0, 0.2, 0.1]])
    refused(ffs, lambda: ctx.index_peaks(15.0), "no grid is resident")
    for n in (0, 8, 24, 512, 100):
        refused(ffs, lambda: ctx.index_grid(rlp, 2.0, 10.0, n), "n_points")
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(ffs, lambda: ctx.index_grid(rlp, bad, 10.0, 16), "dmin")
    refused(ffs, lambda: ctx.index_grid(rlp, 2.0, np.nan, 16), "b_iso")
    refused(ffs, lambda: ctx.index_grid(np.where(np.arange(6).reshape(2, 3) == 4, np.nan, rlp), 2.0, 10.0, 16), "rlp", "not finite")
    refused(ffs, lambda: ctx.index_peaks(15.0), "no grid is resident")   # (a refused call leaves none)
    grid = np.zeros(16 ** 3)
    grid[5] = np.inf
    refused(ffs, lambda: ctx.index_load_grid(grid, 16), "power", "not finite")
    ctx.index_grid(rlp, 2.0, 10.0, 16)
    for bad in (-1.0, np.inf, np.nan):
        refused(ffs, lambda: ctx.index_peaks(bad), "rmsd_cutoff")
    import ctypes as C
    lib = ffs.load_library()
    n = C.c_uint32(77)
    assert lib.ffs_ctx_index_peaks(ctx._h, 15.0, None, 3, C.byref(n), None, None) == -1 and n.value == 77
    assert b"NULL" in lib.ffs_last_error(ctx._h)
    assert lib.ffs_ctx_index_grid(ctx._h, None, 2, 2.0, 10.0, 16, None, None, None) == -1 and b"NULL" in lib.ffs_last_error(ctx._h)
    assert lib.ffs_ctx_index_load_grid(ctx._h, None, 16) == -1 and b"NULL" in lib.ffs_last_error(ctx._h)
    peaks, _ = ctx.index_peaks(15.0)   # the refused calls changed nothing: the grid of the last good call is still resident
    want, _ = O.peaks(O.power_grid(O.dedup(*O.map_spots(rlp, 2.0, 10.0, 16)), 16), 16, 15.0)
    assert peaks.tobytes() == want.tobytes()
