"""GPU: the peak search of ffs_ctx_index_peaks (selection, union-find over the sorted list, per-root sums, compaction; kernels_index.hpp) on
power grids built to break it, loaded with ffs_ctx_index_load_grid at n_points 16 and 32 and held to tests/index_oracle.py bit for bit:
components across each of the six faces and across all eight corners, two pieces that touch only through the wrap, a one-voxel-wide snake
through the whole grid, a component across the seams of the selection's workgroups (4096 voxels) and of the list passes (256 entries),
diagonal neighbours that must stay apart, an all-equal grid, a cutoff above the maximum, cap below the count, and a component that reaches
exactly N/2 - 1 from its root."""
import numpy as np
import pytest

import index_cases as K
import index_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (16, 32)


SHAPES = K.SHAPES
faces, diagonals = K.SHAPES["faces"], K.SHAPES["diagonals"]
_oracle = {}


def expected(name, n, rmsd_cutoff=1.0):
    if (name, n, rmsd_cutoff) not in _oracle:
        _oracle[(name, n, rmsd_cutoff)] = O.peaks(SHAPES[name](n).reshape(-1), n, rmsd_cutoff)
    return _oracle[(name, n, rmsd_cutoff)]


@pytest.fixture(scope="module")
def ctx(ffs):
    return ffs.Context(64, 48, np.uint16, max_batch=1)


def stats_bytes(stats):
    st = np.zeros((), O.STATS_DT)
    for k in O.STATS_DT.names:
        st[k] = stats[k]
    return st.tobytes()


def assert_peaks(got, stats, want, want_stats, what):
    assert stats_bytes(stats) == want_stats.tobytes(), (what, stats, want_stats)
    if got.tobytes() != want.tobytes():
        assert len(got) == len(want), (what, len(got), len(want))
        for k in O.PEAK_DT.names:
            bad = np.flatnonzero(np.any(np.atleast_2d((got[k] != want[k]).T), axis=0))
            assert len(bad) == 0, (what, k, bad[:5], got[bad[:3]], want[bad[:3]])
        raise AssertionError(str(what) + ": the bytes differ where no field does")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_peaks_of_a_built_grid_equal_the_oracles(ffs, ctx, name, n):
    want, want_stats = expected(name, n)
    ctx.index_load_grid(SHAPES[name](n), n)
    got, stats = ctx.index_peaks(1.0)
    assert_peaks(got, stats, want, want_stats, (name, n))
    grid = SHAPES[name](n)
    assert stats["n_selected"] == np.count_nonzero(grid)
    if name == "faces":
        assert len(got) == 6 and np.all(got["n_voxels"] == 4)
    if name == "corners":
        assert len(got) == 2 and got["n_voxels"][0] == 8 and got["root"][0] == 0 and np.all(got["sum"][0] == -4)
    if name == "through_the_wrap":
        assert sorted(got["n_voxels"]) == [1, 2, 5, 5]
    if name == "snake":
        assert len(got) == 1 and got["n_voxels"][0] > n ** 3 // 5
    if name == "seams":
        assert len(got) == 1 and (n == 16 or got["n_voxels"][0] > 2 * 256)
    if name == "diagonals":
        assert len(got) == 2 * n
    if name == "reach":
        assert len(got) == 1
        c = np.argwhere(grid > 0)
        root = np.array(np.unravel_index(got["root"][0], (n, n, n)))
        d = (c - root + n // 2) % n - n // 2
        assert d.max() == n // 2 - 1 and d.min() == -(n // 2)


@pytest.mark.parametrize("n", SIZES)
def test_an_all_equal_grid_is_one_component_of_every_voxel(ffs, ctx, n):
    grid = np.full(n ** 3, 3.5)
    ctx.index_load_grid(grid, n)
    got, stats = ctx.index_peaks(O.RMSD_CUTOFF)
    want, want_stats = O.peaks(grid, n, O.RMSD_CUTOFF)
    assert_peaks(got, stats, want, want_stats, ("all equal", n))
    assert stats["rmsd"] == 0.0 and stats["cutoff"] == 0.0 and stats["mean"] == 3.5 and stats["n_selected"] == n ** 3
    assert len(got) == 1 and got["root"][0] == 0 and got["n_voxels"][0] == n ** 3 and np.all(got["sum"][0] == -(n // 2) * n ** 2)


def test_a_cutoff_above_the_maximum_gives_no_peak(ffs, ctx):
    ctx.index_load_grid(faces(16), 16)
    got, stats = ctx.index_peaks(1.0e6)
    assert len(got) == 0 and stats["n_selected"] == 0 and stats["n_peaks"] == 0 and stats["cutoff"] > 1.0
    import ctypes as C
    lib = ffs.load_library()
    n = C.c_uint32(77)
    assert lib.ffs_ctx_index_peaks(ctx._h, 1.0e6, None, 0, C.byref(n), None, None) == 0 and n.value == 0


def test_a_cap_below_the_count_gives_the_first_records_and_the_full_count(ffs, ctx):
    want, want_stats = expected("diagonals", 32)
    ctx.index_load_grid(diagonals(32), 32)
    for cap in (1, 5, len(want) - 1):
        with pytest.raises(ffs.FfsError) as e:
            ctx.index_peaks(1.0, cap=cap)
        assert e.value.code == -4 and e.value.n == len(want) and stats_bytes(e.value.stats) == want_stats.tobytes()
        assert e.value.records.tobytes() == want[:cap].tobytes(), cap
    got, _ = ctx.index_peaks(1.0, cap=len(want) + 100)
    assert got.tobytes() == want.tobytes()
