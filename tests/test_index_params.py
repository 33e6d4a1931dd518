"""CPU: the declarations of the indexer's basis-vector search in include/ffs_hip.h and their mirror in the Python binding; the host-only
entries (ffs_index_rlp / defaults / twiddles / map / basis_vectors) through ctypes against tests/index_oracle.py, bit for bit, and their
refusals; the device entries refused without a context, not a crash."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import index_cases as K
import index_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ffs_hip.h")).read()
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
ENTRIES = ("ffs_index_rlp", "ffs_index_defaults", "ffs_index_twiddles", "ffs_index_map", "ffs_index_basis_vectors", "ffs_ctx_index_grid", "ffs_ctx_index_load_grid",
           "ffs_ctx_index_peaks", "ffs_ctx_index_launch_ms")


def test_the_header_declares_the_entries_and_cites_what_they_replace():
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", HEADER), name
    for text in ("ffs_index_peak;                 /* 56 bytes */", "ffs_index_grid_stats;           /* 40 bytes */", "ffs_index_vector;               /* 40 bytes */",
                 "indexer.cc:171-245", "xyz_to_rlp.cc:46-109", "fft3d.cc:37-91", "fft3d.cc:102-182", "flood_fill.cc:31-149", "flood_fill.cc:158-192", "peaks_to_rlvs.cc:74-186",
                 "DESIGN.md section 3.8e", "csrc/index_model.hpp", "highest spot number", "FFS_ERR_OVERFLOW"):
        assert text in HEADER, text


def test_the_model_header_states_the_rule_and_the_plan_the_bytes():
    model = open(os.path.join(CSRC, "index_model.hpp")).read()
    for text in ("xyz_to_rlp.cc:46-109", "indexer.cc:184-206", "fft3d.cc:37-91", "flood_fill.cc:38-49", "flood_fill.cc:59-147", "flood_fill.cc:158-192", "peaks_to_rlvs.cc:74-186",
                 "HIGHEST SPOT NUMBER", "radix 2", "decimation in time", "four products, one difference, one sum", "axis 0", "DEPARTURES", "THIS TEXT IS THE CONTRACT"):
        assert text in model, text
    assert "hip/hip_runtime" not in model and "__global__" not in model
    plan = open(os.path.join(CSRC, "index_plan.hpp")).read()
    assert "268 MB + 134 MB" in plan and "hip/hip_runtime" not in plan
    assert "ffs_index.hip" in open(os.path.join(CSRC, "ffs_internal.hpp")).read()


def test_the_binding_mirrors_the_header(ffs):
    from ffs_amd import api
    lib = ffs.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in api.EXPORTS
    assert ffs.INDEX_PEAK_DT == O.PEAK_DT and ffs.INDEX_VECTOR_DT == O.VECTOR_DT and C.sizeof(api._IndexGridStats) == O.STATS_DT.itemsize == 40
    assert [f for f, _ in api._IndexGridStats._fields_] == list(O.STATS_DT.names)
    assert (ffs.INDEX_RMSD_CUTOFF, ffs.INDEX_PEAK_VOLUME_CUTOFF, ffs.INDEX_MIN_CELL, ffs.INDEX_NOT_USED) == (15.0, 0.15, 3.0, O.NOT_USED)
    assert len(ffs.INDEX_LAUNCH_SPANS) == 9 and "#define FFS_INDEX_LAUNCH_SPANS 9" in HEADER
    for name in ("index_grid", "index_load_grid", "index_peaks", "index_basis", "index_launch_ms"):
        assert callable(getattr(ffs.Context, name))


@pytest.mark.parametrize("n_points", (16, 64, 256))
def test_the_host_only_entries_equal_the_oracle(ffs, n_points):
    assert ffs.index_twiddles(n_points).tobytes() == O.twiddles(n_points).tobytes()
    for c in K.cases():
        rlp, s1, mm = ffs.index_rlp(c["g"], c["xyz"])
        want = O.rlp(c["g"], c["xyz"])
        assert rlp.tobytes() == want[0].tobytes() and s1.tobytes() == want[1].tobytes() and mm.tobytes() == want[2].tobytes(), c["name"]
        dmin, b_iso = ffs.index_defaults(rlp, c["max_cell"], n_points, c["dmin"])
        assert (dmin, b_iso) == O.defaults(rlp, c["max_cell"], n_points, c["dmin"]), c["name"]
        cell, weight = ffs.index_map(rlp, dmin, b_iso, n_points)
        want_cell, want_weight = O.map_spots(rlp, dmin, b_iso, n_points)
        assert cell.tobytes() == want_cell.tobytes() and weight.tobytes() == want_weight.tobytes(), c["name"]
    cell, weight = ffs.index_map(np.array([[0.1, 0.0, 0.0], [0.0, 0.0, 0.0]]), 2.0, 0.0, n_points)
    assert np.all(weight == 1.0) and cell[1] == (n_points // 2) * (1 + n_points + n_points ** 2)   # b_iso 0: weight 1; the origin lies in the middle


def test_the_basis_vectors_entry_equals_the_oracle(ffs):
    c = K.by_name("orthogonal-disturbed")
    o = O.chain(c["g"], c["xyz"], c["max_cell"], 64)
    assert len(o["vectors"]) >= 3
    assert ffs.index_basis_vectors(o["peaks"], 64, o["dmin"], c["max_cell"]).tobytes() == o["vectors"].tobytes()
    for pvc, min_cell in ((0.0, 3.0), (0.5, 10.0), (0.15, 0.0)):
        assert ffs.index_basis_vectors(o["peaks"], 64, o["dmin"], c["max_cell"], pvc, min_cell).tobytes() == O.basis_vectors(o["peaks"], 64, o["dmin"], c["max_cell"], pvc, min_cell).tobytes()
    assert len(ffs.index_basis_vectors(np.zeros(0, O.PEAK_DT), 64, 2.0, 45.0)) == 0   # an empty peak list gives an empty result
    lib = ffs.load_library()
    out, n = np.zeros(2, O.VECTOR_DT), C.c_uint32()
    pk = np.ascontiguousarray(o["peaks"])
    rc = lib.ffs_index_basis_vectors(pk.ctypes.data_as(C.c_void_p), len(pk), 64, o["dmin"], 0.15, 3.0, c["max_cell"], out.ctypes.data_as(C.c_void_p), 2, C.byref(n))
    assert rc == -4 and n.value == len(o["vectors"]) and out.tobytes() == o["vectors"][:2].tobytes()


def refused(ffs, call, *needles):
    with pytest.raises(ffs.FfsError) as e:
        call()
    assert e.value.code == -1 and all(n in str(e.value) for n in needles), str(e.value)


def test_what_the_host_only_entries_refuse(ffs):
    g, xyz = K.geometry(), [[100.0, 200.0, 3.0]]
    rlp = np.array([[0.1, 0.02, -0.03]])
    refused(ffs, lambda: ffs.index_rlp(dict(g, wavelength=np.inf), xyz), "ffs_index_rlp", "not finite")
    refused(ffs, lambda: ffs.index_rlp(dict(g, wavelength=-1.0), xyz), "positive")
    refused(ffs, lambda: ffs.index_rlp(dict(g, pixel_size_mm=[0.1, 0.0]), xyz), "positive")
    refused(ffs, lambda: ffs.index_rlp(dict(g, rot_axis=[0.0, 0.0, 0.0]), xyz), "rot_axis must not be zero")
    refused(ffs, lambda: ffs.index_rlp(dict(g, d_matrix=np.array([1, 0, 0, 0, 1, 0, 1, 1, 0.0])), xyz), "d_matrix is singular")
    refused(ffs, lambda: ffs.index_rlp(g, [[np.nan, 1.0, 2.0]]), "xyz_px", "not finite")
    for n in (0, 8, 48, 512):
        refused(ffs, lambda: ffs.index_defaults(rlp, 45.0, n), "ffs_index_defaults", "n_points must be a power of two in 16 .. 256")
        refused(ffs, lambda: ffs.index_map(rlp, 2.0, 10.0, n), "ffs_index_map", "n_points")
        refused(ffs, lambda: ffs.index_twiddles(n), "ffs_index_twiddles", "n_points")
        refused(ffs, lambda: ffs.index_basis_vectors(np.zeros(0, O.PEAK_DT), n, 2.0, 45.0), "n_points")
    for bad in (0.0, -2.0, np.inf, np.nan):
        refused(ffs, lambda: ffs.index_defaults(rlp, bad, 64), "max_cell")
        refused(ffs, lambda: ffs.index_map(rlp, bad, 10.0, 64), "dmin")
        refused(ffs, lambda: ffs.index_basis_vectors(np.zeros(0, O.PEAK_DT), 64, bad, 45.0), "dmin")
        refused(ffs, lambda: ffs.index_basis_vectors(np.zeros(0, O.PEAK_DT), 64, 2.0, bad), "max_cell")
    refused(ffs, lambda: ffs.index_defaults(rlp, 45.0, 64, -1.0), "dmin")
    refused(ffs, lambda: ffs.index_defaults([[np.inf, 0, 0]], 45.0, 64), "rlp", "not finite")
    refused(ffs, lambda: ffs.index_map([[np.nan, 0, 0]], 2.0, 10.0, 64), "rlp", "not finite")
    refused(ffs, lambda: ffs.index_map(rlp, 2.0, np.inf, 64), "b_iso")
    pk = np.zeros(1, O.PEAK_DT)
    refused(ffs, lambda: ffs.index_basis_vectors(pk, 64, 2.0, 45.0), "peak 0 has no voxels")
    lib = ffs.load_library()
    assert lib.ffs_index_rlp(None, None, 0, None, None, None) == -1 and b"NULL" in lib.ffs_last_error(None)
    assert lib.ffs_index_twiddles(64, None) == -1 and b"NULL" in lib.ffs_last_error(None)
    assert lib.ffs_index_map(None, 1, 2.0, 10.0, 64, None, None) == -1 and b"NULL" in lib.ffs_last_error(None)
    assert lib.ffs_index_defaults(None, 0, 45.0, 64, None, None) == -1 and b"NULL" in lib.ffs_last_error(None)


def test_the_device_entries_without_a_context_are_refused_not_a_crash(ffs):
    lib = ffs.load_library()
    n = C.c_uint32(5)
    assert lib.ffs_ctx_index_grid(None, None, 0, 2.0, 10.0, 64, None, None, None) == -1
    assert lib.ffs_ctx_index_load_grid(None, None, 64) == -1
    assert lib.ffs_ctx_index_peaks(None, 15.0, None, 0, C.byref(n), None, None) == -1 and n.value == 5
    assert lib.ffs_ctx_index_launch_ms(None, None) == -1
