"""CPU: the declarations of index assignment in include/ffs_hip.h and their mirror in the Python binding; the host-only entries
(ffs_index_select / settings / absence_table / absence_detect / reindex) through ctypes against tests/assign_oracle.py, bit for bit, and their
refusals; the device entries refused without a context, not a crash."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import assign_cases as AC
import assign_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ffs_hip.h")).read()
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
ENTRIES = ("ffs_index_select", "ffs_index_settings", "ffs_index_absence_table", "ffs_index_absence_detect", "ffs_index_reindex", "ffs_ctx_index_assign",
           "ffs_ctx_index_assign_launch_ms")


def test_the_header_declares_the_entries_and_cites_what_they_replace():
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", HEADER), name
    for text in ("ffs_index_assignment;           /* 472 bytes */", "ffs_index_absence_test;         /* 56 bytes */", "ffs_index_setting;              /* 160 bytes */",
                 "#define FFS_INDEX_ABSENCE_TESTS 111", "#define FFS_INDEX_ASSIGN_SINGULAR 1u", "assign_indices.cc:56-165", "non_primitive_basis.cc", "indexer.cc:266-276",
                 "combinations.cc", "DESIGN.md section 3.8f", "csrc/assign_model.hpp", "No fit, no refinement, no Niggli reduction", "FFS_ERR_NOMEM", "#define FFS_INDEX_LAUNCH_SPANS 9"):
        assert text in HEADER, text


def test_the_model_header_states_the_rule_and_the_plan_the_bytes():
    model = open(os.path.join(CSRC, "assign_model.hpp")).read()
    for text in ("assign_indices.cc:56-165", "non_primitive_basis.cc:25-34", "indexer.cc:266-276", "combinations.cc", "THIS TEXT IS THE CONTRACT", "524288.0", "1099511627776.0",
                 "a tie kills the later spot", "niggli_reduce() after it is NOT restated", "ON THE CELL AS BUILT", "An rlp of\n//       zero"):
        assert text in model, text
    kernels = open(os.path.join(CSRC, "kernels_assign.hpp")).read()
    for name in ("assign_model.hpp", "assign_plan.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/hip_runtime" not in text and "__global__" not in text and "-ffp-contract=off" in model
    assert "#include \"assign_model.hpp\"" in kernels and "atomicAdd((float" not in kernels and "atomicAdd((double" not in kernels
    others = [f for f in os.listdir(CSRC) if f.startswith("kernels_") and f != "kernels_assign.hpp"]
    assert others and all("assign_" not in open(os.path.join(CSRC, f)).read() for f in others), "no existing kernel includes the new headers"
    assert "ffs_assign.hip" in open(os.path.join(CSRC, "ffs_internal.hpp")).read()


def test_the_binding_mirrors_the_header(ffs):
    from ffs_amd import api
    lib = ffs.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in api.EXPORTS
    assert ffs.INDEX_ASSIGNMENT_DT == AO.ASSIGNMENT_DT and ffs.INDEX_ABSENCE_TEST_DT == AO.ABSENCE_TEST_DT and ffs.INDEX_SETTING_DT == AO.SETTING_DT
    assert (ffs.INDEX_ABSENCE_TESTS, ffs.INDEX_ASSIGN_SINGULAR, ffs.INDEX_ASSIGN_TOLERANCE, ffs.INDEX_ABSENCE_THRESHOLD, ffs.INDEX_MAX_COMBINATIONS) == (111, 1, 0.3, 0.9, 1000)
    assert len(ffs.INDEX_ASSIGN_LAUNCH_SPANS) == 3
    for name in ("index_assign", "index_correct"):
        assert callable(getattr(ffs.Context, name))


def test_the_host_only_entries_equal_the_oracle(ffs):
    assert ffs.index_absence_table().tobytes() == AO.table().tobytes()
    for name in ("small-disturbed", "triclinic-disturbed"):
        c = AC.lattice(name, 200 if name.startswith("tri") else None)
        s = ffs.index_settings(c["vectors"])
        assert s.tobytes() == AO.settings(c["vectors"]["v"]).tobytes() and len(s) >= 200, name
        assert ffs.index_settings(c["vectors"]["v"], 50).tobytes() == AO.settings(c["vectors"]["v"], 50).tobytes()
        for dmin, osc in ((1.5, 0.0), (2.5, -330.0), (0.0, 0.0)):
            got = ffs.index_select(c["rlp"], c["phi"], dmin, osc)
            assert got.astype(np.uint8).tobytes() == AO.select(c["rlp"], c["phi"], dmin, osc).tobytes() and (dmin == 0.0 or 0 < got.sum() < len(got)), (name, dmin, osc)
        recs = AC.expected(c)[0]
        for k in (0, 1, c["n_own"], c["n_own"] + 1, c["n_own"] + 2):
            t = ffs.index_absence_detect(recs[k])
            assert t == AO.detect(recs[k])
            for test in {max(t, 0), 5, 110}:
                assert ffs.index_reindex(c["A"][k], test).tobytes() == AO.reindex(c["A"][k], test).tobytes()
        for threshold in (0.0, 0.5, 0.99, 1.0):
            assert ffs.index_absence_detect(recs[c["n_own"] + 1], threshold) == AO.detect(recs[c["n_own"] + 1], threshold)
    assert ffs.index_select([[0.0, 0.0, 0.0]], [0.0], 2.0).tolist() == [True]   # an rlp of zero is selected (and never accepted)
    assert len(ffs.index_settings(np.zeros((0, 3)))) == 0 and len(ffs.index_settings(np.eye(3)[:2])) == 0
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "index_assign_reference_cases.json")))["combinations"]
    assert len(ffs.index_settings(golden["vectors"], golden["max_combinations"])) == 2
    lib = ffs.load_library()
    v, out, n = np.ascontiguousarray(AC.lattice("small-disturbed")["vectors"]["v"]), np.zeros(2, AO.SETTING_DT), C.c_uint32()
    rc = lib.ffs_index_settings(v.ctypes.data_as(C.c_void_p), len(v), 1000, out.ctypes.data_as(C.c_void_p), 2, C.byref(n))
    assert rc == -4 and n.value == AC.lattice("small-disturbed")["n_own"] and out.tobytes() == AO.settings(v)[:2].tobytes()


def refused(ffs, call, *needles):
    with pytest.raises(ffs.FfsError) as e:
        call()
    assert e.value.code == -1 and all(n in str(e.value) for n in needles), str(e.value)


def test_what_the_host_only_entries_refuse(ffs):
    rlp, phi, A = np.array([[0.1, 0.02, -0.03]]), np.array([0.5]), np.eye(3).reshape(9)
    for bad in (-1.0, np.inf, np.nan):
        refused(ffs, lambda: ffs.index_select(rlp, phi, bad), "ffs_index_select", "dmin")
    refused(ffs, lambda: ffs.index_select(rlp, phi, 2.0, np.nan), "osc_start_deg")
    refused(ffs, lambda: ffs.index_select([[np.nan, 0, 0]], phi, 2.0), "rlp", "not finite")
    refused(ffs, lambda: ffs.index_select(rlp, [np.inf], 2.0), "phi", "not finite")
    refused(ffs, lambda: ffs.index_settings([[1.0, np.nan, 0.0]]), "ffs_index_settings", "vectors", "not finite")
    refused(ffs, lambda: ffs.index_settings(np.eye(3), 0), "max_combinations must be positive")
    rec = np.zeros((), AO.ASSIGNMENT_DT)
    for bad in (-0.1, 1.1, np.nan):
        refused(ffs, lambda: ffs.index_absence_detect(rec, bad), "ffs_index_absence_detect", "threshold must be in [0, 1]")
    for bad in (-1, 111):
        refused(ffs, lambda: ffs.index_reindex(A, bad), "ffs_index_reindex", "test must be in 0 .. 110")
    refused(ffs, lambda: ffs.index_reindex(A * np.nan, 0), "A has an entry that is not finite")
    refused(ffs, lambda: ffs.index_reindex(np.zeros(9), 0), "A is singular")
    lib = ffs.load_library()
    t = C.c_int32(7)
    assert lib.ffs_index_select(None, None, 1, 2.0, 0.0, None) == -1 and b"NULL" in lib.ffs_last_error(None)
    assert lib.ffs_index_settings(None, 3, 1000, None, 0, None) == -1 and b"NULL" in lib.ffs_last_error(None)
    assert lib.ffs_index_absence_table(None) == -1 and b"NULL" in lib.ffs_last_error(None)
    assert lib.ffs_index_absence_detect(None, 0.9, C.byref(t)) == -1 and t.value == 7 and b"NULL" in lib.ffs_last_error(None)
    assert lib.ffs_index_reindex(None, 0, None) == -1 and b"NULL" in lib.ffs_last_error(None)


def test_the_device_entries_without_a_context_are_refused_not_a_crash(ffs):
    lib = ffs.load_library()
    assert lib.ffs_ctx_index_assign(None, None, None, None, 0, None, 0, 0.3, 0, None, None, None) == -1
    assert lib.ffs_ctx_index_assign_launch_ms(None, None) == -1
