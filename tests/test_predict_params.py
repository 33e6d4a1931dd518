"""CPU: the ABI of scan prediction -- the header's structs, constants and comments, the Python binding's mirrors (ffs_crystal 80 bytes,
ffs_prediction 96), the library's exports, and the one entry that needs no GPU: ffs_predict_scan_settings against NumPy's Rodrigues
matrices and its refusals.  ffs_ctx_predict without a context is refused, not a crash."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import predict_cases as K
import predict_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ffs_hip.h")


def test_the_header_declares_the_structs_constants_and_rule():
    src = open(HEADER).read()
    for name, value in (("P", 0), ("I", 1), ("F", 2), ("A", 3), ("B", 4), ("C", 5), ("R", 6)):
        assert re.search(r"#define\s+FFS_CENTRING_%s\s+%d\b" % (name, value), src)
    for name, value in (("ENTERING", 1), ("CORNER_LOST", 2), ("ZETA_SMALL", 4), ("BOX_REFUSED", 8)):
        assert re.search(r"#define\s+FFS_PREDICT_%s\s+%du\b" % (name, value), src)
    assert re.search(r"typedef struct \{\s*double a_matrix\[9\];[^}]*int32_t centring, reserved;\s*\} ffs_crystal;", src)
    assert re.search(r"typedef struct \{\s*ffs_shoebox box;[^}]*double x_px, y_px, z;[^}]*int32_t h, k, l;\s*uint32_t flags;[^}]*\} ffs_prediction;", src)
    assert re.search(r"int ffs_predict_scan_settings\(const ffs_scan_geometry \*\w+, const ffs_crystal \*\w+, uint32_t n_images, double \*out\);", src)
    assert re.search(r"int ffs_ctx_predict\(ffs_ctx \*\w+, const ffs_scan_geometry \*\w+, const ffs_crystal \*\w+, uint32_t n_images, double dmin,\s*double delta_b, "
                     r"double delta_m, ffs_prediction \*out, uint32_t cap, uint32_t \*n, float \*kernel_ms\);", src)
    comment = src[src.index("/* Scan prediction for a rotation sweep"):src.index("int ffs_ctx_predict(")]
    for what in ("predict.cc:31-128", "ray_predictors.cc:115-201", "extent.cc:14-198", "csrc/predict_model.hpp", "no trigonometric function", "Rodrigues",
                 "floor(|real-space axis| / dmin) + 1", "h slowest, l fastest", "squared norms", "1e-10", "candidate number, then image", "FFS_ERR_OVERFLOW",
                 "cap 0 with out NULL", "65 535", "2^31 - 1", "in flight"):
        assert what in comment, what


def test_the_binding_mirrors_the_structs():
    import ffs_amd
    from ffs_amd import api
    assert C.sizeof(api._Crystal) == 80 and api._Crystal.centring.offset == 72
    assert api.PREDICTION_DT.itemsize == 96 and api.PREDICTION_DT == O.PREDICTION_DT
    assert list(api.PREDICTION_DT.names[:len(api.SHOEBOX_DT.names)]) == list(api.SHOEBOX_DT.names)
    for name in api.SHOEBOX_DT.names:
        assert api.PREDICTION_DT.fields[name][1] == api.SHOEBOX_DT.fields[name][1], name
    assert [api.PREDICTION_DT.fields[n][1] for n in ("x_px", "y_px", "z", "h", "k", "l", "flags")] == [56, 64, 72, 80, 84, 88, 92]
    assert api.CENTRINGS == O.CENTRINGS == dict(zip("PIFABCR", range(7)))
    assert (api.PREDICT_ENTERING, api.PREDICT_CORNER_LOST, api.PREDICT_ZETA_SMALL, api.PREDICT_BOX_REFUSED) == (O.ENTERING, O.CORNER_LOST, O.ZETA_SMALL, O.BOX_REFUSED)
    assert callable(api.Context.predict) and ffs_amd.predict_scan_settings is api.predict_scan_settings and ffs_amd.shoeboxes_of is api.shoeboxes_of
    p = np.zeros(3, api.PREDICTION_DT)
    p["flags"] = [0, 8, 1]
    p["x_max"] = [5, 6, 7]
    assert list(ffs_amd.shoeboxes_of(p)["x_max"]) == [5, 7] and list(ffs_amd.shoeboxes_of(p, skip_refused=False)["x_max"]) == [5, 6, 7]
    assert ffs_amd.shoeboxes_of(p).dtype == api.SHOEBOX_DT


def test_the_library_exports_the_entries_and_refuses_null():
    from ffs_amd import api
    lib = api.load_library()
    for name in ("ffs_predict_scan_settings", "ffs_ctx_predict"):
        assert hasattr(lib, name) and name in api.EXPORTS
    n = C.c_uint32(7)
    assert lib.ffs_ctx_predict(None, None, None, 16, 2.0, 0.01, 0.004, None, 0, C.byref(n), None) == -1 and n.value == 7   # (no context: refused, not a crash)
    out = np.zeros(9 * 3)
    assert lib.ffs_predict_scan_settings(None, None, 2, out.ctypes.data_as(C.c_void_p)) == -1
    assert b"ffs_predict_scan_settings" in lib.ffs_last_error(None) and b"NULL" in lib.ffs_last_error(None)


def test_the_scan_settings_of_the_library_are_the_rodrigues_matrices():
    import ffs_amd
    worst = 0.0
    for c in K.cases():
        got = ffs_amd.predict_scan_settings(c["g"], c["A"], c["n_images"])
        assert got.shape == (c["n_images"] + 1, 9)
        worst = max(worst, float(np.max(np.abs(got - O.rodrigues_settings(c["g"], c["A"], c["n_images"])))))
    assert worst <= 2 * 2.78e-17   # (the bound of tests/test_predict_oracle.py, measured there)
    g = K.MAIN["g"]
    for bad, needle in ((dict(g, rot_axis=[0.0, 0.0, 0.0]), "rot_axis"), (dict(g, osc_start_deg=np.nan), "not finite")):
        with pytest.raises(ffs_amd.FfsError) as e:
            ffs_amd.predict_scan_settings(bad, K.MAIN["A"], 4)
        assert e.value.code == -1 and needle in str(e.value)
    for n in (0, 65536):
        with pytest.raises(ffs_amd.FfsError) as e:
            ffs_amd.predict_scan_settings(g, K.MAIN["A"], n)
        assert "n_images" in str(e.value)
