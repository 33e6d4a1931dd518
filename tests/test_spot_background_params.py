"""CPU: the per-spot background's ABI and binding (ffs_stream_spot_backgrounds, ffs_spot_background), spot_intensities, and the driver's
--spot-background with its refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HEADER = os.path.join(ROOT, "include", "ffs_hip.h")
FIELDS = ["n_pixels", "n_overflow", "q1", "median", "q3", "n_inliers", "inlier_sum", "status", "reserved", "mean"]


def test_header_declares_the_entry_and_the_struct():
    src = open(HEADER).read()
    assert re.search(r"\bint\s+ffs_stream_spot_backgrounds\s*\(\s*ffs_stream\s*\*\s*s\s*,\s*uint32_t\s+border\s*,\s*const\s+ffs_spot_background\s*\*\*\s*out\s*,"
                     r"\s*uint32_t\s*\*\s*n\s*,\s*float\s*\*\s*kernel_ms\s*\)\s*;", src)
    body = src[src.index("typedef struct {\n    uint32_t n_pixels, n_overflow;"):]
    body = body[:body.index("} ffs_spot_background;")]
    assert re.findall(r"(\w+)\s*[,;]", body) == FIELDS
    assert re.search(r"uint32_t\s+n_pixels,\s*n_overflow;\s*int32_t\s+q1,\s*median,\s*q3;\s*uint32_t\s+n_inliers;\s*uint64_t\s+inlier_sum;\s*uint32_t\s+status,\s*reserved;\s*double\s+mean;", body)
    for name, value in (("OK", 0), ("NO_PIXELS", 1), ("OVERFLOW", 2), ("RANGE", 3), ("NO_INLIERS", 4)):
        assert re.search(r"#define\s+FFS_SPOT_BG_%s\s+%du\b" % (name, value), src)
    comment = src[:src.index("#define FFS_SPOT_BG_OK")]
    comment = comment[comment.rindex("/*"):]
    for what in ("1..16", "OUTSIDE the bounding box", "max_valid", "2^24", "(N + 3) / 4", "(N + 1) / 2", "(3 N + 1) / 4", "2 * q3 + 3 * iqr >= 512",
                 "2 * q1 - 3 * iqr <= 2 * p", "4 * n_overflow > N", "want_reflections", "in flight", "ffs_submit_device", "mask must not have been replaced",
                 "Cannot be reached", "ffs_stream_batch_arrays", "kernel_ms may be NULL"):
        assert what in comment, what


def test_struct_is_48_bytes_and_the_binding_matches():
    from ffs_amd import api
    assert C.sizeof(api._SpotBackground) == 48 and api.SPOT_BG_DT.itemsize == 48
    assert [f for f, _ in api._SpotBackground._fields_] == FIELDS and list(api.SPOT_BG_DT.names) == FIELDS
    for f in FIELDS:
        assert getattr(api._SpotBackground, f).offset == api.SPOT_BG_DT.fields[f][1], f
    assert api._SpotBackground.inlier_sum.offset == 24 and api._SpotBackground.mean.offset == 40
    assert (api.SPOT_BG_OK, api.SPOT_BG_NO_PIXELS, api.SPOT_BG_OVERFLOW, api.SPOT_BG_RANGE, api.SPOT_BG_NO_INLIERS) == (0, 1, 2, 3, 4)


def test_library_exports_the_entry_and_refuses_null():
    from ffs_amd import api
    lib = api.load_library()
    assert hasattr(lib, "ffs_stream_spot_backgrounds") and "ffs_stream_spot_backgrounds" in api.EXPORTS
    assert lib.ffs_stream_spot_backgrounds.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    p, n = C.c_void_p(), C.c_uint32(7)
    assert lib.ffs_stream_spot_backgrounds(None, 3, C.byref(p), C.byref(n), None) != 0      # (no stream: refused, not a crash)
    assert lib.ffs_stream_spot_backgrounds(None, 3, None, None, None) != 0
    assert b"ffs_stream_spot_backgrounds" in lib.ffs_last_error(None)
    assert callable(api.Stream.spot_backgrounds) and callable(api.spot_intensities)


def test_spot_intensities():
    import ffs_amd
    from ffs_amd import api
    refl = np.zeros(4, api.REFL_DT)
    refl["sum_intensity"] = [9000, 500, (1 << 40) + 3, 7]
    refl["num_pixels"] = [9, 4, 100, 3]
    bg = np.zeros(4, api.SPOT_BG_DT)
    bg["status"] = [0, 2, 0, 3]
    bg["n_inliers"] = [54, 0, 7, 0]
    bg["inlier_sum"] = [108, 0, 22, 0]
    bg["mean"] = [2.0, 0.0, 22 / 7, 0.0]
    intensity, variance = ffs_amd.spot_intensities(refl, bg)
    assert intensity.dtype == variance.dtype == np.float64
    assert intensity[0] == 9000 - 9 * 2.0 and variance[0] == 9000 + 81 * 2.0 / 54
    assert intensity[2] == float((1 << 40) + 3) - 100.0 * (22 / 7) and variance[2] == float((1 << 40) + 3) + 100.0 * 100.0 * (22 / 7) / 7.0
    assert np.isnan(intensity[[1, 3]]).all() and np.isnan(variance[[1, 3]]).all()
    e = ffs_amd.spot_intensities(refl[:0], bg[:0])
    assert len(e[0]) == len(e[1]) == 0


def _cli(*argv):
    return subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True, timeout=60)


def test_help_lists_spot_background():
    r = _cli("--help")
    assert r.returncode == 0
    assert "\n                  [--spot-background B]\n" in r.stdout and "\n--spot-background:" in r.stdout
    for key in ('"spot_background_mean"', '"spot_intensity"', '"spot_variance"', '"total_intensity"'):
        assert key in r.stdout, key


@pytest.mark.parametrize("argv,message", [
    (["--spot-background", "0"], "--spot-background takes a border in 1..16: 0"),
    (["--spot-background", "17"], "--spot-background takes a border in 1..16: 17"),
    (["--spot-background", "x"], "pattern not found for '--spot-background': x"),
    (["--spot-background", "-3"], "pattern not found for '--spot-background': -3"),
    (["--spot-background"], "Too few arguments for '--spot-background'")])
def test_bad_spot_background_is_refused_with_usage(argv, message):
    r = _cli("synth:tiny:1", *argv)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout and "Usage: spotfinder" in r.stdout, r.stdout
