"""CPU: the ABI and binding of the robust GLM background (ffs_stream_spot_backgrounds_glm, ffs_spot_background_glm), spot_intensities_glm,
`ffs_hosttool spotbgglm`, and the driver's --spot-background-model with its refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SPOTFINDER = os.path.join(BIN, "spotfinder")
HOSTTOOL = os.path.join(BIN, "ffs_hosttool")
HEADER = os.path.join(ROOT, "include", "ffs_hip.h")
FIELDS = ["n_pixels", "n_overflow", "median", "n_iter", "status", "reserved", "beta", "mean"]


def test_header_declares_the_entry_the_struct_and_the_rule():
    src = open(HEADER).read()
    assert re.search(r"\bint\s+ffs_stream_spot_backgrounds_glm\s*\(\s*ffs_stream\s*\*\s*s\s*,\s*uint32_t\s+border\s*,\s*const\s+ffs_spot_background_glm\s*\*\*\s*out\s*,"
                     r"\s*uint32_t\s*\*\s*n\s*,\s*float\s*\*\s*kernel_ms\s*\)\s*;", src)
    body = src[:src.index("} ffs_spot_background_glm;")]
    body = body[body.rindex("typedef struct {"):]
    assert re.findall(r"(\w+)\s*[,;]", body) == FIELDS
    assert re.search(r"uint32_t\s+n_pixels,\s*n_overflow;\s*int32_t\s+median;\s*uint32_t\s+n_iter;\s*uint32_t\s+status,\s*reserved;\s*double\s+beta,\s*mean;", body)
    for name, value in (("FEW_PIXELS", 5), ("DEGENERATE", 6), ("NOT_CONVERGED", 7)):
        assert re.search(r"#define\s+FFS_SPOT_BG_%s\s+%du\b" % (name, value), src)
    comment = src[:src.index("#define FFS_SPOT_BG_FEW_PIXELS")]
    comment = comment[comment.rindex("/*"):]
    for what in ("N < 10", "4 * n_overflow > N", "N / 2 + 1", "ALL-ZERO RING", "beta = -inf", "1.345", "100 steps", "1e-3", "mu not < 512", "(-300, 300)",
                 "psi = +c", "median is -1 under status 1, 2 and 5", "mean / N", "want_reflections", "in flight", "kernel_ms may be NULL", "bit for bit"):
        assert what in comment, what


def test_struct_is_40_bytes_and_the_binding_matches():
    from ffs_amd import api
    assert C.sizeof(api._SpotBackgroundGlm) == 40 and api.SPOT_BG_GLM_DT.itemsize == 40
    assert [f for f, _ in api._SpotBackgroundGlm._fields_] == FIELDS and list(api.SPOT_BG_GLM_DT.names) == FIELDS
    for f in FIELDS:
        assert getattr(api._SpotBackgroundGlm, f).offset == api.SPOT_BG_GLM_DT.fields[f][1], f
    assert api._SpotBackgroundGlm.median.offset == 8 and api._SpotBackgroundGlm.status.offset == 16
    assert api._SpotBackgroundGlm.beta.offset == 24 and api._SpotBackgroundGlm.mean.offset == 32
    assert (api.SPOT_BG_FEW_PIXELS, api.SPOT_BG_DEGENERATE, api.SPOT_BG_NOT_CONVERGED) == (5, 6, 7)
    import spot_background_glm_oracle as G
    assert G.DT == api.SPOT_BG_GLM_DT


def test_library_exports_the_entry_and_refuses_null():
    import ffs_amd
    from ffs_amd import api
    lib = api.load_library()
    assert hasattr(lib, "ffs_stream_spot_backgrounds_glm") and "ffs_stream_spot_backgrounds_glm" in api.EXPORTS
    assert lib.ffs_stream_spot_backgrounds_glm.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    p, n = C.c_void_p(), C.c_uint32(7)
    assert lib.ffs_stream_spot_backgrounds_glm(None, 3, C.byref(p), C.byref(n), None) != 0      # (no stream: refused, not a crash)
    assert b"ffs_stream_spot_backgrounds_glm" in lib.ffs_last_error(None)
    assert callable(api.Stream.spot_backgrounds_glm) and callable(ffs_amd.spot_intensities_glm) and ffs_amd.SPOT_BG_GLM_DT is api.SPOT_BG_GLM_DT


def test_spot_intensities_glm():
    import ffs_amd
    from ffs_amd import api
    refl = np.zeros(4, api.REFL_DT)
    refl["sum_intensity"] = [9000, 500, (1 << 40) + 3, 7]
    refl["num_pixels"] = [9, 4, 100, 3]
    bg = np.zeros(4, api.SPOT_BG_GLM_DT)
    bg["status"] = [0, 5, 0, 7]
    bg["n_pixels"] = [72, 9, 7, 100]
    bg["mean"] = [2.5, 0.0, 22 / 7, 0.0]
    intensity, variance = ffs_amd.spot_intensities_glm(refl, bg)
    assert intensity.dtype == variance.dtype == np.float64
    assert intensity[0] == 9000 - 9 * 2.5 and variance[0] == 9000 + 81 * 2.5 / 72
    assert intensity[2] == float((1 << 40) + 3) - 100.0 * (22 / 7) and variance[2] == float((1 << 40) + 3) + 100.0 * 100.0 * (22 / 7) / 7.0
    assert np.isnan(intensity[[1, 3]]).all() and np.isnan(variance[[1, 3]]).all()
    e = ffs_amd.spot_intensities_glm(refl[:0], bg[:0])
    assert len(e[0]) == len(e[1]) == 0


def test_hosttool_spotbgglm_reads_a_file_and_standard_input(tmp_path):
    """One record a line, the doubles as 16 hex digits; an all-zero ring, a ring of 9, a one-bin ring whose mean is near its bin."""
    import struct
    hists = [[72] + [0] * 256, [9] + [0] * 256, [0] * 7 + [64] + [0] * 249]
    text = "".join(" ".join(str(c) for c in h) + "\n" for h in hists)
    by_stdin = subprocess.run([HOSTTOOL, "spotbgglm"], input=text, capture_output=True, text=True, timeout=60)
    path = tmp_path / "hists.txt"
    path.write_text(text)
    by_file = subprocess.run([HOSTTOOL, "spotbgglm", str(path)], capture_output=True, text=True, timeout=60)
    assert by_stdin.returncode == by_file.returncode == 0 and by_stdin.stdout == by_file.stdout
    lines = by_stdin.stdout.splitlines()
    assert lines[0] == "72 0 0 0 0 fff0000000000000 0000000000000000"
    assert lines[1] == "9 0 -1 0 5 0000000000000000 0000000000000000"
    t = lines[2].split()
    assert t[:3] == ["64", "0", "7"] and t[4] == "0" and len(t[5]) == len(t[6]) == 16
    assert 6.9 < struct.unpack("<d", struct.pack("<Q", int(t[6], 16)))[0] < 7.2
    short = subprocess.run([HOSTTOOL, "spotbgglm"], input="1 2 3\n", capture_output=True, text=True, timeout=60)
    assert short.returncode == 2 and "short" in short.stderr


def _cli(*argv):
    return subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True, timeout=60)


def test_help_lists_the_model():
    r = _cli("--help")
    assert r.returncode == 0
    assert "\n                  [--spot-background-model constant|glm]\n" in r.stdout and "\n--spot-background-model:" in r.stdout
    assert "robust Poisson GLM" in r.stdout and "Needs --spot-background" in r.stdout


@pytest.mark.parametrize("argv,message", [
    (["--spot-background-model", "glm"], "--spot-background-model belongs to --spot-background"),
    (["--spot-background-model", "constant"], "--spot-background-model belongs to --spot-background"),
    (["--spot-background", "3", "--spot-background-model", "tukey"], "--spot-background-model takes constant or glm: tukey"),
    (["--spot-background", "3", "--spot-background-model", ""], "--spot-background-model takes constant or glm: "),
    (["--spot-background", "3", "--spot-background-model"], "Too few arguments for '--spot-background-model'")])
def test_bad_model_is_refused_with_usage(argv, message):
    r = _cli("synth:tiny:1", *argv)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout and "Usage: spotfinder" in r.stdout, r.stdout
