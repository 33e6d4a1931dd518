"""CPU: the detector gain (ffs_ctx_set_gain) -- its ABI and binding, and the driver's --gain with its refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HEADER = os.path.join(ROOT, "include", "ffs_hip.h")


def test_header_declares_the_setter():
    src = open(HEADER).read()
    assert re.search(r"\bint\s+ffs_ctx_set_gain\s*\(\s*ffs_ctx\s*\*\s*ctx\s*,\s*double\s+gain\s*\)\s*;", src)
    # (a setter, not a field: the layout of ffs_params is pinned by test_window_params.py)
    body = src[src.index("typedef struct {\n    int32_t min_count;"):]
    assert "gain" not in body[:body.index("} ffs_params;")]
    # what it stands for, and that the reference's kernels have no counterpart
    comment = src[:src.index("int ffs_ctx_set_gain")]
    comment = comment[comment.rindex("/*"):]
    assert "baseline.cpp" in comment and "dispersion.gain" in comment and "standalone.cc" in comment


def test_library_exports_the_setter_and_the_binding_knows_it():
    from ffs_amd import api
    lib = api.load_library()
    assert hasattr(lib, "ffs_ctx_set_gain")
    assert "ffs_ctx_set_gain" in api.EXPORTS
    assert lib.ffs_ctx_set_gain.argtypes == [C.c_void_p, C.c_double]
    assert lib.ffs_ctx_set_gain(None, 2.5) != 0   # (no context: refused, not a crash)
    assert callable(api.Context.set_gain)


def _cli(*argv):
    return subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True, timeout=60)


def test_help_lists_gain():
    r = _cli("--help")
    assert r.returncode == 0
    assert "[--gain G]" in r.stdout and "\n--gain:" in r.stdout


@pytest.mark.parametrize("argv,message", [
    (["--gain", "0"], "--gain takes a finite number above 0: 0"),
    (["--gain", "-2"], "--gain takes a finite number above 0: -2"),
    (["--gain", "nan"], "--gain takes a finite number above 0: nan"),
    (["--gain", "inf"], "--gain takes a finite number above 0: inf"),
    (["--gain", "x"], "pattern not found for '--gain': x"),
    (["--gain", "2.5x"], "pattern not found for '--gain': 2.5x"),
    (["--gain", ""], "pattern not found for '--gain'"),
    (["--gain"], "Too few arguments for '--gain'")])
def test_bad_gain_is_refused_with_usage(argv, message):
    r = _cli("synth:tiny:1", *argv)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout and "Usage: spotfinder" in r.stdout, r.stdout
