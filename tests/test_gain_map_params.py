"""CPU: the per-pixel gain map (ffs_ctx_set_gain_map) -- its ABI and binding, and the driver's --gain-map with its refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HEADER = os.path.join(ROOT, "include", "ffs_hip.h")
TINY = (200, 300)   # synth:tiny, H x W


def test_header_declares_the_setter():
    src = open(HEADER).read()
    assert re.search(r"\bint\s+ffs_ctx_set_gain_map\s*\(\s*ffs_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*host_gain\s*\)\s*;", src)
    comment = src[:src.index("int ffs_ctx_set_gain_map")]
    comment = comment[comment.rindex("/*"):]
    # what it stands for: the reference's gain array read at the centre, DIALS's lookup, and the float32 promise
    assert "baseline.cpp" in comment and "lookup.gain_map" in comment and "gain[k]" in comment
    assert "ffs_ctx_set_gain(ctx, (double)(float)c)" in comment and "FFS_ERR_INVALID" in comment


def test_library_exports_the_setter_and_the_binding_knows_it():
    from ffs_amd import api
    lib = api.load_library()
    assert hasattr(lib, "ffs_ctx_set_gain_map")
    assert "ffs_ctx_set_gain_map" in api.EXPORTS
    assert lib.ffs_ctx_set_gain_map.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.ffs_ctx_set_gain_map(None, None) != 0   # (no context: refused, not a crash)
    assert callable(api.Context.set_gain_map)


def _cli(*argv):
    return subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True, timeout=60)


def test_help_lists_the_flag():
    r = _cli("--help")
    assert r.returncode == 0
    assert "[--gain-map FILE]" in r.stdout and "\n--gain-map:" in r.stdout and "lookup.gain_map" in r.stdout


def _map_file(tmp_path, values, name="gain.f32"):
    p = tmp_path / name
    np.asarray(values, "<f4").tofile(p)
    return str(p)


def _refused(r, message):
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout and "Usage: spotfinder" in r.stdout, r.stdout


def test_a_missing_file_is_refused_with_usage(tmp_path):
    _refused(_cli("synth:tiny:1", "--gain-map", str(tmp_path / "nothing.f32")), "--gain-map: no such file")
    _refused(_cli("synth:tiny:1", "--gain-map"), "Too few arguments for '--gain-map'")


@pytest.mark.parametrize("n", [0, 200 * 300 - 1, 200 * 300 + 1, 300])
def test_a_file_of_another_size_is_refused_with_usage(tmp_path, n):
    r = _cli("synth:tiny:1", "--gain-map", _map_file(tmp_path, np.ones(n)))
    _refused(r, "--gain-map: ")
    assert f"holds {4 * n} bytes" in r.stdout and "300 x 200" in r.stdout and str(4 * 200 * 300) in r.stdout


def test_gain_together_with_a_map_is_refused_with_usage(tmp_path):
    f = _map_file(tmp_path, np.ones(TINY))
    for argv in (["--gain", "2.5", "--gain-map", f], ["--gain-map", f, "--gain", "2.5"]):
        _refused(_cli("synth:tiny:1", *argv), "--gain and --gain-map exclude each other")


@pytest.mark.parametrize("bad", [0.0, float("nan"), -2.5, float("inf"), 2.0 ** -61, 2.0 ** 61])
def test_a_file_with_a_bad_value_is_refused_with_usage(tmp_path, bad):
    g = np.full(TINY, 2.5, np.float32)
    g[7, 11] = bad
    r = _cli("synth:tiny:1", "--gain-map", _map_file(tmp_path, g))
    _refused(r, f"--gain-map: value {7 * 300 + 11} of ")
    assert "[2^-60, 2^60]" in r.stdout
