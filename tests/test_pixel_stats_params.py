"""CPU: the per-pixel statistics' ABI and binding, and the driver's --pixel-stats with its refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HEADER = os.path.join(ROOT, "include", "ffs_hip.h")


def test_header_declares_the_entry_points():
    src = open(HEADER).read()
    assert re.search(r"\bint\s+ffs_ctx_set_pixel_stats\s*\(\s*ffs_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*\)\s*;", src)
    assert re.search(r"\bint\s+ffs_ctx_get_pixel_stats\s*\(\s*ffs_ctx\s*\*\s*ctx\s*,\s*ffs_pixel_stats\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"\bint\s+ffs_bench_pixel_stats\s*\(\s*ffs_stream\s*\*\s*s\s*,\s*const\s+void\s*\*\s*device_pixels\s*,\s*size_t\s+pitch_bytes\s*,"
                     r"\s*size_t\s+frame_stride_bytes\s*,\s*uint32_t\s+n_frames\s*,\s*uint32_t\s+iters\s*,\s*float\s*\*\s*ms\s*\)\s*;", src)
    for name, value in (("FFS_PIXEL_STATS_OFF", "0"), ("FFS_PIXEL_STATS_START", "1"), ("FFS_PIXEL_STATS_RESUME", "2"), ("FFS_PATH_PIXEL_STATS", "256u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), src), name
    body = src[:src.index("} ffs_pixel_stats;")]
    body = body[body.rindex("typedef struct {"):]
    assert re.findall(r"(\w+)\s*;", body) == ["n_frames", "count", "sum", "sum_sq", "max"]
    assert "uint64_t n_frames" in body and "uint32_t *count" in body and "uint64_t *sum;" in body and "uint64_t *sum_sq" in body and "uint32_t *max" in body
    # (setters on the context, not fields: the layout of ffs_params is pinned by other tests)
    params = src[src.index("typedef struct {\n    int32_t min_count;"):]
    assert "pixel_stats" not in params[:params.index("} ffs_params;")]
    comment = src[:src.index("#define FFS_PIXEL_STATS_OFF")]
    comment = comment[comment.rindex("/*"):]
    for what in ("max_valid", "2^24", "modulo 2^64", "65 536", "mask plays no part", "n_frames", "in flight", "counts once", "undefined", "24 bytes per pixel",
                 "FFS_ERR_NOMEM", "ffs_bench_pixel_stats"):
        assert what in comment, what
    assert '"stats_stream"' in src


def test_library_exports_them_and_the_binding_knows_them():
    from ffs_amd import api
    lib = api.load_library()
    for name in ("ffs_ctx_set_pixel_stats", "ffs_ctx_get_pixel_stats", "ffs_bench_pixel_stats"):
        assert hasattr(lib, name) and name in api.EXPORTS
    assert lib.ffs_ctx_set_pixel_stats.argtypes == [C.c_void_p, C.c_int]
    assert lib.ffs_ctx_get_pixel_stats.argtypes == [C.c_void_p, C.POINTER(api._PixelStats)]
    assert lib.ffs_bench_pixel_stats.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    assert lib.ffs_ctx_set_pixel_stats(None, 1) != 0        # (no context: refused, not a crash)
    assert lib.ffs_ctx_get_pixel_stats(None, None) != 0
    assert lib.ffs_bench_pixel_stats(None, None, 0, 0, 0, 0, None) != 0
    assert api.Stream.PATH_BITS["pixel_stats"] == 256
    assert [f for f, _ in api._PixelStats._fields_] == ["n_frames", "count", "sum", "sum_sq", "max"]
    assert C.sizeof(api._PixelStats) == 40
    assert api.PIXEL_STATS_MODES == {"off": 0, "start": 1, "resume": 2}
    assert callable(api.Context.set_pixel_stats) and callable(api.Context.pixel_stats) and callable(api.Stream.bench_pixel_stats)


def _cli(*argv, cwd=None):
    return subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True, timeout=60, cwd=cwd)


def test_help_lists_pixel_stats():
    r = _cli("--help")
    assert r.returncode == 0
    assert "[--pixel-stats PREFIX]" in r.stdout and "\n--pixel-stats:" in r.stdout
    for suffix in ("PREFIX.count.u32", "PREFIX.sum.u64", "PREFIX.sum_sq.u64", "PREFIX.max.u32"):
        assert suffix in r.stdout


@pytest.mark.parametrize("argv,message", [
    (["--pixel-stats"], "Too few arguments for '--pixel-stats'"),
    (["--pixel-stats", ""], "--pixel-stats takes the prefix of the four files it writes")])
def test_bad_pixel_stats_is_refused_with_usage(argv, message):
    r = _cli("synth:tiny:1", *argv)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout and "Usage: spotfinder" in r.stdout, r.stdout
