"""CPU: the window-size parameter (ffs_params.kernel_half_x / _y) -- its ABI, the CLI flag's refusals, and the oracle's
restatement of standalone.cc at windows other than 7x7 against a direct NumPy window sum."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HEADER = os.path.join(ROOT, "include", "ffs_hip.h")


def test_default_params_window_is_3_3():
    from ffs_amd import api
    lib = api.load_library()
    p = api.Params()
    lib.ffs_default_params(C.byref(p))
    assert (p.kernel_half_x, p.kernel_half_y) == (3, 3)


def test_params_field_order_matches_header():
    from ffs_amd import api
    src = open(HEADER).read()
    body = src[src.index("typedef struct {\n    int32_t min_count;"):]
    body = body[:body.index("} ffs_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [f for f, _ in api.Params._fields_]
    assert fields[-2:] == ["kernel_half_x", "kernel_half_y"]
    assert "#define FFS_PATH_WINDOW 64u" in src
    assert api.Stream.PATH_BITS["window"] == 64


def _cli(*argv):
    return subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True, timeout=60)


def test_help_lists_kernel_size():
    r = _cli("--help")
    assert r.returncode == 0 and "--kernel-size" in r.stdout


_RANGE = "--kernel-size takes half-sizes 1..7"
_PATTERN = "pattern not found for '--kernel-size'"


@pytest.mark.parametrize("argv,message", [
    (["--kernel-size", "0"], _RANGE), (["--kernel-size", "8"], _RANGE), (["--kernel-size", "3,9"], _RANGE),
    (["--kernel-size", "3,"], _PATTERN), (["--kernel-size", ",3"], _PATTERN), (["--kernel-size", "a"], _PATTERN),
    (["--kernel-size", "2,3,4"], _PATTERN), (["--kernel-size", "-1"], _PATTERN),
    (["--kernel-size"], "Too few arguments for '--kernel-size'"),
    (["-a", "dispersion_extended", "--kernel-size", "5"], "not available with the dispersion_extended algorithm"),
    (["--kernel-size", "2,3", "-a", "Dispersion_Extended"], "not available with the dispersion_extended algorithm")])
def test_bad_kernel_size_is_refused_with_usage(argv, message):
    r = _cli("synth:tiny:1", *argv)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout and "Usage: spotfinder" in r.stdout, r.stdout


# ---- the oracle at other windows against a direct restatement of standalone.cc:113-174 (window sums, clipping, the predicate)
def _numpy_dispersion(img, mask, kx, ky, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0):
    H, W = img.shape
    v = img.astype(np.int64)
    ok = (mask != 0) & (v < (1 << 24))               # standalone.cc:78,90
    pv = np.where(ok, v, 0)
    out = np.zeros((H, W), np.uint8)
    for yy in range(H):
        for xx in range(W):
            y0, y1 = max(yy - ky, 0), min(yy + ky, H - 1)    # :126-130
            x0, x1 = max(xx - kx, 0), min(xx + kx, W - 1)
            m = int(ok[y0:y1 + 1, x0:x1 + 1].sum())
            x = int(pv[y0:y1 + 1, x0:x1 + 1].sum())
            y = int((pv[y0:y1 + 1, x0:x1 + 1] ** 2).sum())
            src = float(v[yy, xx])
            if not (mask[yy, xx] and m >= min_count and x >= 0 and src > threshold):
                continue
            md, xd, yd = np.float64(m), np.float64(x), np.float64(y)
            a = md * yd - xd * xd - xd * (md - 1.0)
            b = md * np.float64(src) - xd
            c = xd * np.float64(nsig_b) * np.sqrt(2.0 * (md - 1.0))
            d = np.float64(nsig_s) * np.sqrt(xd * md)
            out[yy, xx] = 1 if (a > c and b > d) else 0
    return out


def _frame(W, H, dtype, seed, masked):
    rng = np.random.default_rng(seed)
    img = rng.poisson(3.0, size=(H, W))
    spots = rng.random((H, W)) < 0.04
    img[spots] = rng.integers(20, 900, size=spots.sum())
    if dtype == np.uint32:
        big = rng.random((H, W)) < 0.03
        img[big] = rng.choice([(1 << 24) - 1, 1 << 24, (1 << 24) + 7], size=big.sum())
    mask = (rng.random((H, W)) > 0.12).astype(np.uint8) if masked else np.ones((H, W), np.uint8)
    return img.astype(dtype), mask


@pytest.mark.parametrize("kx,ky", [(1, 1), (2, 5), (7, 7), (7, 1)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("W,H,masked", [(37, 29, True), (40, 31, False), (5, 40, True), (33, 3, False), (2, 2, True)])
def test_oracle_other_windows_against_numpy(kx, ky, dtype, W, H, masked):
    img, mask = _frame(W, H, dtype, seed=W * 7 + H + kx * 100 + ky, masked=masked)
    want = _numpy_dispersion(img, mask, kx, ky)
    got = O.dispersion(img, mask, O.DispParams(kx, ky, 2, 0.0, 6.0, 3.0))
    assert np.array_equal(got, want)
    if min(W, H) > 10:
        assert want.sum() > 0
