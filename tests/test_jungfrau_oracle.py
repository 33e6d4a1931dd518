"""CPU: the truth of the Jungfrau gain-stage conversion (tests/jungfrau_oracle.py, NumPy float32) agrees with a pixel loop over np.float32
scalars and with the header the kernel and the host converter compile (csrc/jungfrau_model.hpp), run as a process of its own -- built with
g++ -ffp-contract=off, plain and under the address and undefined-behaviour sanitizers -- through tests/jungfrau_check.cc.  The cases: every
gain code, the three invalid words and a zero factor, ties on both parities, negative results, the clamp on both sides of 16777215,
negative factors, denormal pedestals, the range edges of the setter."""
import os
import subprocess

import numpy as np
import pytest

import jungfrau_oracle as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jf") / f"jungfrau_check_{request.param}")
    flags = SANITIZE if request.param == "sanitized" else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "jungfrau_check.cc")], check=True)
    return exe


def _run_frame(exe, raw, ped, fac):
    n = raw.size
    text = " ".join(map(str, raw.reshape(-1).tolist())) + " " + " ".join(map(str, np.concatenate([_bits(ped).reshape(-1), _bits(fac).reshape(-1)]).tolist()))
    out = subprocess.run([exe, "frame", str(n)], input=text, capture_output=True, text=True, check=True).stdout
    return np.array(out.split(), dtype=np.uint64).astype(np.uint32).reshape(raw.shape)


# ---- the hand-made cases: (word, pedestal of its stage, factor of its stage, expected) -------------------------------------------------
def _word(g, adc):
    return (g << 14) | adc


HAND = [
    # every gain code
    (_word(0, 1000), 100.0, 1.0, 900), (_word(1, 1000), 1500.0, -1.0, 500), (_word(3, 1000), 1250.0, -2.0, 500), (_word(2, 1000), 100.0, 1.0, J.INVALID),
    # the three invalid words and a zero factor
    (0xFFFF, 0.0, 1.0, J.INVALID), (0xC000, 0.0, 1.0, J.INVALID), (_word(2, 0), 0.0, 1.0, J.INVALID), (_word(0, 500), 0.0, 0.0, J.INVALID),
    (_word(1, 500), 0.0, -0.0, J.INVALID), (0xC001, 0.0, 1.0, 1), (0xBFFF, 0.0, 1.0, J.INVALID), (0x3FFF, 0.0, 1.0, 16383), (0x7FFF, 0.0, 1.0, 16383),
    # ties on both parities (pedestal 0.5, factor 1): 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    (_word(0, 1), 0.5, 1.0, 0), (_word(0, 2), 0.5, 1.0, 2), (_word(0, 3), 0.5, 1.0, 2), (_word(0, 4), 0.5, 1.0, 4), (_word(0, 1001), 0.5, 1.0, 1000),
    (_word(0, 1002), 0.5, 1.0, 1002),
    # negative results go to 0 (and a tie below zero, and a negative zero)
    (_word(0, 10), 100.0, 1.0, 0), (_word(1, 1000), 100.0, -1.0, 0), (_word(0, 0), 0.5, 1.0, 0), (_word(0, 0), 1.5, 1.0, 0), (_word(0, 0), 0.0, -1.0, 0),
    # the clamp on both sides of 16777215: 16383 * 1024 = 16776192 below; 16383 x 1024.0625 = 16777215.9 -> float32 16777216 -> clamp
    (_word(0, 16383), 0.0, 1024.0, 16776192), (_word(0, 16383), 0.0, 1024.0625, J.MAX_PHOTONS), (_word(0, 16383), -0.75, 1024.0, 16776960),
    # (4095 x 4097 = 16777215 exactly; 4095 x (4097 - 2^-11) = 16777213.0005 -> 16777213)
    (_word(0, 16383), -1.0, 1024.0, J.MAX_PHOTONS), (_word(0, 16383), 0.0, 65536.0, J.MAX_PHOTONS), (_word(0, 4095), 0.0, 4097.0, J.MAX_PHOTONS),
    (_word(0, 4095), 0.0, 4096.99951171875, 16777213), (_word(0, 4095), 0.0, 4096.75, 16776191), (_word(0, 16383), -65536.0, 65536.0, J.MAX_PHOTONS),
    # negative factors
    (_word(1, 14000), 14600.0, -0.05, 30), (_word(3, 15000), 15300.0, -0.7, 210), (_word(1, 15000), 14600.0, -0.05, 0), (_word(3, 1), 65536.0, -65536.0, J.MAX_PHOTONS),
    # denormal pedestals: with or without flushing
    (_word(0, 0), 1e-40, 1.0, 0), (_word(0, 0), -1e-40, 65536.0, 0), (_word(0, 0), 1e-40, -65536.0, 0), (_word(0, 7), 1e-40, 1.0, 7), (_word(0, 7), -1e-45, 1.0, 7),
    # the smallest factor: a normal d, a denormal-free v far below a half
    (_word(0, 16383), -65536.0, 2.0 ** -30, 0), (_word(0, 16383), 65536.0, -(2.0 ** -30), 0),
]


def _hand_arrays():
    n = len(HAND)
    raw = np.array([h[0] for h in HAND], np.uint16).reshape(1, n)
    ped = np.zeros((3, 1, n), F)
    fac = np.ones((3, 1, n), F)
    for i, (r, p, f, _) in enumerate(HAND):
        s = {0: 0, 1: 1, 2: 2, 3: 2}[r >> 14]
        ped[:, 0, i], fac[:, 0, i] = 12345.0, 0.25       # the other stages: a calibration that would give something else
        ped[s, 0, i], fac[s, 0, i] = p, f
    want = np.array([h[3] for h in HAND], np.uint32).reshape(1, n)
    return raw, ped, fac, want


def test_hand_cases_in_the_oracle():
    raw, ped, fac, want = _hand_arrays()
    got = J.convert(raw, ped, fac)
    assert got.dtype == np.uint32
    bad = np.nonzero(got != want)[1]
    assert bad.size == 0, [(hex(HAND[i][0]), HAND[i][1:], int(got[0, i])) for i in bad]
    assert np.array_equal(J.convert_loop(raw, ped, fac), want)


def test_hand_cases_in_the_header(check):
    raw, ped, fac, want = _hand_arrays()
    assert np.array_equal(_run_frame(check, raw, ped, fac), want)


def _random_case(seed, H=24, W=41):
    """Words of every code and calibrations that reach every branch: ties (pedestals at halves, factor +-1), zero and negative factors,
    denormal pedestals, factors at the setter's edges, results around the clamp."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 16, (3, H, W)).astype(np.uint16)
    raw[0, 0, :8] = [0xFFFF, 0xC000, 0x8000, 0xBFFF, 0x0000, 0x4000, 0xC001, 0x3FFF]
    ped = rng.normal(3000, 2500, (3, H, W)).astype(F)
    fac = (rng.normal(0, 1, (3, H, W)) * 10.0 ** rng.integers(-4, 4, (3, H, W))).astype(F)
    u = rng.random((3, H, W))
    ped[u < 0.15] = np.round(ped[u < 0.15]) + F(0.5)
    fac[u < 0.15] = np.where(rng.random((u < 0.15).sum()) < 0.5, 1.0, -1.0)
    ped[(u >= 0.15) & (u < 0.2)] = F(1e-41)
    ped[(u >= 0.2) & (u < 0.22)] = F(-3e-39)
    fac[(u >= 0.22) & (u < 0.3)] = 0.0
    fac[(u >= 0.3) & (u < 0.33)] = F(J.MIN_FACTOR)
    fac[(u >= 0.33) & (u < 0.36)] = -F(J.MAX_FACTOR)
    ped[(u >= 0.36) & (u < 0.38)] = F(J.MAX_PEDESTAL)
    ped[(u >= 0.38) & (u < 0.40)] = -F(J.MAX_PEDESTAL)
    fac[(u >= 0.40) & (u < 0.45)] = F(1024.0) + rng.integers(0, 4, ((u >= 0.40) & (u < 0.45)).sum()).astype(F) / F(16)
    ok = np.abs(fac) >= F(J.MIN_FACTOR)
    fac[~ok & (fac != 0)] = F(J.MIN_FACTOR)
    fac = np.clip(fac, -F(J.MAX_FACTOR), F(J.MAX_FACTOR))
    ped = np.clip(ped, -F(J.MAX_PEDESTAL), F(J.MAX_PEDESTAL))
    return raw, ped, fac


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_equals_the_pixel_loop(seed):
    raw, ped, fac = _random_case(seed)
    got = J.convert(raw, ped, fac)
    assert np.array_equal(got, J.convert_loop(raw, ped, fac))
    assert (got == J.INVALID).sum() > 100 and (got == 0).sum() > 100 and (got == J.MAX_PHOTONS).sum() > 5
    assert ((got > 0) & (got < J.MAX_PHOTONS)).sum() > 500
    assert all(J.entry_ok(False, v) for v in ped.reshape(-1)[:200]) and all(J.entry_ok(True, v) for v in fac.reshape(-1)[:200])


@pytest.mark.parametrize("seed", [3, 4])
def test_header_equals_the_oracle(check, seed):
    raw, ped, fac = _random_case(seed)
    for f in range(raw.shape[0]):
        assert np.array_equal(_run_frame(check, raw[f], ped, fac), J.convert(raw[f], ped, fac))


EDGES = [(0, 65536.0, 1), (0, -65536.0, 1), (0, np.nextafter(F(65536), F(np.inf)), 0), (0, np.nextafter(F(-65536), F(-np.inf)), 0), (0, 0.0, 1), (0, 1e-40, 1),
         (0, np.inf, 0), (0, -np.inf, 0), (0, np.nan, 0),
         (1, 0.0, 1), (1, -0.0, 1), (1, 2.0 ** -30, 1), (1, -(2.0 ** -30), 1), (1, np.nextafter(F(2.0 ** -30), F(0)), 0), (1, -np.nextafter(F(2.0 ** -30), F(0)), 0),
         (1, 65536.0, 1), (1, -65536.0, 1), (1, np.nextafter(F(65536), F(np.inf)), 0), (1, 1e-40, 0), (1, np.inf, 0), (1, np.nan, 0), (1, 1.0, 1), (1, -0.002, 1)]


def test_setter_range_edges_in_the_oracle():
    for is_factor, v, ok in EDGES:
        assert J.entry_ok(bool(is_factor), v) == bool(ok), (is_factor, v)


def test_setter_range_edges_in_the_header(check):
    text = "\n".join(f"{k} {int(_bits(np.array([v], F))[0])}" for k, v, _ in EDGES)
    out = subprocess.run([check, "entry"], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [ok for _, _, ok in EDGES]
