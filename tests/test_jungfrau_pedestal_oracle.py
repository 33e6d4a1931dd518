"""CPU: the truth of the Jungfrau pedestal measurement (tests/jungfrau_pedestal_oracle.py, NumPy) agrees with a pixel loop in Python
integers and with the header the kernel, the library, the driver and ffs_hosttool compile (csrc/jungfrau_pedestal_model.hpp), run as a
process of its own -- built with g++ -ffp-contract=off, plain and under the address and undefined-behaviour sanitizers -- through
tests/jungfrau_pedestal_check.cc.  The cases: counts 0, 1 and 2^32 - 1, sums of squares near 2^60, a variance that rounding makes negative,
an rms exactly at max_rms, every invalid word, the words at the stages' edges.  And the synthetic dark run: deterministic, its stages in
thirds, stuck pixels, every measured pedestal within the generator's amplitude of the true one."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import jungfrau_pedestal_oracle as P
from ffs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
F = np.float32
TOP = (1 << 32) - 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jfped") / f"jungfrau_pedestal_check_{request.param}")
    flags = SANITIZE if request.param == "sanitized" else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "jungfrau_pedestal_check.cc")], check=True)
    return exe


def _run(exe, args, text):
    return subprocess.run([exe, *map(str, args)], input=text, capture_output=True, text=True, check=True).stdout.split()


# ---- the fold ---------------------------------------------------------------------------------------------------------------------------
# every invalid word, the words the issue names, and both ends of every gain code
WORDS = [0xFFFF, 0xC000, 0x8000, 0x8001, 0xBFFF, 0x0000, 0x3FFF, 0x7FFF, 0xFFFE, 0x4000, 0xC001, 0x0001, 0x4001, 0x3FFE]


def _fold_case(seed, n=5, H=3, W=29):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 16, (n, H, W)).astype(np.uint16)
    raw[:, 0, :len(WORDS)] = WORDS                       # the same word in every frame: its pixel's sums are n times the word's
    raw[0, 1, :len(WORDS)] = WORDS[::-1]
    raw[:, 2, :4] = 0x3FFF, 0x7FFF, 0xFFFE, 0xFFFF       # the largest ADC of every stage, frame after frame
    return raw


def test_hand_words_in_the_oracle():
    acc = P.fold(P.zeros(1, len(WORDS)), np.array(WORDS, np.uint16).reshape(1, 1, -1))
    want = {0x0000: (0, 0), 0x3FFF: (0, 16383), 0x7FFF: (1, 16383), 0xFFFE: (2, 16382), 0x4000: (1, 0), 0xC001: (2, 1), 0x0001: (0, 1), 0x4001: (1, 1),
            0x3FFE: (0, 16382)}
    assert acc[0] == 1
    for i, r in enumerate(WORDS):
        counts = [int(acc[1][s, 0, i]) for s in range(3)]
        if r in want:
            s, a = want[r]
            assert counts == [int(t == s) for t in range(3)], hex(r)
            assert int(acc[2][s, 0, i]) == a and int(acc[3][s, 0, i]) == a * a
        else:
            assert counts == [0, 0, 0], hex(r)
        assert sum(int(acc[2][s, 0, i]) for s in range(3)) == (want[r][1] if r in want else 0)


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_fold_equals_the_integer_loop(seed):
    raw = _fold_case(seed)
    n, H, W = raw.shape
    acc = P.fold(P.zeros(H, W), raw[:2])
    acc = P.fold(acc, raw[2])                      # a single (H, W) frame, and accumulation across calls
    acc = P.fold(acc, raw[3:])
    n_loop, count, total, total_sq = P.fold_loop(H, W, raw)
    assert acc[0] == n_loop == n
    assert acc[1].reshape(3, -1).tolist() == count and acc[2].reshape(3, -1).tolist() == total and acc[3].reshape(3, -1).tolist() == total_sq
    assert (acc[1].sum(axis=0) < n).any() and (acc[1] > 0).any(axis=(1, 2)).all()   # (some words count nowhere; every stage has some)
    assert acc[1].dtype == np.uint32 and acc[2].dtype == np.uint64 and acc[3].dtype == np.uint64


@pytest.mark.parametrize("seed", [3, 4])
def test_header_fold_equals_the_oracle(check, seed):
    raw = _fold_case(seed)
    n, H, W = raw.shape
    out = _run(check, ["fold", n, H * W], " ".join(map(str, raw.reshape(-1).tolist())))
    got = np.array([int(x) for x in out], dtype=object).reshape(3, 3, H, W)
    acc = P.fold(P.zeros(H, W), raw)
    for j in range(3):
        assert got[j].tolist() == acc[1 + j].tolist(), ("count", "sum", "sum_sq")[j]


def test_frame_limit(check):
    cases = [(0, 1, 1), (0, TOP, 1), (0, TOP + 1, 0), (TOP - 1, 1, 1), (TOP - 1, 2, 0), (TOP, 1, 0), (TOP, 0, 1), (5, TOP - 5, 1), (5, TOP - 4, 0)]
    out = _run(check, ["fit"], "\n".join(f"{a} {b}" for a, b, _ in cases))
    assert [int(x) for x in out] == [ok for _, _, ok in cases]
    assert P.MAX_FRAMES == TOP


# ---- the planes -------------------------------------------------------------------------------------------------------------------------
def _exact_entry(c, s, q):
    """One stage of one pixel from the rule's text, each float64 operation as a correctly rounded one of exact rationals."""
    if c == 0:
        return F(0), F(0)
    m = float(Fraction(float(s)) / Fraction(float(c)))       # float(int) rounds to nearest even; Fraction -> float likewise
    qq = float(Fraction(float(q)) / Fraction(float(c)))
    mm = float(Fraction(m) * Fraction(m))
    v = float(Fraction(qq) - Fraction(mm))
    return F(m), F(math.sqrt(v if v > 0 else 0.0))


def _plane_cases():
    """(count, sum, sum_sq) triples: the edges the issue names and random ones a fold can produce."""
    cases = [(0, 0, 0), (0, 5, 25), (1, 0, 0), (1, 16383, 16383 ** 2), (1, 2812, 2812 ** 2), (2, 2 * 2812 + 1, 2812 ** 2 + 2813 ** 2),
             (TOP, TOP * 16383, TOP * 16383 ** 2), (TOP, TOP * 9000 + 12345, TOP * 9000 ** 2 + 2 * 9000 * 12345 + 99999),      # sum_sq near 2^60
             (TOP, 0, 0), (3, 3 * 16383, 3 * 16383 ** 2), (1000, 1000 * 15111, 1000 * 15111 ** 2),
             (3, 10, 34), (7, 7 * 3 + 1, 7 * 9 + 7)]
    # constant pixels: the true variance is 0.  Where c a^2 is beyond 2^53 its conversion to float64 may round down, q comes out below
    # m * m and v is -2^-25: clamped to 0 (4000000001 x 16376^2 and 3000000007 x 16381^2 do)
    for c, a in ((3, 16383), (7, 12345), (TOP, 16383), (11, 9999), (1 << 31, 15001), (6, 2801), (4000000001, 16376), (3000000007, 16381), (3000000007, 16379)):
        cases.append((c, c * a, c * a * a))
    # one count lost to an invalid word: a / c is inexact
    for c, a in ((3, 10001), (49, 14600), (77777, 2899)):
        cases.append((c, c * a + 1, c * a * a + 2 * a + 1))
    rng = np.random.default_rng(5)
    for _ in range(300):
        c = int(rng.integers(1, 5000))
        vals = rng.integers(int(rng.integers(0, 16000)), 16384, c)
        if rng.random() < 0.5:
            vals = np.clip(int(vals[0]) + rng.integers(-2, 3, c), 0, 16383)
        cases.append((c, int(vals.sum()), int((vals.astype(np.int64) ** 2).sum())))
    return cases


def test_oracle_planes_equal_the_rule_in_exact_rationals():
    cases = _plane_cases()
    c = np.array([x[0] for x in cases], np.uint32)
    s = np.array([x[1] for x in cases], np.uint64)
    q = np.array([x[2] for x in cases], np.uint64)
    assert int(q.max()) > (1 << 59) and int(q.max()) > (1 << 53)
    ped, rms, ok = P.planes(c, s, q)
    assert ped.dtype == F and rms.dtype == F and ok.dtype == bool
    negative = 0
    for i, (ci, si, qi) in enumerate(cases):
        wp, wr = _exact_entry(ci, si, qi)
        assert _bits(ped[i:i + 1])[0] == _bits(np.array([wp]))[0] and _bits(rms[i:i + 1])[0] == _bits(np.array([wr]))[0], cases[i]
        assert ok[i] == (ci > 0)
        if ci:
            m = float(Fraction(float(si)) / Fraction(float(ci)))
            negative += float(Fraction(float(qi)) / Fraction(float(ci))) - m * m < 0
    assert negative >= 1, "no case whose variance rounding makes negative"
    assert ped[0] == 0 and rms[0] == 0 and not ok[0] and not ok[1]


def _thresholds():
    """(min_frames, max_rms) pairs, among them an rms exactly at max_rms and its two float32 neighbours."""
    _, rms, _ = P.planes(np.array([3], np.uint32), np.array([10], np.uint64), np.array([34], np.uint64))
    assert rms[0] > 0
    return [(1, 0.0), (2, 0.0), (3, 0.0), (1000, 0.0), (TOP, 0.0), (1, float(rms[0])), (1, float(np.nextafter(rms[0], F(0)))), (1, float(np.nextafter(rms[0], F(9)))),
            (1, 1.5), (4, 0.25), (1, float(np.finfo(F).max)), (1, 1e-45)], rms[0]


def test_header_planes_equal_the_oracle(check):
    cases = _plane_cases()
    c = np.array([x[0] for x in cases], np.uint32)
    s = np.array([x[1] for x in cases], np.uint64)
    q = np.array([x[2] for x in cases], np.uint64)
    text = "\n".join(f"{a} {b} {d}" for a, b, d in cases)
    thresholds, at = _thresholds()
    i_at = cases.index((3, 10, 34))
    seen = set()
    for min_frames, max_rms in thresholds:
        ped, rms, ok = P.planes(c, s, q, min_frames, max_rms)
        out = np.array(_run(check, ["planes", min_frames, int(_bits(np.array([max_rms], F))[0])], text), dtype=np.uint64).reshape(-1, 3)
        assert np.array_equal(out[:, 0].astype(np.uint32), _bits(ped)), (min_frames, max_rms)
        assert np.array_equal(out[:, 1].astype(np.uint32), _bits(rms)), (min_frames, max_rms)
        assert np.array_equal(out[:, 2].astype(bool), ok), (min_frames, max_rms)
        if max_rms:
            seen.add((F(max_rms) < at, F(max_rms) == at, bool(ok[i_at])))
    # exactly at max_rms is usable, the float32 below it is not
    assert (False, True, True) in seen and (True, False, False) in seen and (False, False, True) in seen


def test_plane_arguments(check):
    cases = [(1, 0.0, 1), (0, 0.0, 0), (1, -0.0, 1), (1, -1e-45, 0), (1, -1.0, 0), (1, np.inf, 0), (1, -np.inf, 0), (1, np.nan, 0), (TOP, 3.5, 1),
             (1, float(np.finfo(F).max), 1), (1, 1e-45, 1)]
    out = _run(check, ["args"], "\n".join(f"{m} {int(_bits(np.array([r], F))[0])}" for m, r, _ in cases))
    assert [int(x) for x in out] == [ok for _, _, ok in cases]
    for m, r, ok in cases:
        assert P.args_ok(m, r) == bool(ok), (m, r)


def test_repedestalled_calibration(check):
    n = 40
    rng = np.random.default_rng(9)
    old_ped = rng.normal(3000, 100, (3, 1, n)).astype(F)
    old_fac = rng.normal(0, 1, (3, 1, n)).astype(F)
    old_fac[rng.random((3, 1, n)) < 0.1] = 0.0
    ped = rng.normal(3000, 100, (3, 1, n)).astype(F)
    ok = rng.random((3, 1, n)) < 0.7
    new_ped, new_fac = P.repedestal(old_ped, old_fac, ped, ok)
    assert np.array_equal(_bits(new_ped), _bits(ped)) and np.array_equal(_bits(new_fac[ok]), _bits(old_fac[ok])) and (new_fac[~ok] == 0).all()
    assert (_bits(new_fac[~ok]) == 0).all(), "+0, not -0"
    text = " ".join(map(str, np.concatenate([_bits(old_ped).reshape(-1), _bits(old_fac).reshape(-1), _bits(ped).reshape(-1), ok.astype(np.uint32).reshape(-1)]).tolist()))
    out = np.array(_run(check, ["repedestal", n], text), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(out, np.concatenate([_bits(new_ped).reshape(-1), _bits(new_fac).reshape(-1)]))


# ---- the synthetic dark run -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dark():
    W, H, seed, n = 300, 200, 7, 48
    ped, fac = synth.jungfrau_calibration(W, H, seed)
    return W, H, seed, n, ped, synth.dark_frames(W, H, seed, n)


def test_dark_run_is_deterministic_in_thirds_and_has_stuck_pixels(dark):
    W, H, seed, n, ped, frames = dark
    assert frames.dtype == np.uint16 and frames.shape == (n, H, W)
    assert np.array_equal(frames[17], synth.jungfrau_dark(W, H, ped, seed, 17, n))
    assert not np.array_equal(frames[17], synth.jungfrau_dark(W, H, ped, seed + 1, 17, n))
    assert not np.array_equal(frames[16], frames[17])
    counts = P.word_counts(frames)
    stages = P.stage(frames)
    # a pixel is stuck when it reports G0 in the frames forced into G2
    stuck = (counts[2 * n // 3:] & (stages[2 * n // 3:] == 0)).any(axis=0)
    assert 0.0003 < stuck.mean() < 0.003, stuck.mean()
    for f in range(n):
        forced = 3 * f // n
        assert (stages[f][counts[f] & ~stuck] == forced).all(), f
        assert (stages[f][counts[f] & stuck] == 0).all(), f
    invalid = ~counts
    assert 0.5 / 4096 < invalid.mean() < 2.0 / 4096
    assert {0xFFFF, 0xC000} <= set(np.unique(frames[invalid]).tolist()) and ((frames[invalid] >> 14) == 2).any()
    with pytest.raises(ValueError):
        synth.jungfrau_dark(W, H, ped, seed, n, n)


def test_measured_pedestals_lie_within_the_generators_amplitude(dark, ffs):
    W, H, seed, n, ped, frames = dark
    acc = P.fold(P.zeros(H, W), frames)
    assert acc[0] == n
    got, rms, ok = P.planes(*acc[1:], min_frames=n // 3 - 2, max_rms=2.5)
    some = acc[1] > 0
    lo = np.floor(ped) - 2
    assert some[0].all() and 0.997 < some[1].mean() < 1 and 0.997 < some[2].mean() < 1
    assert (got[some] >= lo[some]).all() and (got[some] <= lo[some] + 4).all()
    assert (rms[some] <= 2.0).all() and ok[0].all() and (ok == some).mean() > 0.99 and not ok[~some].any()
    # the stuck pixels: no G1, no G2, twice as many G0 words
    stuck = ~some[2]
    assert (acc[1][0][stuck] > 2 * n // 3).all() and not some[1][stuck].any()
    # ... and the library's host function gives the oracle's planes (no GPU involved)
    lib_ped, lib_rms, lib_ok = ffs.jungfrau_pedestal_planes(acc, min_frames=n // 3 - 2, max_rms=2.5)
    assert np.array_equal(_bits(lib_ped), _bits(got)) and np.array_equal(_bits(lib_rms), _bits(rms)) and np.array_equal(lib_ok, ok)
    for bad in (dict(min_frames=0), dict(max_rms=-1.0), dict(max_rms=float("nan")), dict(max_rms=float("inf"))):
        with pytest.raises(ffs.FfsError, match="min_frames|max_rms"):
            ffs.jungfrau_pedestal_planes(acc, **bad)
