"""CPU: the robust Poisson GLM background.  The text the kernel compiles (csrc/spot_background_glm_model.hpp), as a stand-alone program
built plain and under the address and undefined-behaviour sanitizers, against
  - tests/golden/spot_background_glm_ref.json: what the reference's own glm_constant_background returned for every case of
    tests/spot_background_glm_cases.py (DESIGN.md section 3.8b says how the file was made), and
  - tests/spot_background_glm_oracle.py, the per-pixel Python form with lgamma and libm.

TOLERANCE.  The largest relative difference of the header program's mean from the golden file over the cases was measured at 6.3e-15
(DESIGN.md section 3.8b).  The tests use eight times that, 5.1e-14, for the libm of other machines on the Python side; it is far below
the 1e-9 that must hold in any case.  beta = log(mean), so the same figure bounds beta's absolute difference (scaled by |beta| where
that is above 1, for the rounding of beta itself)."""
import json
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import spot_background_glm_cases as K
import spot_background_glm_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "spot_background_glm_check.cc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "spot_background_glm_ref.json")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
MEASURED = 6.3e-15
TOL = 8 * MEASURED
assert TOL < 1e-9


def _double(hex16):
    return struct.unpack("<d", struct.pack("<Q", int(hex16, 16)))[0]


def parse(line):
    """A line of the check program (or of `ffs_hosttool spotbgglm`) -> (n_pixels, n_overflow, median, n_iter, status, beta, mean)."""
    t = line.split()
    assert len(t) == 7, line
    return tuple(int(v) for v in t[:5]) + (_double(t[5]), _double(t[6]))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("spot_background_glm")
    flags = ["-std=c++20", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, CHECK]
    subprocess.run(["g++", "-O1", *flags, "-o", str(d / "plain")], check=True)
    subprocess.run(["g++", *SANITIZE, *flags, "-o", str(d / "sanitized")], check=True)
    return d


def run(program, rings):
    r = subprocess.run([str(program)], input=K.histogram_text(rings), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(rings)
    return lines


@pytest.fixture(scope="module")
def header_lines(programs):
    rings = [v for _, v in K.cases()]
    plain = run(programs / "plain", rings)
    return plain, run(programs / "sanitized", rings)


def test_sanitized_program_prints_the_same_lines(header_lines, programs):
    plain, sanitized = header_lines
    assert plain == sanitized
    short = subprocess.run([str(programs / "sanitized")], input="1 2 3\n", capture_output=True, text=True, timeout=60)
    assert short.returncode == 2 and "short" in short.stderr


def test_header_against_the_reference(header_lines):
    """valid <=> status 0 on every case; the mean within TOL on every valid case but the all-zero rings, where the reference's 1e-33 is
    compared as below 1e-30 against the header's 0.  No case the reference calls valid ends in status 6."""
    gold = json.load(open(GOLDEN))
    cases = K.cases()
    assert [g["name"] for g in gold] == [n for n, _ in cases]
    worst, n_zero = 0.0, 0
    for (name, v), g, line in zip(cases, gold, header_lines[0]):
        assert g["n"] == len(v) and g["sum"] == int(v.sum()), name       # (the file was made from these very rings)
        rec = parse(line)
        assert g["valid"] == (rec[4] == G.OK), (name, g, line)
        assert not (g["valid"] and rec[4] == G.DEGENERATE)
        if not g["valid"]:
            assert rec[6] == 0.0
            continue
        ref = _double(g["mean"])
        if len(v) and not v.any():
            assert abs(ref) < 1e-30 and rec[6] == 0.0 and rec[5] == -math.inf and rec[3] == 0, (name, ref, line)
            n_zero += 1
            continue
        rel = abs(rec[6] - ref) / ref
        worst = max(worst, rel)
        assert rel <= TOL, (name, rel, rec[6], ref)
    print("largest relative difference from the reference:", worst)
    assert n_zero >= 1


def test_header_against_the_python_oracle(header_lines):
    """Status, n_iter and the other integers equal on every case; mean and beta within TOL."""
    for (name, v), want, line in zip(K.cases(), K.results(), header_lines[0]):
        rec = parse(line)
        assert rec[:5] == tuple(want[k] for k in G.INTEGER_FIELDS), (name, line, want)
        if want["status"] != G.OK:
            assert rec[6] == 0.0 and want["mean"] == 0.0
        if want["mean"] > 0.0:
            assert abs(rec[6] - want["mean"]) <= TOL * want["mean"], (name, rec[6], want["mean"])
        else:
            assert rec[6] == 0.0
        if math.isinf(want["beta"]):
            assert rec[5] == want["beta"]
        elif want["status"] in (G.OK, G.NOT_CONVERGED):
            # (a fit that cycles for 100 steps keeps no digits to compare: its beta is only asked to be finite)
            if want["status"] == G.OK:
                assert abs(rec[5] - want["beta"]) <= TOL * max(1.0, abs(want["beta"])), (name, rec[5], want["beta"])
            else:
                assert math.isfinite(rec[5])
        else:
            assert rec[5] == 0.0 and want["beta"] == 0.0


def test_census():
    """The cases reach every status found reachable (6 was reached by no histogram: csrc/spot_background_glm_model.hpp), n_iter 0, 1 and
    >= 10, the seed 0 -> 1, j1 < 0 and j2 >= 255 (where the clamp of the look-up works)."""
    res = K.results()
    assert {r["status"] for r in res} == {G.OK, G.NO_PIXELS, G.OVERFLOW, G.FEW_PIXELS, G.NOT_CONVERGED}
    iters = [r["n_iter"] for r in res if r["status"] == G.OK]
    assert 0 in iters and 1 in iters and max(iters) >= 10
    assert sum(r["seed_from_zero"] for r in res) > 50
    assert sum(1 for r in res if r["j1_min"] is not None and r["j1_min"] < 0) > 50
    assert sum(1 for r in res if r["j2_max"] is not None and r["j2_max"] >= 255) >= 2
    names = [n for n, _ in K.cases()]
    assert len(names) == len(set(names)) and all(n in names for n in K.planted())


def test_clean_poisson_ring_lies_near_its_sample_mean(header_lines):
    """Within 3 standard errors sqrt(mean / N) of the sample mean."""
    lines = dict(zip((n for n, _ in K.cases()), header_lines[0]))
    for name in ("poisson_3_clean", "poisson_40_clean", "poisson_3_of_100000", "poisson_200", "poisson_0_05"):
        v = K.planted()[name].astype(np.float64)
        rec = parse(lines[name])
        assert rec[4] == G.OK and v.max() < 256
        assert abs(rec[6] - v.mean()) <= 3.0 * math.sqrt(v.mean() / len(v)), (name, rec[6], v.mean())


def test_overflow_height_and_order_change_nothing(programs):
    """Moving the pixels of the tail further up, or permuting the ring, leaves the record as it is: bit for bit in the header program (it
    sees the same histogram), and in the per-pixel oracle status and n_iter stay and the mean moves by rounding only."""
    rng = np.random.default_rng(77)
    picked = [(n, v) for n, v in K.cases() if (v >= 256).any() and 4 * int((v >= 256).sum()) <= len(v) >= 10][:40]
    assert len(picked) == 40
    base = run(programs / "plain", [v for _, v in picked])
    higher = [np.where(v >= 256, v * 1000, v) for _, v in picked]
    shuffled = [rng.permutation(v) for _, v in picked]
    assert run(programs / "plain", higher) == base and run(programs / "plain", shuffled) == base
    for (name, v), hi, sh in zip(picked, higher, shuffled):
        a = G.from_values(v)
        for other in (G.from_values(hi), G.from_values(sh)):
            assert (other["status"], other["n_iter"], other["median"]) == (a["status"], a["n_iter"], a["median"]), name
            assert abs(other["mean"] - a["mean"]) <= TOL * max(a["mean"], 1e-300), name


def test_planted_frames_give_the_planted_boxes(programs):
    """Under the committed oracle (dispersion, connected components, both filters) every planted frame of the GPU test returns its planted
    box, and the ring around it ends as planted -- in the Python form and in the header program alike."""
    from util import oracle_frame
    for name, c in K.planted_frames().items():
        mask = c["mask"] if c["mask"] is not None else np.ones(c["frame"].shape, np.uint8)
        _, _, refl = oracle_frame(c["frame"], mask)
        r = refl.reflections
        boxes = [(int(a), int(b), int(cc), int(d)) for a, b, cc, d in zip(r["x_min"], r["x_max"], r["y_min"], r["y_max"])]
        assert c["box"] in boxes, (name, boxes)
        ring = G.ring_values(c["frame"], c["mask"], -1, c["box"], c["border"])
        want = G.from_values(ring)
        rec = parse(run(programs / "plain", [ring])[0])
        assert not G.near_the_tolerance(want), name
        assert rec[:5] == tuple(want[k] for k in G.INTEGER_FIELDS), (name, rec, want)
        assert rec[4] == c["status"] and rec[0] == c["n_pixels"], (name, rec)
        assert rec[3] == c.get("n_iter", rec[3]) and rec[3] >= c.get("n_iter_at_least", 0) and rec[6] == c.get("mean", rec[6]), (name, rec)
