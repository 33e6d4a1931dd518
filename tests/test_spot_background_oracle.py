"""CPU: the oracle of the per-spot background (tests/spot_background_oracle.py, the histogram form include/ffs_hip.h states) tied to an
independent form -- a Python loop over the padded box, a sort, the three positions, the fences in float64 as the reference writes them --
and to the text the kernel compiles (csrc/spot_background_model.hpp) through a stand-alone program, plain and under the address and
undefined-behaviour sanitizers.  The planted frames of tests/spot_background_cases.py give their planted boxes under the committed oracle."""
import os
import subprocess

import numpy as np
import pytest

import spot_background_cases as cases
import spot_background_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "spot_background_check.cc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def sort_form(frame, mask, max_valid, box, border):
    """The independent form: collect the ring into a list, sort it, take the three positions, fence in float64."""
    H, W = frame.shape
    x_min, x_max, y_min, y_max = box
    ring = []
    for y in range(max(y_min - border, 0), min(y_max + border, H - 1) + 1):
        for x in range(max(x_min - border, 0), min(x_max + border, W - 1) + 1):
            if x_min <= x <= x_max and y_min <= y <= y_max:
                continue
            v = int(frame[y, x])
            if mask is not None and not mask[y, x]:
                continue
            if max_valid >= 0 and v > max_valid:
                continue
            if frame.dtype.itemsize == 4 and v >= 1 << 24:
                continue
            ring.append(v)
    ring.sort()
    N = len(ring)
    over = sum(1 for v in ring if v >= 256)
    if N == 0:
        return (0, 0, -1, -1, -1, 0, 0, 1)
    if float(over) > 0.25 * float(N):
        return (N, over, -1, -1, -1, 0, 0, 2)
    q1, med, q3 = ring[(N + 3) // 4 - 1], ring[(N + 1) // 2 - 1], ring[(3 * N + 1) // 4 - 1]
    iqr = float(q3 - q1)
    lower, upper = q1 - 1.5 * iqr, q3 + 1.5 * iqr
    if upper >= 256.0:
        return (N, over, q1, med, q3, 0, 0, 3)
    inl = [v for v in ring if not (v < lower or v > upper) and v < 256]
    if not inl:
        return (N, over, q1, med, q3, 0, 0, 4)
    return (N, over, q1, med, q3, len(inl), sum(inl), 0)


def _random_rings(seed, n):
    """n rings of 0..200 pixel values: Poisson(3 / 5 / 100 / 240 / 300), two-level mixtures, 25 % outliers, uniform 0..599, in turn."""
    rng = np.random.default_rng(seed)
    kinds = ["p3", "p5", "p100", "p240", "p300", "two_levels", "outliers", "uniform"]
    for i in range(n):
        n_px = int(rng.integers(0, 201))
        kind = kinds[i % len(kinds)]
        if kind == "two_levels":
            v = np.where(rng.random(n_px) < rng.random(), rng.poisson(rng.choice([3.0, 20.0, 120.0]), n_px), rng.poisson(rng.choice([40.0, 180.0, 250.0]), n_px))
        elif kind == "outliers":
            v = np.where(rng.random(n_px) < 0.25, rng.integers(256, 5000, n_px), rng.poisson(4.0, n_px))
        elif kind == "uniform":
            v = rng.integers(0, 600, n_px)
        else:
            v = rng.poisson(float(kind[1:]), n_px)
        yield v.astype(np.int64)


@pytest.fixture(scope="module")
def rings():
    return list(_random_rings(5, 4000))


def test_histogram_form_equals_sort_form(rings):
    """Every random ring through both forms, as values; statuses 0, 1, 2 and 3 all occur, 4 never."""
    seen = {}
    for v in rings:
        frame = v.astype(np.uint16)[None, :] if len(v) else np.zeros((1, 0), np.uint16)
        # a frame of one row of len(v) + 1 pixels whose last pixel is the box: border 200 makes the row's other pixels the ring
        f = np.concatenate([frame, np.zeros((1, 1), np.uint16)], axis=1)
        box = (f.shape[1] - 1, f.shape[1] - 1, 0, 0)
        want = sort_form(f, None, -1, box, 200)
        got = B.from_values(B.ring_values(f, None, -1, box, 200))
        assert got == want, (v, got, want)
        seen[got[-1]] = seen.get(got[-1], 0) + 1
    assert set(seen) == {0, 1, 2, 3}, seen
    assert min(seen[0], seen[2], seen[3]) > 100 and seen[1] >= 5, seen


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_ring_geometry_and_validity_rules(dtype):
    """Boxes at the corners, the edges, as wide as the frame, borders 1, 3 and 16, a mask, max_valid, and for 32-bit pixels 2^24 - 1 and 2^24."""
    rng = np.random.default_rng(8)
    Wf, Hf = 37, 29
    f = rng.poisson(3.0, (Hf, Wf)).astype(dtype)
    f[rng.random((Hf, Wf)) < 0.1] = 700
    if np.dtype(dtype).itemsize == 4:
        f[rng.random((Hf, Wf)) < 0.1] = (1 << 24) - 1
        f[rng.random((Hf, Wf)) < 0.1] = 1 << 24
    mask = (rng.random((Hf, Wf)) > 0.2).astype(np.uint8)
    boxes = [(0, 0, 0, 0), (36, 36, 28, 28), (0, 36, 10, 12), (5, 7, 0, 28), (17, 19, 13, 15), (0, 36, 0, 28), (30, 36, 0, 3), (1, 1, 27, 27)]
    for border in (1, 3, 16):
        for m in (None, mask):
            for mv in (-1, 5, 700):
                got = B.spot_backgrounds(f, m, mv, boxes, border)
                for i, box in enumerate(boxes):
                    want = sort_form(f, m, mv, box, border)
                    assert tuple(int(got[name][i]) for name in B.INTEGER_FIELDS) == want, (border, mv, box)
                    assert got["mean"][i] == (want[6] / want[5] if want[7] == 0 else 0.0)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("spot_background")
    flags = ["-std=c++20", "-Wall", "-Werror", "-I", CSRC, CHECK]
    subprocess.run(["g++", "-O1", *flags, "-o", str(d / "plain")], check=True)
    subprocess.run(["g++", *SANITIZE, *flags, "-o", str(d / "sanitized")], check=True)
    return d


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_model_header_equals_the_oracle(programs, rings, which):
    """The header the kernel compiles, as its own process, on the same rings (and a few histograms no ring of 200 pixels gives)."""
    hists = [B.histogram(v) for v in rings]
    big = np.zeros(256, np.uint32)
    big[7] = 4_000_000_000          # counts near 2^32: the positions and the inlier sum need 64 bits
    hists += [(big, 200_000_000), (np.zeros(256, np.uint32), 0), (np.zeros(256, np.uint32), 9), (np.full(256, 3, np.uint32), 256)]
    text = "".join(" ".join(str(int(c)) for c in bins) + " %d\n" % tail for bins, tail in hists)
    r = subprocess.run([str(programs / which)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(hists)
    for line, (bins, tail) in zip(lines, hists):
        assert tuple(int(t) for t in line.split()) == B.from_histogram(bins, tail), (line, tail)
    short = subprocess.run([str(programs / which)], input="1 2 3\n", capture_output=True, text=True, timeout=60)
    assert short.returncode == 2 and "short" in short.stderr


def test_planted_frames_give_the_planted_boxes():
    """Under the committed oracle (dispersion, connected components, both filters) every planted frame returns its planted box, and the ring
    around it ends in the planted status; the frames built without noise return nothing else."""
    from util import oracle_frame
    seen = set()
    for name, c in cases.cases().items():
        mask = c["mask"] if c["mask"] is not None else np.ones(c["frame"].shape, np.uint8)
        _, _, refl = oracle_frame(c["frame"], mask)
        r = refl.reflections
        boxes = [(int(a), int(b), int(cc), int(d)) for a, b, cc, d in zip(r["x_min"], r["x_max"], r["y_min"], r["y_max"])]
        assert c["box"] in boxes, (name, boxes)
        if c.get("only"):
            assert boxes == [c["box"]], (name, boxes)
        if "box2" in c:
            assert c["box2"] in boxes, (name, boxes)
        got = B.spot_backgrounds(c["frame"], c["mask"], -1, [c["box"]] + ([c["box2"]] if "box2" in c else []), 3)
        assert all(int(s) == c["status"] for s in got["status"]), (name, got)
        if "record" in c:
            assert {k: int(got[k][0]) for k in c["record"]} == c["record"], name
        seen.add(c["status"])
    assert seen == {0, 1, 2, 3}
