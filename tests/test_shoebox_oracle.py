"""CPU: the NumPy statement of summation integration (tests/shoebox_oracle.py) tied to (a) an independent per-pixel, per-corner loop in
Python floats and integers, (b) csrc/shoebox_model.hpp run as a plain C++ program over the same inputs -- built with g++
-ffp-contract=off, plain and under the address and undefined-behaviour sanitizers -- bit for bit on every integer, on the records and on
the foreground maps, and (c) cases that can be checked by hand.  The inputs are four random geometries with 500 random boxes each on
frames of 96 x 80 pixels, 16 and 32 bits, both algorithms; the census test asserts on the oracle alone that they contain everything the
rule distinguishes."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import shoebox_cases as K
import shoebox_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "shoebox_check.cc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
N_IMAGES, N_BOXES = 8, 500
#            dtype      algorithm    max_valid  mask
SCENARIOS = [(np.uint16, O.ELLIPSOID, 60000, True), (np.uint16, O.DIALS, -1, True), (np.uint32, O.ELLIPSOID, -1, True), (np.uint32, O.DIALS, 1000000, False)]


def scenario(k):
    dtype, algorithm, max_valid, masked = SCENARIOS[k]
    rng = np.random.default_rng(4200 + k)
    g = K.random_geometry(rng)
    return dict(g=g, algorithm=algorithm, max_valid=max_valid, frames=K.frames(rng, dtype, N_IMAGES), mask=K.mask(rng) if masked else None,
                boxes=K.random_boxes(rng, g, N_BOXES, N_IMAGES), delta_b=2.0 * K.pixel_angle(g), delta_m=float(g["osc_width_deg"] * O.DEG))


@pytest.fixture(scope="module")
def folded():
    """The four scenarios with the oracle's accumulators and census, computed once."""
    out = []
    for k in range(len(SCENARIOS)):
        s = scenario(k)
        s["census"] = {}
        s["acc"] = O.fold(s["g"], s["boxes"], s["algorithm"], s["delta_b"], s["delta_m"], s["frames"], 0, s["mask"], s["max_valid"],
                          O.new_accumulators(len(s["boxes"])), s["census"])
        out.append(s)
    return out


def test_the_fixtures_contain_everything_the_rule_distinguishes(folded):
    total = lambda name: sum(s["census"].get(name, 0) for s in folded)
    boxes_with = lambda name: sum(len(s["census"].get(name, ())) for s in folded)
    assert total("foreground") > 1000 and total("background") > 1000 and total("overflow") > 10
    for cause in ("edge", "mask", "max_valid", "ge_2_24"):
        assert boxes_with(cause) > 0, cause
    assert sum(int(np.sum((np.array(s["acc"]["fg_count"]) == 0) & (s["acc"]["hist"].sum(axis=1) > 0))) for s in folded) > 0, "boxes without foreground"
    assert sum(len(s["boxes"]) for s in folded) == 2000


# ---- (a) an independent loop: one pixel, one corner, one image at a time, Python floats --------------------------------------------------
def slow_box(s, b):
    g = s["g"]
    D, px, lam = [float(v) for v in g["d_matrix"]], [float(v) for v in g["pixel_size_mm"]], float(g["wavelength"])
    s0, axis = [float(v) for v in g["s0"]], [float(v) for v in g["rot_axis"]]
    s1, phi = [float(v) for v in b["s1"]], float(b["phi"])
    dot = lambda a, c: (a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]
    cross = lambda a, c: [a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]]

    def unit(v):
        n = math.sqrt(dot(v, v))
        return [v[0] / n, v[1] / n, v[2] / n]
    e1 = unit(cross(s1, s0))
    e2 = unit(cross(s1, e1))
    length, zeta = math.sqrt(dot(s1, s1)), dot(axis, e1)
    ib, im = 1.0 / (s["delta_b"] * s["delta_b"]), 1.0 / (s["delta_m"] * s["delta_m"])
    to_rad = math.pi / 180.0
    start, width = float(g["osc_start_deg"]), float(g["osc_width_deg"])

    def corner(cx, cy, n):
        x, y = float(cx) * px[0], float(cy) * px[1]
        L = [(D[3 * i] * x + D[3 * i + 1] * y) + D[3 * i + 2] for i in range(3)]
        norm = math.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
        d = [(L[i] / norm) / lam - s1[i] for i in range(3)]
        eps1, eps2 = dot(e1, d) / length, dot(e2, d) / length
        xy = (eps1 * eps1 + eps2 * eps2) * ib
        if s["algorithm"] == O.DIALS:
            return xy <= 1.0
        low, high = (start + float(n) * width) * to_rad, (start + float(n + 1) * width) * to_rad
        for e3 in (zeta * (low - phi), zeta * (high - phi)):
            if xy + (e3 * e3) * im <= 1.0:
                return True
        return phi >= low and phi <= high and xy + (0.0 * 0.0) * im <= 1.0
    frames, mask, max_valid = s["frames"], s["mask"], s["max_valid"]
    r = dict(fg_sum=0, fg_count=0, m_x=0, m_y=0, m_z=0, n_overflow=0, flags=0, hist=[0] * 256)
    for n in range(max(int(b["z_min"]), 0), min(int(b["z_max"]), len(frames))):
        for y in range(int(b["y_min"]), int(b["y_max"])):
            for x in range(int(b["x_min"]), int(b["x_max"])):
                fg = corner(x, y, n) or corner(x + 1, y, n) or corner(x, y + 1, n) or corner(x + 1, y + 1, n)
                counts = 0 <= x < K.W and 0 <= y < K.H
                p = int(frames[n, y, x]) if counts else 0
                counts = counts and (mask is None or mask[y, x] != 0) and (max_valid < 0 or p <= max_valid) and (frames.dtype.itemsize == 2 or p < 1 << 24)
                if fg and counts:
                    r["fg_sum"] += p
                    r["fg_count"] += 1
                    r["m_x"] += p * (2 * x + 1)
                    r["m_y"] += p * (2 * y + 1)
                    r["m_z"] += p * (2 * n + 1)
                elif fg:
                    r["flags"] |= O.FG_INVALID
                elif counts and p < 256:
                    r["hist"][p] += 1
                elif counts:
                    r["n_overflow"] += 1
    return r


@pytest.mark.parametrize("k", range(len(SCENARIOS)))
def test_oracle_against_a_per_pixel_per_corner_loop(folded, k):
    s = folded[k]
    for i in range(0, N_BOXES, 4):   # (every fourth box: the loop is Python, a corner at a time)
        want = slow_box(s, s["boxes"][i])
        for name in ("fg_sum", "fg_count", "m_x", "m_y", "m_z", "n_overflow", "flags"):
            assert int(s["acc"][name][i]) == want[name], (k, i, name)
        assert list(s["acc"]["hist"][i]) == want["hist"], (k, i)


# ---- (b) the header as a C++ program ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("shoebox")
    flags = ["-std=c++20", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, CHECK]
    subprocess.run(["g++", "-O2", *flags, "-o", str(d / "plain")], check=True)
    subprocess.run(["g++", "-O1", *SANITIZE, *flags, "-o", str(d / "sanitized")], check=True)
    return d


def geometry_bytes(g):
    return np.concatenate([g["d_matrix"], g["pixel_size_mm"], [g["wavelength"]], g["s0"], g["rot_axis"], [g["osc_start_deg"], g["osc_width_deg"]]]).astype("<f8").tobytes()


def run_header(program, s, background, work):
    frames = s["frames"]
    head = struct.pack("<8i2q2d", K.W, K.H, frames.dtype.itemsize, len(frames), len(s["boxes"]), s["algorithm"], int(s["mask"] is not None), background,
                       s["max_valid"], 0, s["delta_b"], s["delta_m"])
    src, dst = work / "in.bin", work / "out.bin"
    src.write_bytes(head + geometry_bytes(s["g"]) + s["boxes"].tobytes() + (s["mask"].tobytes() if s["mask"] is not None else b"") + frames.tobytes())
    r = subprocess.run([str(program), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    raw = dst.read_bytes()
    per_box = np.dtype([("acc", "<u8", (4,)), ("acc32", "<u4", (4,)), ("hist", "<u4", (256,)), ("sum", O.SUM_DT)])
    assert per_box.itemsize == 48 + 1024 + 80
    n = len(s["boxes"])
    return np.frombuffer(raw[:n * per_box.itemsize], per_box), np.frombuffer(raw[n * per_box.itemsize:], np.uint8)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("k", range(len(SCENARIOS)))
def test_header_program_agrees_bit_for_bit(folded, programs, tmp_path, k, build):
    s = folded[k]
    background = k % 2   # (Tukey for the even scenarios, GLM for the odd ones)
    got, maps = run_header(programs / build, s, background, tmp_path)
    acc = s["acc"]
    for j, name in enumerate(("fg_sum", "m_x", "m_y", "m_z")):
        assert np.array_equal(got["acc"][:, j], np.array(acc[name], np.uint64)), (k, name)
    for j, name in enumerate(("fg_count", "n_overflow", "flags")):
        assert np.array_equal(got["acc32"][:, j], np.array(acc[name], np.uint32)), (k, name)
    assert np.array_equal(got["hist"], acc["hist"].astype(np.uint32)), k
    O.assert_records_equal(got["sum"], O.sums(acc, "glm" if background else "tukey"), f"scenario {k}")
    want_maps = []
    for b in s["boxes"]:
        images = range(max(int(b["z_min"]), 0), min(int(b["z_max"]), N_IMAGES))
        m = O.foreground_maps(s["g"], b, s["algorithm"], s["delta_b"], s["delta_m"], images)
        want_maps += [m[n].astype(np.uint8).ravel() for n in images]
    assert np.array_equal(maps, np.concatenate(want_maps)), k


# ---- (c) by hand ----------------------------------------------------------------------------------------------------------------------------
def flat():
    return O.flat_geometry(200.0, 48.0, 40.0, 0.1, 0.1, 1.0, 10.0, 0.2)


def maps_of(g, b, algorithm, delta_b, delta_m):
    return O.foreground_maps(g, b, algorithm, delta_b, delta_m, range(int(b["z_min"]), int(b["z_max"])))


@pytest.mark.parametrize("algorithm", [O.ELLIPSOID, O.DIALS])
def test_a_tiny_delta_b_leaves_the_corners_next_to_the_centre(algorithm):
    g = flat()
    one_pixel = K.pixel_angle(g)
    # the centre in the middle of pixel (30, 20): its four corners are 0.71 pixels away, the next ones 1.58 -- at 1.0 pixel the foreground
    # is the 3 x 3 block of pixels that touch one of the four
    b = K.box(g, 30.5, 20.5, 1.5, 25, 36, 15, 26, 1, 2)
    fg = maps_of(g, b, algorithm, 1.0 * one_pixel, 1.0)[1]
    want = np.zeros((11, 11), bool)
    want[4:7, 4:7] = True
    assert np.array_equal(fg, want)
    # the centre ON the corner (30, 20): at 0.5 pixels that corner alone, and the 2 x 2 pixels around it
    b = K.box(g, 30.0, 20.0, 1.5, 25, 36, 15, 26, 1, 2)
    fg = maps_of(g, b, algorithm, 0.5 * one_pixel, 1.0)[1]
    want = np.zeros((11, 11), bool)
    want[4:6, 4:6] = True
    assert np.array_equal(fg, want)


@pytest.mark.parametrize("algorithm", [O.ELLIPSOID, O.DIALS])
def test_a_large_delta_b_makes_every_pixel_foreground(algorithm):
    g = flat()
    b = K.box(g, 30.5, 20.5, 1.5, 20, 41, 12, 29, 0, 3)
    for fg in maps_of(g, b, algorithm, 100.0 * K.pixel_angle(g), 1.0).values():
        assert fg.all()


def test_dials_ignores_z():
    g = flat()
    b = K.box(g, 30.5, 20.5, 1.5, 25, 36, 15, 26, 0, 40)   # images far from phi among them
    m = maps_of(g, b, O.DIALS, 2.0 * K.pixel_angle(g), 1e-6)
    assert m[0].any() and all(np.array_equal(m[0], v) for v in m.values())
    # the ellipsoid with the same delta_b and a delta_m nothing passes keeps only the image that holds phi
    e = maps_of(g, b, O.ELLIPSOID, 2.0 * K.pixel_angle(g), 1e-6)
    assert [n for n, v in e.items() if v.any()] == [1] and np.array_equal(e[1], m[1])


def test_centre_holds_on_exactly_one_image_of_three():
    g = flat()
    b = K.box(g, 30.5, 20.5, 1.5, 25, 36, 15, 26, 0, 3)
    fr = O.kabsch_frame(g, b["s1"], b["phi"])
    assert [O.image_terms(g, fr, n, 1.0)[3] for n in range(3)] == [False, True, False]
    # a delta_m far below half an image's width: both edges of every image fail, the centre term alone lets image 1 through
    m = maps_of(g, b, O.ELLIPSOID, 2.0 * K.pixel_angle(g), 1e-3 * float(g["osc_width_deg"] * O.DEG))
    assert [bool(m[n].any()) for n in range(3)] == [False, True, False]
    # phi exactly on an image's phi_low is also its predecessor's phi_high: centre holds on both
    b2 = K.box(g, 30.5, 20.5, 2.0, 25, 36, 15, 26, 0, 4)
    fr2 = O.kabsch_frame(g, b2["s1"], b2["phi"])
    assert [O.image_terms(g, fr2, n, 1.0)[3] for n in range(4)] == [False, True, True, False]


def test_final_sums_follow_the_integrator():
    acc = O.new_accumulators(3)
    acc["hist"][0, 3], acc["hist"][0, 4] = 40, 60           # background mean 3.6 under the Tukey fence
    acc["fg_sum"][0], acc["fg_count"][0] = 500, 10
    acc["fg_sum"][1], acc["fg_count"][1] = 77, 5            # no background pixels: status 1, b = 0
    acc["hist"][2, 2] = 30                                  # no foreground
    r = O.sums(acc, "tukey")
    assert r["bg_mean"][0] == 3.6 and r["intensity"][0] == 500.0 - 36.0 and r["variance"][0] == 464.0 + 36.0 * (1.0 + 10.0 / 100.0)
    assert (r["bg_status"][1], r["bg_mean"][1], r["intensity"][1], r["variance"][1]) == (1, 0.0, 77.0, 77.0)
    assert (r["intensity"][2], r["variance"][2], r["n_background"][2]) == (0.0, -1.0, 30)
