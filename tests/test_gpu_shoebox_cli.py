"""GPU: the driver with --integrate on the smallest synthetic sweep source and a shoebox file written here, centres on and between
pixels.  PREFIX.shoebox_sums must be byte for byte what `ffs_hosttool shoebox` -- csrc/shoebox_model.hpp on the CPU -- writes for the same
frames, file and geometry; the summary line's four counts must be those of tests/shoebox_oracle.py over the s1 and phi that
`ffs_hosttool shoeboxgeom` (the driver's own text, host/shoebox_geometry.hpp) gives; --integrate without --sigma-b is a usage error."""
import os
import re
import subprocess

import numpy as np
import pytest

import shoebox_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SPOTFINDER, HOSTTOOL = os.path.join(BIN, "spotfinder"), os.path.join(BIN, "ffs_hosttool")
W, H, N = 300, 200, 8
RECORD_DT = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("box", "<i4", (6,))])
SUMMARY = re.compile(r"shoeboxes: (\d+) boxes, (\d+) with foreground, (\d+) FG_INVALID, (\d+) background failures")


def shoebox_file(path):
    rng = np.random.default_rng(31)
    rows = [(120.0, 80.0, 4.0, (114, 127, 74, 87, 2, 6)),            # the centre on a corner and on an image's edge
            (60.5, 40.5, 3.5, (55, 67, 35, 47, 1, 6)),               # in the middle of a pixel and of an image
            (200.25, 150.75, 2.1, (190, 211, 145, 157, 0, 5)),       # between
            (1.5, 100.5, 3.5, (-4, 8, 95, 107, 2, 5)),               # over the left edge: FG_INVALID
            (298.5, 198.5, 6.5, (293, 305, 193, 205, 5, 9)),         # over a corner and past the last image
            (100.5, 20.5, 3.5, (140, 150, 15, 27, 2, 5)),            # the centre far from its box: no foreground
            (100.5, 60.5, 20.5, (95, 107, 55, 67, 19, 23))]          # no image of the run
    for _ in range(50):
        x, y, z = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0, N)
        hx, hy, hz = rng.integers(2, 8), rng.integers(2, 8), rng.integers(1, 3)
        ix, iy, iz = int(x), int(y), int(z)
        rows.append((x, y, z, (ix - hx, ix + hx + 1, iy - hy, iy + hy + 1, iz - hz, iz + hz + 1)))
    rec = np.array(rows, RECORD_DT)
    assert rec.itemsize == 48
    rec.tofile(path)
    return rec


def run(argv, cwd):
    r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, timeout=300)
    return r.returncode, re.sub(r"\x1b\[[0-9;]*m", "", r.stdout), r.stderr


@pytest.mark.parametrize("algorithm,background", [("ellipsoid", "tukey"), ("dials", "glm")])
def test_driver_writes_what_the_host_tool_writes(tmp_path, algorithm, background):
    source = f"synth:tinysweep:{N}"
    rec = shoebox_file(tmp_path / "boxes.bin")
    sigmas = ["--sigma-b", "0.01", "--sigma-m", "0.04"]
    rc, out, err = run([SPOTFINDER, source, "--threads", "1", "--batch", "3", "--single-buffer", "--max-valid", "none", "--integrate", "boxes.bin", *sigmas,
                        "--integrate-algorithm", algorithm, "--integrate-background", background, "--integrate-out", "run"], tmp_path)
    assert rc == 0 and not err, (out[-3000:], err)
    geometry_words = re.search(r"Integration geometry: (.*)", out).group(1).split()
    assert len(geometry_words) == 8
    rc, _, err = run([HOSTTOOL, "synthframes", source, "frames.bin"], tmp_path)
    assert rc == 0, err
    rc, tool_out, err = run([HOSTTOOL, "shoebox", "frames=frames.bin", f"width={W}", f"height={H}", "bytes=2", *geometry_words, "boxes=boxes.bin", "sigma_b=0.01",
                             "sigma_m=0.04", f"algorithm={algorithm}", f"background={background}", "out=tool.shoebox_sums"], tmp_path)
    assert rc == 0, (tool_out, err)
    got, want = (tmp_path / "run.shoebox_sums").read_bytes(), (tmp_path / "tool.shoebox_sums").read_bytes()
    assert len(got) == len(rec) * O.SUM_DT.itemsize and got == want
    # the summary line against the oracle, over the driver's own s1 and phi
    rc, geom_out, err = run([HOSTTOOL, "shoeboxgeom", *geometry_words, "boxes=boxes.bin"], tmp_path)
    assert rc == 0, err
    lines = geom_out.splitlines()
    words = np.array([int(w, 16) for w in lines[0].split()], np.uint64).view(np.float64)
    g = O.geometry(words[0:9], words[9:11], words[11], words[12:15], words[15:18], words[18], words[19])
    kv = {w.split("=")[0]: float(w.split("=")[1]) for w in geometry_words}
    flat = O.flat_geometry(kv["distance"], kv["beam_x"], kv["beam_y"], kv["pixel_x"], kv["pixel_y"], kv["wavelength"], kv["osc_start"], kv["osc_width"])
    assert all(np.array_equal(np.asarray(g[k]), np.asarray(flat[k])) for k in g)          # the driver's flat panel is the oracle's
    boxes = np.zeros(len(rec), O.BOX_DT)
    for i, line in enumerate(lines[1:]):
        v = np.array([int(w, 16) for w in line.split()], np.uint64).view(np.float64)
        boxes["s1"][i], boxes["phi"][i] = v[:3], v[3]
    for k, name in enumerate(("x_min", "x_max", "y_min", "y_max", "z_min", "z_max")):
        boxes[name] = rec["box"][:, k]
    frames = np.fromfile(tmp_path / "frames.bin", np.uint16).reshape(N, H, W)
    # (delta = n_sigma * sigma * (pi / 180), multiplied in that order, as host/shoebox_geometry.hpp does)
    acc = O.fold(g, boxes, O.DIALS if algorithm == "dials" else O.ELLIPSOID, 3.0 * 0.01 * (np.pi / 180.0), 3.0 * 0.04 * (np.pi / 180.0), frames, 0, None, -1,
                 O.new_accumulators(len(boxes)))
    records = O.sums(acc, background)
    O.assert_records_equal(np.frombuffer(got, O.SUM_DT), records, "the driver's records")
    counts = O.summary_counts(records)
    assert tuple(int(v) for v in SUMMARY.search(out).groups()) == counts == tuple(int(v) for v in SUMMARY.search(tool_out).groups())
    assert counts[0] == len(rec) and 0 < counts[1] < counts[0] and counts[2] > 0


def test_integrate_without_sigma_b_is_a_usage_error(tmp_path):
    shoebox_file(tmp_path / "boxes.bin")
    rc, out, err = run([SPOTFINDER, "synth:tinysweep:4", "--integrate", "boxes.bin", "--sigma-m", "0.04", "--integrate-out", "run"], tmp_path)
    assert rc != 0 and "--integrate needs both --sigma-b and --sigma-m" in out
    assert not (tmp_path / "run.shoebox_sums").exists()
