"""CPU: the launch geometry of the threshold stage (csrc/launch_geometry.hpp) is plain integer arithmetic in a header without HIP.
tests/launch_geometry_check.cc walks it over a sweep of shapes, pixel sizes, frame strides and tuning values, in its own process
under the address and undefined-behaviour sanitizers.  Checked here: every row equals what the same arithmetic gave while it was
part of make_threshold_args (tests/golden/launch_geometry.json, recorded from that commit's statements); the invariants the kernels
and the buffer sizing rely on hold on every case (the program checks them and says so); and the numbers the GPU tests assume."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_geometry.json")
FLAGS = ["-std=c++20", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
DEFAULT_GROUP, DEFAULT_WAVES = 1 << 30, 16384   # Tuning: frames_per_group, target_waves


def parse(text):
    """The program's lines -> {"stream": {case: [row per n_frames]}, "window": ..., "ext": ...}.  A case is the line's inputs without
    n_frames, its rows come in the order n_frames = 1, 2, ..."""
    kinds = {"S": "stream", "W": "window", "E": "ext"}
    out = {k: {} for k in kinds.values()}
    for line in text.splitlines():
        if line[:2] not in ("S ", "W ", "E "):
            continue
        key, *vals = [part.split() for part in line.split("|")]
        rows = out[kinds[key[0]]].setdefault(" ".join(key[1:-1]), [])
        assert int(key[-1]) == len(rows) + 1, line
        rows.append([[int(v) for v in part] for part in vals])
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("geometry") / "launch_geometry_check"
    subprocess.run(["g++", *FLAGS, "-I", CSRC, os.path.join(ROOT, "tests", "launch_geometry_check.cc"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def geometry(run):
    return parse(run.stdout)


def stream_rows(geometry, W, H, px, group=DEFAULT_GROUP, waves=DEFAULT_WAVES, bands=0, taper=0):
    """[(group_frames, n_groups, n_strips, n_bands, band_rows, band_rows2, band_split), (sub, sub_rows, plan holds)] per n_frames,
    frames at the default stride"""
    pitch = (W + 127) // 128 * 128 * px
    return geometry["stream"][f"{W} {H} {px} {pitch * H} {group} {waves} {bands} {taper}"]


def test_invariants_hold_and_sanitizers_are_clean(run):
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])


def test_every_row_equals_the_arithmetic_it_was_moved_from(geometry):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sum(len(rows) for cases in geometry.values() for rows in cases.values()) > 5000
    for kind in ("stream", "window", "ext"):
        assert geometry[kind].keys() == golden[kind].keys()
        for case, rows in geometry[kind].items():
            assert [r[0] for r in rows] == golden[kind][case], (kind, case)


def test_the_geometries_the_gpu_tests_assume(run, geometry):
    split = {}                                 # band height -> (sub-bands, rows of each)
    for line in run.stdout.splitlines():
        if line.startswith("B "):
            _, rows, _, sub, sub_rows = line.split()
            split[int(rows)] = (int(sub), int(sub_rows))
    assert [split[r] for r in (150, 173, 104, 100)] == [(2, 75), (2, 87), (2, 52), (2, 50)]
    assert [split[r] for r in (75, 74, 50, 47, 96)] == [(1, 75), (1, 74), (1, 50), (1, 47), (1, 96)]
    assert split[97] == (2, 49) and split[1024] == (11, 94)


    def at(n_frames, W, H, **tuning):
        (_, _, strips, bands, rows, rows2, split), (sub, sub_rows, holds) = stream_rows(geometry, W, H, 2, **tuning)[n_frames - 1]
        return dict(strips=strips, bands=bands, rows=rows, rows2=rows2, split=split, sub=sub, sub_rows=sub_rows, holds=holds)

    g = at(3, 640, 1800)                       # tests/batch_walk.py: 24 bands of 75 rows
    assert (g["strips"], g["bands"], g["rows"], g["rows2"], g["split"], g["sub"]) == (4, 24, 75, 75, 24, 1)
    g = at(5, 1000, 300, waves=22)             # test_gpu_bands.py: two streaming bands of 150 rows, each cut in two
    assert (g["strips"], g["bands"], g["rows"], g["split"], g["sub"], g["sub_rows"]) == (11, 2, 150, 2, 2, 75)
    g = at(5, 1203, 517, waves=40)             # ... three of 173 (the last 171), each cut in two
    assert (g["strips"], g["bands"], g["rows"], g["split"], g["sub"], g["sub_rows"]) == (13, 3, 173, 3, 2, 87)
    assert 517 - 2 * 173 == 171
    g = at(2, 700, 2400, taper=50)             # ... tapered: 16 bands of 100 rows (cut in two), then 16 of 50
    assert (g["strips"], g["rows"], g["rows2"], g["split"], g["bands"], g["sub"], g["sub_rows"]) == (3, 100, 50, 16, 32, 2, 50)
    for n_frames in range(1, 9):               # ... tuning stream_bands: any number of bands, whatever the batch
        for bands, rows, sub in ((3, 173, 2), (5, 104, 2), (7, 74, 1), (11, 47, 1)):
            g = at(n_frames, 1203, 517, bands=bands)
            assert (g["bands"], g["rows"], g["rows2"], g["sub"], g["holds"]) == (bands, rows, rows, sub, 1)
