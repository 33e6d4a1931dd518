"""GPU: the driver with --predict on the smallest synthetic sweep source and a crystal file written here.  PREFIX.predictions must be byte
for byte what `ffs_hosttool predict` -- csrc/predict_model.hpp on the CPU -- writes for the printed geometry, PREFIX.shoebox_sums byte for
byte what `ffs_hosttool shoebox` writes for the boxes taken from PREFIX.predictions; the three usage errors exit non-zero and name the
flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import predict_cases as K
import predict_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SPOTFINDER, HOSTTOOL = os.path.join(BIN, "spotfinder"), os.path.join(BIN, "ffs_hosttool")
N = 8
SUMMARY = re.compile(r"prediction: (\d+) candidates, (\d+) predictions, (\d+) flagged")
SIGMAS = ["--sigma-b", "0.01", "--sigma-m", "0.04"]


def crystal_file(path):
    """The panel of the tiny sweep subtends a degree at 300 mm, so only reflections beyond 25 A meet it: a cell of 300 x 310 x 320 A puts
    a few tens of them into the eight images of 0.1 deg."""
    K.a_matrix((300.0, 310.0, 320.0), 5).astype("<f8").tofile(path)


def run(argv, cwd):
    r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, timeout=300)
    return r.returncode, re.sub(r"\x1b\[[0-9;]*m", "", r.stdout), r.stderr


def test_driver_writes_what_the_host_tool_writes(tmp_path):
    source = f"synth:tinysweep:{N}"
    crystal_file(tmp_path / "crystal.bin")
    rc, out, err = run([SPOTFINDER, source, "--predict", "crystal.bin", "--predict-dmin", "2", *SIGMAS, "--integrate-out", "run", "--threads", "1", "--batch", "3",
                        "--single-buffer", "--max-valid", "none"], tmp_path)
    assert rc == 0 and not err, (out[-3000:], err)
    geometry_words = re.search(r"Integration geometry: (.*)", out).group(1).split()
    scan_words = re.search(r"Prediction scan: (.*)", out).group(1).split()
    assert len(geometry_words) == 8 and scan_words == ["width=300", "height=200", f"n_images={N}"]
    rc, tool_out, err = run([HOSTTOOL, "predict", *geometry_words, *scan_words, "crystal=crystal.bin", "dmin=2", "sigma_b=0.01", "sigma_m=0.04",
                             "out=tool.predictions"], tmp_path)
    assert rc == 0, (tool_out, err)
    got, want = (tmp_path / "run.predictions").read_bytes(), (tmp_path / "tool.predictions").read_bytes()
    assert got == want
    pred = np.frombuffer(got, O.PREDICTION_DT)
    counts = tuple(int(v) for v in SUMMARY.search(out).groups())
    assert counts == tuple(int(v) for v in SUMMARY.search(tool_out).groups())
    assert counts[1] == len(pred) > 10 and counts[2] == int(np.count_nonzero(pred["flags"] & ~np.uint32(O.ENTERING)))
    assert np.all((0 <= pred["x_px"]) & (pred["x_px"] < 300) & (0 <= pred["y_px"]) & (pred["y_px"] < 200) & (0 <= pred["z"]) & (pred["z"] < N))
    rc, _, err = run([HOSTTOOL, "synthframes", source, "frames.bin"], tmp_path)
    assert rc == 0, err
    rc, tool_out, err = run([HOSTTOOL, "shoebox", "frames=frames.bin", "width=300", "height=200", "bytes=2", *geometry_words, "predictions=run.predictions",
                             "sigma_b=0.01", "sigma_m=0.04", "out=tool.shoebox_sums"], tmp_path)
    assert rc == 0, (tool_out, err)
    sums, want = (tmp_path / "run.shoebox_sums").read_bytes(), (tmp_path / "tool.shoebox_sums").read_bytes()
    kept = int(np.count_nonzero((pred["flags"] & O.BOX_REFUSED) == 0))
    assert len(sums) == 80 * kept and kept > 10 and sums == want
    assert f"Integration: {kept} reflections from the prediction" in out


@pytest.mark.parametrize("argv,needle", [
    (["--predict", "crystal.bin", "--predict-dmin", "2", *SIGMAS, "--integrate", "boxes.bin", "--integrate-out", "run"], "--predict and --integrate"),
    (["--predict", "crystal.bin", *SIGMAS, "--integrate-out", "run"], "--predict needs --predict-dmin"),
    (["--predict", "crystal.bin", "--predict-dmin", "2", "--sigma-m", "0.04", "--integrate-out", "run"], "--predict needs both --sigma-b and --sigma-m"),
], ids=["with-integrate", "without-dmin", "without-sigma-b"])
def test_the_usage_errors_name_the_flag(tmp_path, argv, needle):
    crystal_file(tmp_path / "crystal.bin")
    rc, out, err = run([SPOTFINDER, "synth:tinysweep:4", *argv], tmp_path)
    assert rc != 0 and needle in out
    assert not (tmp_path / "run.predictions").exists() and not (tmp_path / "run.shoebox_sums").exists()
