"""GPU: the spotfinder driver's pedestal mode (--jungfrau-pedestal PREFIX).  The files it writes from synth:tinydark equal the NumPy truth
(tests/jungfrau_pedestal_oracle.py), byte for byte, with the fold on the GPU and, under --cpu-decode, on the worker threads; the calibration
it writes converts raw data to the same JSON lines on the GPU and on the host; the mode's refusals."""
import json
import os
import subprocess

import numpy as np
import pytest

import jungfrau_pedestal_oracle as P
from ffs_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SPOTFINDER = os.path.join(BIN, "spotfinder")
TOOL = os.path.join(BIN, "ffs_hosttool")
W, H, SEED, N = 300, 200, 7, 48
SUFFIXES = ("count.u32", "sum.u64", "sum_sq.u64", "pedestal.f32", "rms.f32", "ok.u8", "calibration.f32")


def run_with_pipe(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [json.loads(l) for l in f.read().split("\n") if l]
    return proc.returncode, out, err, sorted(lines, key=lambda j: j["file-number"])


@pytest.fixture(scope="module")
def measured(tmp_path_factory):
    """The dark run through the driver, on the GPU (prefix P) and on the worker threads (prefix C), and the truth's files."""
    d = tmp_path_factory.mktemp("jfped")
    old = str(d / "old.f32")
    assert subprocess.run([TOOL, "jfcal", "synth:tinydark", old]).returncode == 0
    ped, fac = synth.jungfrau_calibration(W, H, SEED)
    acc = P.fold(P.zeros(H, W), synth.dark_frames(W, H, SEED, N))
    new_ped, rms, ok = P.planes(*acc[1:])
    cal_ped, cal_fac = P.repedestal(ped, fac, new_ped, ok)
    want = {"count.u32": acc[1].astype("<u4").tobytes(), "sum.u64": acc[2].astype("<u8").tobytes(), "sum_sq.u64": acc[3].astype("<u8").tobytes(),
            "pedestal.f32": new_ped.astype("<f4").tobytes(), "rms.f32": rms.astype("<f4").tobytes(), "ok.u8": ok.astype(np.uint8).tobytes(),
            "calibration.f32": np.concatenate([cal_ped, cal_fac]).astype("<f4").tobytes()}
    runs = {}
    for prefix, extra in (("P", ["-n", "3"]), ("C", ["--cpu-decode", "-n", "3"])):
        runs[prefix] = run_with_pipe([f"synth:tinydark:{N}", "--jungfrau-pedestal", str(d / prefix), "--jungfrau-calibration", old, "--batch", "5", *extra], d)
    return d, want, acc, ok, runs


def test_the_files_equal_the_oracles(measured):
    d, want, acc, ok, runs = measured
    rc, out, err, lines = runs["P"]
    assert rc == 0 and not err, (out, err)
    assert lines == [], "the mode prints no JSON lines"
    for suffix in SUFFIXES:
        assert (d / f"P.{suffix}").read_bytes() == want[suffix], suffix
    words = [int(acc[1][s].sum()) for s in range(3)]
    summary = [l for l in out.split("\n") if l.startswith("Jungfrau pedestals: %d frames" % N)]
    assert len(summary) == 1, out
    assert f"words counted G0 {words[0]} G1 {words[1]} G2 {words[2]}, invalid words {N * W * H - sum(words)};" in summary[0]
    assert f"usable pixels G0 {int(ok[0].sum())} G1 {int(ok[1].sum())} G2 {int(ok[2].sum())} of {W * H}" in summary[0]
    assert "on the GPU" in out


def test_cpu_decode_writes_the_same_files(measured):
    d, want, _, _, runs = measured
    rc, out, err, lines = runs["C"]
    assert rc == 0 and not err and lines == [], (out, err)
    assert "on the worker threads" in out
    for suffix in SUFFIXES:
        assert (d / f"C.{suffix}").read_bytes() == (d / f"P.{suffix}").read_bytes() == want[suffix], suffix


def test_without_an_old_calibration_no_calibration_is_written(measured):
    d = measured[0]
    p = subprocess.run([SPOTFINDER, "synth:tinydark:6", "--jungfrau-pedestal", str(d / "Q")], capture_output=True, text=True, cwd=d)
    assert p.returncode == 0 and not p.stderr, (p.stdout, p.stderr)
    assert (d / "Q.ok.u8").stat().st_size == 3 * W * H and not (d / "Q.calibration.f32").exists()
    acc = P.fold(P.zeros(H, W), synth.dark_frames(W, H, SEED, 6))
    assert (d / "Q.sum_sq.u64").read_bytes() == acc[3].astype("<u8").tobytes()


def test_thresholds_and_the_host_tools_last_step(measured):
    d, _, acc, _, _ = measured
    p = subprocess.run([SPOTFINDER, f"synth:tinydark:{N}", "--jungfrau-pedestal", str(d / "M"), "--jungfrau-calibration", str(d / "old.f32"), "--pedestal-min-frames", "10",
                        "--pedestal-max-rms", "1.25"], capture_output=True, text=True, cwd=d)
    assert p.returncode == 0 and not p.stderr, (p.stdout, p.stderr)
    ped, fac = synth.jungfrau_calibration(W, H, SEED)
    new_ped, rms, ok = P.planes(*acc[1:], min_frames=10, max_rms=1.25)
    assert 0.05 < ok.mean() < 0.95 and ok.mean() < P.planes(*acc[1:])[2].mean()      # (both thresholds bite)
    cal_ped, cal_fac = P.repedestal(ped, fac, new_ped, ok)
    assert (d / "M.ok.u8").read_bytes() == ok.astype(np.uint8).tobytes() and (d / "M.rms.f32").read_bytes() == rms.astype("<f4").tobytes()
    assert (d / "M.calibration.f32").read_bytes() == np.concatenate([cal_ped, cal_fac]).astype("<f4").tobytes()
    assert "(min frames 10, max rms 1.25)" in p.stdout
    # ... and ffs_hosttool does the last step from the statistics files, with no GPU
    assert subprocess.run([TOOL, "jfrepedestal", str(d / "old.f32"), str(d / "P"), str(d / "T.f32"), "10", "1.25"]).returncode == 0
    assert (d / "T.f32").read_bytes() == (d / "M.calibration.f32").read_bytes()


def test_raw_data_under_the_new_calibration_on_the_gpu_and_on_the_host(measured):
    d = measured[0]
    cal = str(d / "P.calibration.f32")
    got = {}
    for name, extra in (("gpu", []), ("cpu", ["--cpu-decode"])):
        rc, out, err, lines = run_with_pipe(["synth:tinyraw:8", "--jungfrau-calibration", cal, "--output-for-index", "--batch", "4", *extra], d)
        assert rc == 0 and not err, (out, err)
        assert len(lines) == 8 and sum(j["n_spots_total"] for j in lines) > 50
        got[name] = lines
    assert got["gpu"] == got["cpu"]


def test_refusals(measured):
    d = measured[0]

    def refused(argv, match):
        p = subprocess.run([SPOTFINDER, *argv], capture_output=True, text=True, cwd=d)
        assert p.returncode == 1 and match in p.stdout, (argv, p.stdout, p.stderr)
        assert not (d / "R.count.u32").exists()

    base = ["synth:tinydark:6", "--jungfrau-pedestal", str(d / "R")]
    refused([*base, "--gpus", "2"], "--jungfrau-pedestal takes one GPU")
    refused([*base, "--devices", "0,1"], "--jungfrau-pedestal takes one GPU")
    refused([*base, "--validate"], "not with --validate")
    refused([*base, "--writeout"], "not with --writeout")
    refused([*base, "--pedestal-min-frames", "0"], "--pedestal-min-frames must be at least 1")
    refused([*base, "--pedestal-max-rms", "-1"], "--pedestal-max-rms takes a finite number")
    refused([*base, "--pedestal-max-rms", "nan"], "--pedestal-max-rms takes a finite number")
    refused(["synth:tinydark:6", "--pedestal-min-frames", "3"], "belong to --jungfrau-pedestal")
    refused(["synth:jungfrau9m:1", "--jungfrau-pedestal", str(d / "R")], "uncompressed frames of 32 bits")
    shm = d / "shm"
    assert subprocess.run([TOOL, "mkshm", "synth:tiny:2", str(shm)]).returncode == 0
    refused([str(shm), "--jungfrau-pedestal", str(d / "R")], "compressed frames of 16 bits")
