"""GPU: the spotfinder driver on raw Jungfrau words (--jungfrau-calibration FILE).  Its JSON lines are those of the Python pipeline on the
frames the NumPy truth (tests/jungfrau_oracle.py) converts the same words to -- with the conversion on the GPU and, under --cpu-decode, on
the worker threads; the flag decides, not the source's name; a compressed source is refused."""
import json
import os
import subprocess

import numpy as np
import pytest

import jungfrau_oracle as J
from ffs_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SPOTFINDER = os.path.join(BIN, "spotfinder")
TOOL = os.path.join(BIN, "ffs_hosttool")
N = 6
TOP = (1 << 24) - 1


def run_with_pipe(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [json.loads(l) for l in f.read().split("\n") if l]
    return proc.returncode, out, err, sorted(lines, key=lambda j: j["file-number"])


@pytest.fixture(scope="module")
def calibration(tmp_path_factory):
    d = tmp_path_factory.mktemp("jf")
    path = d / "cal.f32"
    assert subprocess.run([TOOL, "jfcal", "synth:tinyraw:1", str(path)]).returncode == 0
    ped, fac = synth.jungfrau_calibration(300, 200, 7)
    assert np.array_equal(np.fromfile(path, "<f4").reshape(6, 200, 300), np.concatenate([ped, fac]))
    return d, str(path), ped, fac


def python_pipeline(ffs, frames, max_valid):
    """(strong pixels, spots, spot centres) per frame, from 32-bit frames through the binding with the driver's defaults."""
    ctx = ffs.Context(300, 200, np.uint32, max_batch=len(frames))
    ctx.set_params(max_valid=max_valid)
    out = []
    for r in ctx.stream().process(frames):
        centres = np.stack([r.reflections["com_x"], r.reflections["com_y"], r.reflections["com_z"]], 1).reshape(-1)
        out.append((r.num_strong_pixels, len(r.boxes), centres))
    return out


def assert_lines(lines, want, source):
    assert [j["file-number"] for j in lines] == list(range(len(want)))
    for j, (n_strong, n_spots, centres) in zip(lines, want):
        assert j["file"] == source
        assert (j["num_strong_pixels"], j["n_spots_total"]) == (n_strong, n_spots), j["file-number"]
        np.testing.assert_array_equal(np.array(j["spot_centers"], np.float32), centres.astype(np.float32))


def test_raw_words_on_the_gpu_and_on_the_host(ffs, calibration):
    d, path, ped, fac = calibration
    raw = synth.raw_frames(synth.tiny_params(7, np.uint32), range(N))
    frames = J.convert(raw, ped, fac)
    assert (frames == J.INVALID).sum() > N and (frames[frames != J.INVALID] > 300).sum() > 100
    want = python_pipeline(ffs, frames, TOP)
    assert sum(w[1] for w in want) > 50
    source = "synth:tinyraw:%d" % N
    runs = {}
    for name, extra, where in (("gpu", [], "on the GPU"), ("cpu", ["--cpu-decode"], "on the worker threads")):
        rc, out, err, lines = run_with_pipe([source, "--jungfrau-calibration", path, "--output-for-index", "--batch", "4", *extra], d)
        assert rc == 0 and not err, (out, err)
        named = [l for l in out.split("\n") if l.startswith("Jungfrau calibration:")]
        assert len(named) == 1 and path in named[0] and where in named[0], (name, named)
        assert "Trusted range: centre pixels above 16777215 are not spots" in out
        assert_lines(lines, want, source)
        runs[name] = lines
    assert runs["gpu"] == runs["cpu"]


def test_the_flag_decides_not_the_source(ffs, calibration):
    """synth:tiny hands over 16-bit PHOTON frames; with the flag they are taken as raw words all the same (mostly G0 near ADC 0)."""
    d, path, ped, fac = calibration
    words = synth.frames(synth.tiny_params(7), range(N), threads=2)
    assert words.dtype == np.uint16
    frames = J.convert(words, ped, fac)
    want = python_pipeline(ffs, frames, 65535)        # min(the source's trusted maximum, 2^24 - 1)
    rc, out, err, lines = run_with_pipe(["synth:tiny:%d" % N, "--jungfrau-calibration", path, "--output-for-index"], d)
    assert rc == 0 and not err, (out, err)
    assert "Jungfrau calibration:" in out and "centre pixels above 65535" in out
    assert_lines(lines, want, "synth:tiny:%d" % N)
    # ... and without the flag nothing changes: 16-bit photon counts
    rc, out, err, plain = run_with_pipe(["synth:tiny:%d" % N, "--output-for-index"], d)
    assert rc == 0 and not err and "Jungfrau" not in out
    ctx = ffs.Context(300, 200, np.uint16, max_batch=N)
    for j, r in zip(plain, ctx.stream().process(words)):
        assert (j["num_strong_pixels"], j["n_spots_total"]) == (r.num_strong_pixels, len(r.boxes))


def test_a_stream_directory_is_refused(calibration):
    d, path, _, _ = calibration
    shm = d / "shm"
    assert subprocess.run([TOOL, "mkshm", "synth:tiny:2", str(shm)]).returncode == 0
    p = subprocess.run([SPOTFINDER, str(shm), "--jungfrau-calibration", path], capture_output=True, text=True, cwd=d)
    assert p.returncode == 1
    assert "--jungfrau-calibration: raw Jungfrau words are uncompressed 16-bit frames" in p.stdout and "compressed frames of 16 bits" in p.stdout
