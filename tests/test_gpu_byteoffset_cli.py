"""GPU: the spotfinder driver on miniCBF files -- the binary sections go to the GPU as they lie in the files (byte-offset decode on
the device) unless --cpu-decode asks for the host decoder; both give the same JSON lines, and --validate agrees image by image."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SPOTFINDER = os.path.join(BIN, "spotfinder")
TOOL = os.path.join(BIN, "ffs_hosttool")
N = 4
DET = json.dumps({"pixel_size_x": 0.075, "pixel_size_y": 0.075, "beam_center_x": 11.25, "beam_center_y": 7.5, "distance": 300.0})


def run_with_pipe(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, out, err, lines


@pytest.fixture(scope="module")
def cbf_argv(tmp_path_factory):
    d = tmp_path_factory.mktemp("cbf")
    assert subprocess.run([TOOL, "mkcbf", "synth:tiny:%d" % N, str(d / "img_")]).returncode == 0
    return d, [str(d / "img_####.cbf"), "--images", str(N), "--start-index", "1", "--wavelength", "0.976", "--detector", DET]


def test_gpu_decode_equals_cpu_decode(cbf_argv):
    d, argv = cbf_argv
    runs = {}
    for name, extra, depth in (("gpu", [], "four batches in flight per GPU"), ("cpu", ["--cpu-decode"], "three batches in flight per GPU")):
        rc, out, err, lines = run_with_pipe(argv + extra, d)
        assert rc == 0 and not err, (out, err)
        batches = [l for l in out.split("\n") if l.startswith("GPU batches:")]
        assert len(batches) == 1 and depth in batches[0], (name, batches)
        runs[name] = sorted((json.loads(l) for l in lines), key=lambda j: j["file-number"])
    assert [j["file-number"] for j in runs["gpu"]] == list(range(N))
    assert runs["gpu"] == runs["cpu"]
    assert sum(j["num_strong_pixels"] for j in runs["gpu"]) > 0


def test_validate(cbf_argv):
    d, argv = cbf_argv
    rc, out, err, _ = run_with_pipe(argv + ["--validate"], d)
    txt = re.sub(r"\x1b\[[0-9;]*m", "", out)
    assert rc == 0 and not err, (out, err)
    assert "four batches in flight per GPU" in txt
    matches = re.findall(r"Image\s+(\d+): Compared: Match (\d+) px", txt)
    assert sorted(int(a) for a, _ in matches) == list(range(N)) and "Mismatch" not in txt
