"""GPU: the driver with --index-basis ... --index-assign on the smallest synthetic sweep source, the one tests/test_gpu_index_cli.py uses.
PREFIX.settings, PREFIX.assignments and PREFIX.hkl must be byte for byte what `ffs_hosttool indexassign` -- csrc/assign_model.hpp on the CPU --
writes for PREFIX.centres, the printed geometry and the same vectors or settings file, and the printed lines the same; the refusals exit
non-zero and name the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import assign_oracle as AO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SPOTFINDER, HOSTTOOL = os.path.join(BIN, "spotfinder"), os.path.join(BIN, "ffs_hosttool")
N = 8
SWEEP = [f"synth:tinysweep:{N}", "--max-cell", "150", "--fft-npoints", "32", "--threads", "1", "--batch", "3", "--single-buffer", "--max-valid", "none"]


def run(argv, cwd):
    r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, timeout=300)
    return r.returncode, re.sub(r"\x1b\[[0-9;]*m", "", r.stdout), r.stderr


def setting_lines(out):
    lines = out.splitlines()
    at = lines.index("Candidate settings:")
    end = next(i for i in range(at, len(lines)) if lines[i].startswith("Indexed "))
    return lines[at:end + 1]


def files(tmp_path, prefix):
    return [(tmp_path / f"{prefix}.{ext}").read_bytes() for ext in ("settings", "assignments", "hkl")]


def test_driver_writes_what_the_host_tool_writes(tmp_path):
    # settings of the caller's own: cells of 40 to 90 A in a few orientations, one of them singular, one a doubled cell of another
    rng = np.random.default_rng(9)
    rows = [np.linalg.inv(np.diag(rng.uniform(40, 90, 3)) @ np.linalg.qr(rng.normal(size=(3, 3)))[0]).reshape(9) for _ in range(6)]
    rows += [np.zeros(9), rows[0] * 0.5]
    np.array(rows, "<f8").tofile(tmp_path / "own.settings")
    rc, out, err = run([SPOTFINDER, *SWEEP, "--index-basis", "run", "--index-assign", "a", "--index-settings", "own.settings", "--index-tolerance", "0.25"], tmp_path)
    assert rc == 0 and not err, (out[-3000:], err)
    geometry_words = re.search(r"Index geometry: (.*)", out).group(1).split()
    n = len(np.fromfile(tmp_path / "run.centres", "<f8")) // 3
    rc, tool_out, err = run([HOSTTOOL, "indexassign", "centres=run.centres", *geometry_words, "settings=own.settings", "tolerance=0.25", "out=tool"], tmp_path)
    assert rc == 0, (tool_out, err)
    got, want = files(tmp_path, "a"), files(tmp_path, "tool")
    assert got == want and len(got[0]) == 8 * 160 and len(got[1]) == 8 * 472 and len(got[2]) == 12 * n
    assert setting_lines(out) == setting_lines(tool_out) and len(setting_lines(out)) == 1 + 8 + 2
    recs = np.frombuffer(got[1], AO.ASSIGNMENT_DT)
    assert recs[6]["status"] == 1 and recs[6]["n_indexed"] == 0
    best = int(re.search(r"Best setting: (\d+)", out).group(1))
    assert recs[best]["n_indexed"] == recs["n_indexed"].max() and f"Indexed {recs[best]['n_indexed']}/{n} reflections" in out
    hkl = np.frombuffer(got[2], "<i4").reshape(n, 3)
    assert np.count_nonzero(np.any(hkl != 0, axis=1)) == recs[best]["n_indexed"]
    # ... and the settings from the run's own basis vectors, as many as they give
    rc, out, err = run([SPOTFINDER, *SWEEP, "--index-basis", "run2", "--index-assign", "b"], tmp_path)
    assert rc == 0 and not err, (out[-3000:], err)
    rc, tool_out, err = run([HOSTTOOL, "indexassign", "centres=run2.centres", *geometry_words, "vectors=run2.basis_vectors", "out=tool2"], tmp_path)
    assert rc == 0, (tool_out, err)
    assert files(tmp_path, "b") == files(tmp_path, "tool2") and setting_lines(out) == setting_lines(tool_out)
    vectors = np.fromfile(tmp_path / "run2.basis_vectors", AO.F).reshape(-1, 5)[:, :3]
    assert (tmp_path / "b.settings").read_bytes() == AO.settings(vectors).tobytes()


@pytest.mark.parametrize("argv,needle", [
    (["--index-assign", "a"], "--index-assign needs --index-basis"),
    (["--index-basis", "run", "--max-cell", "100", "--index-tolerance", "0.3"], "belong to --index-assign"),
    (["--index-basis", "run", "--max-cell", "100", "--index-assign", "a", "--index-tolerance", "0.6"], "--index-tolerance takes a number in (0, 0.5]"),
    (["--index-basis", "run", "--max-cell", "100", "--index-assign", "a", "--gpus", "2"], "--index-basis takes one GPU"),
    (["--index-basis", "run", "--max-cell", "100", "--index-assign", "a", "--validate"], "not available with --validate"),
], ids=["without-index-basis", "tolerance-alone", "tolerance-0.6", "two-gpus", "with-validate"])
def test_the_refusals_name_the_flag(tmp_path, argv, needle):
    rc, out, err = run([SPOTFINDER, "synth:tinysweep:4", *argv], tmp_path)
    assert rc != 0 and needle in out, (out[-1500:], err)
    assert not (tmp_path / "a.settings").exists() and not (tmp_path / "a.assignments").exists()
