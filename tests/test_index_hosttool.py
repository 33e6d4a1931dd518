"""CPU: `ffs_hosttool indexbasis`, the CPU twin of ffs_ctx_index_grid / index_peaks compiled from csrc/index_model.hpp, against
tests/index_oracle.py: the peaks, the candidate vectors, the digest of the power grid and the lines it prints, at n_points 16 .. 64 on the
cases of tests/index_cases.py and once at 256 (the one slow case: some 4 s of the tool and 8 s of the oracle); and what it refuses."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import index_cases as K
import index_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTTOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
GEOMETRY = ["distance=150.0", "beam_x=1231.4", "beam_y=1263.7", "pixel_x=0.172", "pixel_y=0.172", "wavelength=1.0", "osc_start=0.0", "osc_width=0.25"]


@pytest.fixture(scope="module", autouse=True)
def tool():
    if not os.path.exists(HOSTTOOL):
        subprocess.run(["make", "-C", ROOT, "synth", "cli"], check=True, stdout=subprocess.DEVNULL)
    assert np.array_equal(K.geometry()["d_matrix"], K.geometry(0.172, 150.0, (1231.4, 1263.7))["d_matrix"]), "GEOMETRY is the cases' geometry"


def run_tool(tmp, c, n_points, extra=()):
    centres, prefix = os.path.join(tmp, "c.centres"), os.path.join(tmp, f"out{n_points}")
    c["xyz"].astype("<f8").tofile(centres)
    args = [HOSTTOOL, "indexbasis", "centres=" + centres, *GEOMETRY, f"max-cell={c['max_cell']!r}", f"npoints={n_points}", "out=" + prefix, *extra]
    if c["dmin"] is not None:
        args.append(f"dmin={c['dmin']!r}")
    return subprocess.run(args, capture_output=True, text=True), prefix


def assert_tool_equals_oracle(tmp, c, n_points):
    run, prefix = run_tool(tmp, c, n_points)
    assert run.returncode == 0, (run.stdout[-800:], run.stderr[-800:])
    o = O.chain(c["g"], c["xyz"], c["max_cell"], n_points, c["dmin"])
    what = (c["name"], n_points)
    assert open(prefix + ".grid_sha256").read() == hashlib.sha256(o["power"].tobytes()).hexdigest() + "\n", what
    assert open(prefix + ".peaks", "rb").read() == o["peaks"].tobytes(), what
    assert open(prefix + ".basis_vectors", "rb").read() == o["vectors"].tobytes(), what
    lines = run.stdout.splitlines()
    at = lines.index("Candidate basis vectors:")
    assert lines[at + 1:] == [f"{i} {v['length']:.5f} {v['volume']}" for i, v in enumerate(o["vectors"])], what
    assert f"{len(c['xyz'])} spots" in lines[0] and f"{len(o['peaks'])} peaks" in lines[0], lines[0]
    return o


@pytest.mark.parametrize("n_points", (16, 32, 64))
def test_the_tool_equals_the_oracle(tmp_path, n_points):
    for c in K.cases():
        assert_tool_equals_oracle(str(tmp_path), c, n_points)


def test_the_tool_equals_the_oracle_at_256(tmp_path):
    c = K.by_name("triclinic-disturbed")
    o = assert_tool_equals_oracle(str(tmp_path), c, 256)
    assert len(o["peaks"]) > 100 and len(o["vectors"]) >= 3


def test_what_the_tool_refuses(tmp_path):
    c = K.by_name("one-spot")
    for extra, needle in ((["npoints=48"], "n_points must be a power of two in 16 .. 256"), (["npoints=512"], "n_points"), (["max-cell=0"], "max_cell"), (["dmin=-1"], "dmin"),
                          (["wavelength=-1"], "wavelength"), (["pixel_x=-0.1"], "pixel sizes")):
        run, _ = run_tool(str(tmp_path), c, 32, extra)   # (a key given twice: the last one holds)
        assert run.returncode == 1 and "FAIL: indexbasis: " in run.stdout and needle in run.stdout, (extra, run.stdout)
    bad = os.path.join(str(tmp_path), "bad.centres")
    open(bad, "wb").write(b"\0" * 25)
    run = subprocess.run([HOSTTOOL, "indexbasis", "centres=" + bad, *GEOMETRY, "max-cell=45", "out=" + bad], capture_output=True, text=True)
    assert run.returncode == 1 and "whole number of rows" in run.stdout
    run = subprocess.run([HOSTTOOL, "indexbasis", *GEOMETRY, "max-cell=45", "out=" + bad], capture_output=True, text=True)
    assert run.returncode == 1 and "missing centres=" in run.stdout
