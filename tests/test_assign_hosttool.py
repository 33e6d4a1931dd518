"""CPU: `ffs_hosttool indexassign`, the CPU twin of `spotfinder --index-assign` compiled from csrc/assign_model.hpp and host/index_assign.hpp,
against tests/assign_oracle.py: the settings from a lattice's own basis vectors, the records after correction for a non-primitive basis, the
best setting's indices and the lines it prints; a settings file with a doubled cell and a singular row; and what it refuses."""
import os
import subprocess

import numpy as np
import pytest

import assign_cases as AC
import assign_oracle as AO
import index_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTTOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
GEOMETRY = ["distance=150.0", "beam_x=1231.4", "beam_y=1263.7", "pixel_x=0.172", "pixel_y=0.172", "wavelength=1.0", "osc_start=0.0", "osc_width=0.25"]


@pytest.fixture(scope="module", autouse=True)
def tool():
    if not os.path.exists(HOSTTOOL):
        subprocess.run(["make", "-C", ROOT, "synth", "cli"], check=True, stdout=subprocess.DEVNULL)


def run_tool(tmp, xyz, extra):
    centres = os.path.join(tmp, "c.centres")
    np.ascontiguousarray(xyz, "<f8").tofile(centres)
    return subprocess.run([HOSTTOOL, "indexassign", "centres=" + centres, *GEOMETRY, "out=" + os.path.join(tmp, "out"), *extra], capture_output=True, text=True)


def corrected(c, A, tolerance=0.3):
    """the oracle's records after correction, the best setting and its hkl"""
    recs, As = [], []
    for a in A:
        ok = AO.inverse(a)[1]
        a2, rec, hkl, rounds = AO.correct(c["rlp"], c["phi"], a, tolerance) if ok else (a, AO.assign(c["rlp"], c["phi"], a, tolerance)[0], None, 0)
        recs.append(rec), As.append(a2)
    recs = np.array(recs, AO.ASSIGNMENT_DT)
    volume = [1.0 / abs(np.linalg.det(a.reshape(3, 3))) if AO.inverse(a)[1] else 0.0 for a in As]
    best = min(range(len(A)), key=lambda k: (-int(recs[k]["n_indexed"]), volume[k], k))
    return recs, best, AO.assign(c["rlp"], c["phi"], As[best], tolerance)[1]


def test_the_settings_of_a_lattice_s_own_vectors(tmp_path):
    c = AC.lattice("small-disturbed")
    vectors = os.path.join(str(tmp_path), "v.basis_vectors")
    c["vectors"][:9].tofile(vectors)   # (the first nine vectors: 84 triples)
    run = run_tool(str(tmp_path), K.by_name("small-disturbed")["xyz"], ["vectors=" + vectors])
    assert run.returncode == 0, (run.stdout[-800:], run.stderr[-800:])
    s = AO.settings(c["vectors"]["v"][:9])
    assert len(s) > 10 and open(os.path.join(str(tmp_path), "out.settings"), "rb").read() == s.tobytes()
    recs, best, hkl = corrected(c, s["A"])
    assert open(os.path.join(str(tmp_path), "out.assignments"), "rb").read() == recs.tobytes()
    assert open(os.path.join(str(tmp_path), "out.hkl"), "rb").read() == hkl.tobytes()
    lines = run.stdout.splitlines()
    assert lines[0] == "Candidate settings:" and len(lines) == len(s) + 3 and lines[-2] == f"Best setting: {best}"
    n = len(c["rlp"])
    assert lines[-1] == f"Indexed {recs[best]['n_indexed']}/{n} reflections ({100.0 * recs[best]['n_indexed'] / n:.2f}% indexed)"
    for k, line in enumerate(lines[1:-2]):
        assert line.startswith(f"{k} cell ") and f" indexed {recs[k]['n_indexed']} (" in line, line


def test_a_settings_file_with_a_doubled_cell_and_a_singular_row(tmp_path):
    c = AC.lattice("small-disturbed")
    true_A = c["A"][c["n_own"]]
    rows = np.stack([true_A * 0.5, np.zeros(9), true_A, true_A * 2.0])
    path = os.path.join(str(tmp_path), "rows.settings")
    rows.astype("<f8").tofile(path)
    run = run_tool(str(tmp_path), K.by_name("small-disturbed")["xyz"], ["settings=" + path, "tolerance=0.3"])
    assert run.returncode == 0, (run.stdout[-800:], run.stderr[-800:])
    recs, best, hkl = corrected(c, rows)
    got = np.fromfile(os.path.join(str(tmp_path), "out.assignments"), AO.ASSIGNMENT_DT)
    assert got.tobytes() == recs.tobytes() and got[0]["n_indexed"] == got[2]["n_indexed"] == 675 and got[1]["status"] == 1
    assert open(os.path.join(str(tmp_path), "out.hkl"), "rb").read() == hkl.tobytes()
    lines = run.stdout.splitlines()
    # the doubled cell comes back to the true volume in three reindexings; the tie on 675 goes to the smaller volume, then to the lower number
    assert "reindexed 3x" in lines[1] and "reindexed" not in lines[3] and lines[1].split(" volume ")[1].split()[0] == lines[3].split(" volume ")[1].split()[0]
    assert lines[-2] == f"Best setting: {best}" and best in (0, 2)
    settings = np.fromfile(os.path.join(str(tmp_path), "out.settings"), AO.SETTING_DT)
    assert settings["A"].tobytes() == rows.tobytes() and not settings["axes"].any() and not settings["triple"].any()


def test_what_the_tool_refuses(tmp_path):
    xyz = K.by_name("one-spot")["xyz"]
    rows = os.path.join(str(tmp_path), "rows.settings")
    np.eye(3).reshape(1, 9).astype("<f8").tofile(rows)
    for extra, needle in ((["settings=" + rows, "tolerance=0.6"], "tolerance must be in (0, 0.5]"), (["settings=" + rows, "tolerance=0"], "tolerance"),
                          (["settings=" + rows, "wavelength=-1"], "wavelength"), ([], "missing vectors= or settings=")):
        run = run_tool(str(tmp_path), xyz, extra)
        assert run.returncode == 1 and "FAIL: indexassign: " in run.stdout and needle in run.stdout, (extra, run.stdout)
    bad = os.path.join(str(tmp_path), "bad.settings")
    open(bad, "wb").write(b"\0" * 71)
    run = run_tool(str(tmp_path), xyz, ["settings=" + bad])
    assert run.returncode == 1 and "whole number of rows of nine float64" in run.stdout
    nan = os.path.join(str(tmp_path), "nan.settings")
    np.full((1, 9), np.nan).astype("<f8").tofile(nan)
    run = run_tool(str(tmp_path), xyz, ["settings=" + nan])
    assert run.returncode == 1 and "A has an entry that is not finite" in run.stdout
