"""CPU: csrc/assign_model.hpp as a stand-alone program (tests/assign_check.cc), plain and under the address and undefined-behaviour sanitizers,
against tests/assign_oracle.py byte for byte on every case of tests/assign_cases.py: the absence table, the selection, per setting the
record, hkl and lsq, the detected test, the reindexed setting and the settings from the basis vectors.  And the oracle itself against the
expected values of the reference's own unit tests (tests/golden/index_assign_reference_cases.json) and against what the lattices are."""
import json
import os
import subprocess

import numpy as np
import pytest

import assign_cases as AC
import assign_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "index_assign_reference_cases.json")))
DMIN, OSC_START, THRESHOLD = 1.5, 0.0, 0.9


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("assign_check")
    base = ["g++", "-std=c++20", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "assign_check.cc")]
    plain, san = str(d / "assign_check"), str(d / "assign_check_san")
    subprocess.run(base + ["-O2", "-o", plain], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], check=True)
    return plain, san


def write_input(path, c, vectors):
    sel = c["selected"]
    with open(path, "wb") as f:
        f.write(np.array([len(c["rlp"]), len(c["A"]), 0 if sel is None else 1, len(vectors)], "<u4").tobytes())
        f.write(np.array([c["tolerance"], DMIN, OSC_START, THRESHOLD], "<f8").tobytes())
        f.write(c["rlp"].tobytes() + c["phi"].tobytes() + (b"" if sel is None else sel.astype(np.uint8).tobytes()) + c["A"].tobytes())
        f.write(np.ascontiguousarray(vectors, "<f8").tobytes())


def expected_bytes(c, vectors):
    recs, hkl, lsq = AC.expected(c)
    out = [AO.table().tobytes(), AO.select(c["rlp"], c["phi"], DMIN, OSC_START).tobytes()]
    for k in range(len(c["A"])):
        out += [recs[k].tobytes(), hkl[k].tobytes(), lsq[k].tobytes()]
    detected = np.array([AO.detect(r, THRESHOLD) for r in recs], "<i4")
    re = np.zeros((len(c["A"]), 9))
    for k, t in enumerate(detected):
        if t >= 0:
            new = AO.reindex(c["A"][k], t)
            re[k] = new if new is not None else 0.0
    s = AO.settings(vectors)
    return b"".join(out + [detected.tobytes(), re.tobytes(), np.array([len(s)], "<u4").tobytes(), s.tobytes()])


@pytest.mark.parametrize("name", [c["name"] for c in AC.check_cases()])
def test_the_header_equals_the_oracle_plain_and_sanitized(programs, tmp_path, name):
    c = next(x for x in AC.check_cases() if x["name"] == name)
    vectors = c["vectors"]["v"] if "vectors" in c else np.zeros((0, 3))
    want = expected_bytes(c, vectors)
    write_input(str(tmp_path / "in"), c, vectors)
    for exe in programs:
        run = subprocess.run([exe, str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (exe, run.returncode, run.stderr[-2000:])
        got = open(str(tmp_path / "out"), "rb").read()
        assert len(got) == len(want) and got == want, (name, exe, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None))


def test_the_absence_table_is_the_issue_s():
    t = AO.table()
    assert len(t) == 111 and [tuple(x) for x in t["v"][::3][:4]] == [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)]
    assert [tuple(x) for x in t["v"][::3][-3:]] == [(2, -1, -1), (1, 1, -2), (1, -2, 1)] and list(t["modularity"][:6]) == [2, 3, 5, 2, 3, 5]
    for e in t:   # each transform maps the sublattice h . v = 0 mod m onto all integers: its determinant is the modularity
        assert round(np.linalg.det(e["transform"].reshape(3, 3).astype(float))) == e["modularity"]
        assert all(int(np.dot(row, e["v"])) % e["modularity"] == 0 for row in e["transform"].reshape(3, 3))


def test_the_reference_s_assign_indices_values():
    g = GOLDEN["assign_indices"]
    rec, hkl, lsq = AO.assign(g["rlp"], g["phi"], g["A"], g["tolerance"])
    assert rec["n_indexed"] == g["number_indexed"] == rec["n_accepted"] and hkl[:5].tolist() == g["miller_indices"] and hkl[5].tolist() == [0, 0, 0]
    assert lsq[5] > g["tolerance"] ** 2 and np.all(lsq[:5] <= g["tolerance"] ** 2)
    # the same spots with every phi equal: of each pair on one index only the closer stays
    rec2, hkl2, _ = AO.assign(g["rlp"], np.zeros(6), g["A"], g["tolerance"])
    assert rec2["n_accepted"] == 5 and rec2["n_indexed"] == 3 and sorted(map(tuple, hkl2[np.any(hkl2 != 0, 1)].tolist())) == [(22, -4, 4), (22, -4, 5), (22, -2, -1)]


def cell_of(axes):
    a = np.asarray(axes).reshape(3, 3)
    n = np.linalg.norm(a, axis=1)
    ang = [np.degrees(np.arccos(np.dot(a[i], a[j]) / (n[i] * n[j]))) for i, j in ((1, 2), (0, 2), (0, 1))]
    return sorted(n), sorted(ang)


def test_the_reference_s_combinations_values():
    g = GOLDEN["combinations"]
    s = AO.settings(g["vectors"], g["max_combinations"])
    assert len(s) == len(g["cells"]) == 2
    for got, want in zip(s, g["cells"]):
        edges, angles = cell_of(got["axes"])
        # (the reference's Niggli-reduced cell has all angles >= 90 or all <= 90: an angle and its supplement describe the same unreduced cell)
        assert np.allclose(edges, sorted(want[:3]), atol=g["tolerance"]), (edges, want)
        folded = sorted(max(x, 180.0 - x) for x in angles)
        assert np.allclose(folded, sorted(max(x, 180.0 - x) for x in want[3:]), atol=g["tolerance"]), (angles, want)
        assert np.allclose(got["A"].reshape(3, 3) @ got["axes"].reshape(3, 3), np.eye(3), atol=1e-12)


@pytest.mark.parametrize("name,n_settings,indexed,total", (("small-disturbed", None, 675, 709), ("triclinic-disturbed", 200, 3914, 4093)))
def test_the_true_setting_explains_the_lattice(name, n_settings, indexed, total):
    c = AC.lattice(name, n_settings)
    recs, hkl, _ = AC.expected(c)
    k = c["n_own"]
    assert len(c["rlp"]) == total and recs[k]["n_indexed"] == indexed and indexed >= 0.9 * total
    # against NumPy's own inverse and rounding, which share no text with the oracle: the same indices wherever both accept
    hf = c["rlp"] @ np.linalg.inv(c["A"][k].reshape(3, 3)).T
    plain = np.rint(hf).astype(np.int32)
    ok = np.any(hkl[k] != 0, axis=1)
    assert np.array_equal(hkl[k][ok], plain[ok]) and ok.sum() == indexed
    assert recs[k]["n_accepted"] - recs[k]["n_indexed"] in (4, 5, 6, 7, 8, 9, 10, 11, 12)   # a few duplicate groups, each of 2 or 3
    # the cell doubled: (almost) every index even, so the first test (h even) is detected; halved: few spots are accepted
    even = recs[k + 1]["absent0"][0] / recs[k + 1]["n_indexed"]
    assert even > 0.99 and AO.detect(recs[k + 1]) == 0 and AO.detect(recs[k]) == -1
    assert recs[k + 2]["n_accepted"] < 0.2 * total


def test_correct_brings_the_doubled_cell_back_in_three_rounds():
    c = AC.lattice("small-disturbed")
    k = c["n_own"]
    A, rec, hkl, rounds = AO.correct(c["rlp"], c["phi"], c["A"][k + 1])
    volume = abs(np.linalg.det(c["axes"]))
    assert rounds == 3 and abs(1.0 / abs(np.linalg.det(A.reshape(3, 3))) - volume) <= 1e-9 * volume
    assert rec["n_indexed"] == AC.expected(c)[0][k]["n_indexed"]


def test_the_tolerance_edge_is_built_on_the_ulp():
    for c in AC.corners():
        if "targets" in c:
            recs, _, lsq = AC.expected(c)
            assert lsq[0].tolist() == [float(t) for t in c["targets"] for _ in range(2)] and recs[0]["n_accepted"] == 4
