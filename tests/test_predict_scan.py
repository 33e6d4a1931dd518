"""CPU: the cases of predict_cases.scan_cases() -- candidate boxes of 1023, 1024, 1025, 1435 and 2065 workgroups, where the one-workgroup
scan over the workgroups' counts takes one, two and three counts a thread, cuts its last thread's range and leaves threads empty.  The
builders' conditions on the oracle's census, and csrc/predict_model.hpp as a plain C++ program (tests/predict_check.cc, built as
tests/test_predict_oracle.py builds it; the sanitized build runs the smallest case) equal to the oracle bit for bit on every record."""
import subprocess

import numpy as np
import pytest

import predict_cases as K
import predict_oracle as O
import test_predict_oracle as T   # (CSRC, CHECK, SANITIZE, run_check and oracle: the program is built and fed as that file does it)

CASES = K.scan_cases()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("predict_scan")
    out = {"dir": str(d)}
    for name, extra in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g"] + T.SANITIZE)):
        out[name] = str(d / ("predict_check_" + name))
        subprocess.run(["g++", "-std=c++20", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", T.CSRC, T.CHECK, "-o", out[name]], check=True)
    return out


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_check_program_equals_the_oracle_and_the_case_is_what_it_is_named_for(exes, c):
    hm, n_cand, own, rec = T.run_check(exes["plain"], exes["dir"], c)
    census = {}
    want = T.oracle(c, own, census)
    assert hm == c["scan"]["h_max"] == O.h_max(c["A"], c["dmin"]) and n_cand == census["candidates"]
    print(c["name"], K.assert_scan_census(c, census))
    assert len(rec) == len(want) and rec.tobytes() == want.tobytes()
    assert np.max(np.unique(census["q"], return_counts=True)[1]) >= 2, "a candidate with two records: a lane's run a cap can cut"


def test_the_sanitized_build_gives_the_same_bytes_and_reports_nothing(exes):
    c = CASES[0]
    _, _, own, rec = T.run_check(exes["plain"], exes["dir"], c)
    _, _, own_s, rec_s = T.run_check(exes["sanitized"], exes["dir"], c, own)
    assert rec_s.tobytes() == rec.tobytes() and own_s.tobytes() == own.tobytes()
