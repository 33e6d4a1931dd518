"""CPU: the tables of tests/shoebox_seams.py.  (a) The builders' own conditions, asserted on the oracle alone: foreground edges on the strip
seams, on the last corner column and the first and last corner row, the largest boxes and the boxes in the pad, exact ties that decide a
pixel, lists shorter than a workgroup.  (b) csrc/shoebox_model.hpp as a plain C++ program (tests/shoebox_check.cc, built as
tests/test_shoebox_oracle.py builds it) equals the oracle on every job: records, histograms and foreground maps, bit for bit; the address
and undefined-behaviour sanitizers run the same program over the seam, tie and size jobs.  (c) The ties bite: the same program built with
-ffp-contract=fast and the host's FMA differs from the oracle on some of them."""
import subprocess

import numpy as np
import pytest

import shoebox_oracle as O
import shoebox_seams as S
import test_shoebox_oracle as T   # (CSRC, CHECK, SANITIZE and run_header: the program is built and fed as that file does it)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("shoebox_seams")
    flags = ["-std=c++20", "-Wall", "-Werror", "-I", T.CSRC, T.CHECK]
    subprocess.run(["g++", "-O2", "-ffp-contract=off", *flags, "-o", str(d / "plain")], check=True)
    subprocess.run(["g++", "-O1", "-ffp-contract=off", *T.SANITIZE, *flags, "-o", str(d / "sanitized")], check=True)
    return d


# ---- (a) the builders' conditions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,algorithm", S.SEAM_COMBOS, ids=[S.combo_id(d, a) for d, a in S.SEAM_COMBOS])
def test_the_seam_tables_contain_what_they_are_built_for(dtype, algorithm):
    j = S.seam_job(dtype, algorithm)   # (asserts the conditions of every group)
    assert set(j["groups"]) == {"seam-first", "seam-second", "seam-left-overhang", "seam-right-edge", "width-63", "width-64", "width-126", "width-127", "edge-rows", "one-pixel"}
    assert [S.SEAMS[n][0] + S.STRIP * S.SEAMS[n][1] for n in ("first", "second", "left-overhang", "right-edge")] == [68, 86, 3, S.W - 1]
    acc = S.acc_of(j)
    assert sum(acc["fg_count"]) > 1000 and acc["hist"].sum() > 10000
    assert j["frames"].shape == (4, S.H, S.W) and j["frames"].dtype == dtype


@pytest.mark.parametrize("dtype,algorithm", S.LARGEST_COMBOS, ids=[S.combo_id(d, a) for d, a in S.LARGEST_COMBOS])
def test_the_largest_boxes_and_the_boxes_in_the_pad(dtype, algorithm):
    j = S.largest_job(dtype, algorithm)
    b = j["boxes"]
    assert (int(b["x_max"][3]), int(b["x_min"][4]), int(b["y_max"][5]), int(b["y_min"][6])) == (-1023, S.W + 1023, -1023, S.H + 1023)
    assert (int(b["x_min"][7]), int(b["x_max"][7])) == (-1023, -1023 + 1024) and (int(b["x_min"][8]), int(b["x_max"][8])) == (S.W - 1, S.W + 1023)
    sq = S.square_job(*S.SQUARE_COMBO)["boxes"][0]
    assert int(sq["x_max"] - sq["x_min"]) == int(sq["y_max"] - sq["y_min"]) == 1024 and (int(sq["z_min"]), int(sq["z_max"])) == (0, 2)
    (wide, _), (high, _) = S.refused_boxes(j["g"])
    assert int(wide["x_max"] - wide["x_min"]) == 1025 and int(high["y_max"] - high["y_min"]) == 1025


@pytest.mark.parametrize("algorithm", [O.DIALS, O.ELLIPSOID], ids=["dials", "ellipsoid"])
def test_the_ties_are_exact_and_decide_a_pixel(algorithm):
    j = S.tie_job(algorithm)   # (asserts value == 1.0 on the tie, below and above it either side, and a pixel that differs)
    assert len(j["ties"]) >= 12
    print(j["name"], [(t["kind"], t["which"], t["corner"]) for t in j["ties"]])


def test_the_short_lists():
    jobs = S.short_jobs()
    assert [len(j["boxes"]) for j in jobs] == [1, 2, 3, 5, 5]
    assert [S.list_lengths(j["boxes"]) for j in jobs] == [[1] * 3, [2] * 3, [3] * 3, [5] * 3, [1, 4, 5]]
    assert {np.dtype(j["dtype"]).itemsize for j in jobs} == {2, 4} and {j["algorithm"] for j in jobs} == {O.ELLIPSOID, O.DIALS}


# ---- (b) the header as a C++ program -----------------------------------------------------------------------------------------------------
def differences(program, j, work, background=0):
    """What of the program's output differs from the oracle on a job: a list of names, empty when nothing does."""
    got, maps = T.run_header(program, j, background, work)
    acc = S.acc_of(j)
    out = []
    for k, name in enumerate(("fg_sum", "m_x", "m_y", "m_z")):
        if not np.array_equal(got["acc"][:, k], np.array(acc[name], np.uint64)):
            out.append(name)
    for k, name in enumerate(("fg_count", "n_overflow", "flags")):
        if not np.array_equal(got["acc32"][:, k], np.array(acc[name], np.uint32)):
            out.append(name)
    if not np.array_equal(got["hist"], acc["hist"].astype(np.uint32)):
        out.append("hist")
    try:
        O.assert_records_equal(got["sum"], O.sums(acc, "glm" if background else "tukey"), j["name"])
    except AssertionError as e:
        out.append(f"records {e}")
    want = []
    for b in j["boxes"]:
        images = range(max(int(b["z_min"]), 0), min(int(b["z_max"]), j["n_images"]))
        m = O.foreground_maps(j["g"], b, j["algorithm"], j["delta_b"], j["delta_m"], images)
        want += [m[n].astype(np.uint8).ravel() for n in images]
    if not np.array_equal(maps, np.concatenate(want)):
        out.append("foreground maps")
    return out


def job_ids(jobs):
    return [j["name"] for j in jobs]


@pytest.mark.parametrize("j", S.all_jobs(), ids=job_ids(S.all_jobs()))
@pytest.mark.parametrize("background", [0, 1], ids=["tukey", "glm"])
def test_header_program_agrees_bit_for_bit(programs, tmp_path, j, background):
    assert differences(programs / "plain", j, tmp_path, background) == []


SANITIZED_JOBS = S.seam_and_tie_jobs() + [S.largest_job(*S.LARGEST_COMBOS[0]), S.square_job(*S.SQUARE_COMBO)]


@pytest.mark.parametrize("j", SANITIZED_JOBS, ids=job_ids(SANITIZED_JOBS))
def test_sanitized_header_program_agrees_and_reports_nothing(programs, tmp_path, j):
    assert differences(programs / "sanitized", j, tmp_path) == []   # (run_header asserts an empty stderr)


# ---- (c) the ties bite -------------------------------------------------------------------------------------------------------------------
def host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma" in line for line in f)
    except OSError:
        return False


@pytest.mark.skipif(not host_has_fma(), reason="the CPU has no fused multiply-add")
def test_a_contracted_build_gets_ties_wrong(programs, tmp_path):
    """The same program with -ffp-contract=fast -mfma: some tie box's foreground differs from the oracle's.  The random tables of
    tests/test_shoebox_oracle.py do not notice such a build; these do."""
    exe = programs / "contracted"
    subprocess.run(["g++", "-O2", "-ffp-contract=fast", "-mfma", "-std=c++20", "-Wall", "-Werror", "-I", T.CSRC, T.CHECK, "-o", str(exe)], check=True)
    wrong = total = 0
    for algorithm in (O.DIALS, O.ELLIPSOID):
        j = S.tie_job(algorithm)
        got, _ = T.run_header(exe, j, 0, tmp_path)
        acc = S.acc_of(j)
        same = (got["acc32"][:, 0] == np.array(acc["fg_count"], np.uint32)) & (got["acc"][:, 0] == np.array(acc["fg_sum"], np.uint64)) & np.all(got["hist"] == acc["hist"], axis=1)
        for t in j["ties"]:
            total += 1
            wrong += int(not same[t["first"]:t["first"] + 3].all())
    print(f"the contracted build differs from the oracle on {wrong} of {total} ties")
    assert wrong >= 1
