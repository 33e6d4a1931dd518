"""CPU: the rows a streaming wave trims off its band's two ends (csrc/launch_geometry.hpp: empty_runs_of, trim_band) are plain integer
arithmetic in the header the kernels compile.  tests/band_trim_check.cc walks it by brute force -- every frame height up to 48 rows,
every band height, a few thousand flag vectors -- in its own process under the address and undefined-behaviour sanitizers, and prints
what the Eiger-16M mask loses under the bench geometry.  Checked here: the program's properties hold on every case (it checks them and
says so), and the Eiger numbers are the ones DESIGN.md section 3.2f reasons from."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
FLAGS = ["-std=c++20", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# trimmed rows by band: 56 bands of 78 rows, module gaps at rows 512 + 550 k .. 549 + 550 k, k = 0 .. 6
EIGER = {6: 34, 7: 4, 13: 30, 14: 8, 20: 26, 21: 12, 27: 22, 28: 16, 34: 18, 35: 20, 41: 14, 42: 24, 48: 10, 49: 28}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("band_trim") / "band_trim_check"
    subprocess.run(["g++", *FLAGS, "-I", CSRC, os.path.join(ROOT, "tests", "band_trim_check.cc"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_properties_hold_and_sanitizers_are_clean(run):
    failures = [line for line in run.stdout.splitlines() if line.startswith("FAIL")]
    assert not failures, failures[:10]
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])


def test_the_eiger_mask_under_the_bench_geometry(run):
    (line,) = [l for l in run.stdout.splitlines() if l.startswith("E ")]
    got = {int(b): int(n) for b, n in (part.split(":") for part in line.split()[1:])}
    assert got == EIGER
    assert sum(got.values()) == 266
    assert "Eiger: 266 rows trimmed of 266 empty rows, 4698 wave rows a strip" in run.stdout
    assert round(100 * 266 / 4698, 2) == 5.66


def test_the_gaps_are_those_of_the_synthetic_eiger_mask():
    """The rows the program takes for the module gaps are the rows ffs_amd.synth.mask_eiger16m leaves without a valid pixel."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))
    from ffs_amd import synth
    mask = synth.mask_eiger16m()
    empty = [y for y in range(mask.shape[0]) if not mask[y].any()]
    assert mask.shape[0] == 4362 and empty == [y for k in range(7) for y in range(512 + 550 * k, 550 + 550 * k)]
