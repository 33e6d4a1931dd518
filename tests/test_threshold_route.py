"""CPU: which threshold stage and which form of the predicate a batch takes (csrc/threshold_route.hpp) is decided once, in a header
without HIP.  tests/threshold_route_check.cc prints the route for the full product of its inputs, in its own process under the address
and undefined-behaviour sanitizers.  Checked here: every row equals the rules as DESIGN.md section 3.3e states them, restated below
without anything of the header; the instantiation rule of every kernel family; and that no row is missing."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-feedback-service_amd", "csrc")
FLAGS = ["-std=c++20", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

DISPERSION, EXTENDED = 0, 1                                        # include/ffs_hip.h: FFS_ALGO_*
CENTRE, WINDOW_SCOPE = 0, 1                                        # ... FFS_MAX_VALID_*
PHOTON, SCOPE, GAIN = 0, 1, 2                                      # enum Predicate
CROSS_CHECK, WINDOW, STREAM_LIST, STREAM_EXACT, EXT_STAGE = range(5)   # enum ThresholdStage
EXACT, EXT_FINAL, EXT_FUSED, K_WINDOW, EXT_FIRST = range(5)        # enum KernelFamily

INPUTS = dict(algorithm=(DISPERSION, EXTENDED), pixel_bytes=(2, 4), window_3x3=(1, 0), scope=(CENTRE, WINDOW_SCOPE), max_valid=(-1, 1000),
              gain=(0.0, 2.5), path=(0, 1, 2), rerun=(-1, 1), window_kernel=(0, 1), ext_first_pass=(0, 2), ext_fused=(0, 1))


def expected(algorithm, pixel_bytes, window_3x3, scope, max_valid, gain, path, rerun, window_kernel, ext_first_pass, ext_fused):
    """(stage, variant, window scope on, bright_to_plane, ext_variant, first pass streams, fused, extended, has a dense kernel)"""
    scope_on = scope == WINDOW_SCOPE and max_valid >= 0
    variant = GAIN if gain > 0 else SCOPE if scope_on else PHOTON
    to_plane = rerun if rerun >= 0 else path
    ext_variant = ext_first_pass if (pixel_bytes == 2 and rerun < 0 and variant == PHOTON) else 0
    fused = False
    if algorithm == EXTENDED:
        stage = EXT_STAGE
        fused = pixel_bytes == 2 and ext_fused != 0 and variant != GAIN
    elif to_plane == 2:
        stage = CROSS_CHECK
    elif not window_3x3 or window_kernel == 1 or variant != PHOTON:
        stage = WINDOW
    else:
        stage = STREAM_LIST if to_plane == 0 else STREAM_EXACT
    dense_kernel = not (stage == CROSS_CHECK and not window_3x3)
    return (stage, variant, int(scope_on), to_plane, ext_variant, int(ext_variant >= 2), int(fused), int(algorithm == EXTENDED), int(dense_kernel))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("route") / "threshold_route_check"
    subprocess.run(["g++", *FLAGS, "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "threshold_route_check.cc"), "-o", str(exe)],
                   check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def rows(run):
    out = {}
    for line in run.stdout.splitlines():
        if line.startswith("R "):
            key, val = line[2:].split("|")
            k = key.split()
            out[tuple(float(v) if i == 5 else int(v) for i, v in enumerate(k))] = tuple(int(v) for v in val.split())
    return out


def test_the_run_is_clean(run):
    assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])


def test_every_row_follows_the_rules(run, rows):
    cases = list(itertools.product(*INPUTS.values()))   # ten inputs of two values and one of three
    assert len(cases) == 3072 and len(rows) == 3072 and sum(line.startswith("R ") for line in run.stdout.splitlines()) == 3072
    for case in cases:
        assert rows[case] == expected(*case), dict(zip(INPUTS, case))


def test_what_the_launches_rely_on(rows):
    for case, (stage, variant, scope_on, to_plane, ext_variant, streams, fused, ext, dense) in rows.items():
        c = dict(zip(INPUTS, case))
        assert not (variant == GAIN and fused), c                  # no gain batch is fused
        assert not (variant != PHOTON and streams), c              # a gain or window-scope batch never streams its first pass
        assert not (variant != PHOTON and stage in (STREAM_LIST, STREAM_EXACT)), c   # ... nor takes a streaming kernel of the dispersion algorithm
        assert not (fused and c["pixel_bytes"] == 4) and not (streams and c["pixel_bytes"] == 4), c   # both exist for 16-bit pixels only
        assert (stage == EXT_STAGE) == bool(ext) == (c["algorithm"] == EXTENDED), c
        if stage in (STREAM_LIST, STREAM_EXACT):
            assert c["window_3x3"] and to_plane == (0 if stage == STREAM_LIST else 1), c


def test_the_instantiation_rule(run):
    got = {}
    for line in run.stdout.splitlines():
        if line.startswith("I "):
            key, val = line[2:].split("|")
            got[tuple(int(v) for v in key.split())] = tuple(int(v) for v in val.split())
    assert len(got) == 5 * 2 * 3
    for family, pixel_bytes, variant in itertools.product(range(5), (2, 4), (PHOTON, SCOPE, GAIN)):
        # k_window and k_ext_first read the neighbour limit of 32-bit pixels as an argument in every instantiation: the window scope is
        # their photon-count instantiation, and none of theirs counts as carrying the compare
        limit_is_argument = pixel_bytes == 4 and family in (K_WINDOW, EXT_FIRST)
        as_variant = PHOTON if (limit_is_argument and variant == SCOPE) else variant
        assert got[(family, pixel_bytes, variant)] == (as_variant, int(as_variant != PHOTON and not limit_is_argument), int(as_variant == GAIN))
    for family in (K_WINDOW, EXT_FIRST):
        assert got[(family, 4, SCOPE)][0] == PHOTON and got[(family, 2, SCOPE)][0] == SCOPE
