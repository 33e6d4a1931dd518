"""CPU: the threshold route with its trailing input "a gain map is set" (csrc/threshold_route.hpp).
tests/threshold_route_map_check.cc prints the route over the product of inputs of tests/threshold_route_check.cc x {no map, map}, in its own
process under the address and undefined-behaviour sanitizers.  Checked here: every row equals the rules restated below without
anything of the header; with no map every row is what threshold_route_check prints (the parameter is defaulted: that program
compiles and runs unchanged); the instantiation rule of variant 3."""
import itertools
import os
import subprocess

import pytest

import test_threshold_route as R

GAIN_MAP = 3                                                       # enum Predicate
INPUTS = dict(R.INPUTS, gain_map=(0, 1))


def expected(algorithm, pixel_bytes, window_3x3, scope, max_valid, gain, path, rerun, window_kernel, ext_first_pass, ext_fused, gain_map):
    """A map batch takes the route a gain batch takes, under its own variant (which wins over a scalar gain: the ABI refuses the pair)."""
    if not gain_map:
        return R.expected(algorithm, pixel_bytes, window_3x3, scope, max_valid, gain, path, rerun, window_kernel, ext_first_pass, ext_fused)
    as_gain = R.expected(algorithm, pixel_bytes, window_3x3, scope, max_valid, 2.5, path, rerun, window_kernel, ext_first_pass, ext_fused)
    assert as_gain[1] == R.GAIN
    return as_gain[:1] + (GAIN_MAP,) + as_gain[2:]


def _build_and_run(tmp, name):
    exe = tmp / name
    subprocess.run(["g++", *R.FLAGS, "-I", R.CSRC, "-I", os.path.join(R.ROOT, "include"), os.path.join(R.ROOT, "tests", name + ".cc"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("route_map")
    return _build_and_run(tmp, "threshold_route_map_check"), _build_and_run(tmp, "threshold_route_check")


def _rows(run):
    out = {}
    for line in run.stdout.splitlines():
        if line.startswith("R "):
            key, val = line[2:].split("|")
            out[tuple(float(v) if i == 5 else int(v) for i, v in enumerate(key.split()))] = tuple(int(v) for v in val.split())
    return out


def test_the_runs_are_clean(runs):
    for run in runs:
        assert run.returncode == 0 and run.stderr == "" and run.stdout.splitlines()[-1] == "OK", (run.returncode, run.stderr[-2000:])


def test_every_row_follows_the_rules(runs):
    rows = _rows(runs[0])
    cases = list(itertools.product(*INPUTS.values()))
    assert len(cases) == 6144 and len(rows) == 6144
    for case in cases:
        assert rows[case] == expected(*case), dict(zip(INPUTS, case))


def test_without_a_map_every_line_is_what_threshold_route_check_prints(runs):
    with_map_input, plain = _rows(runs[0]), _rows(runs[1])
    assert len(plain) == 3072
    assert {k[:-1]: v for k, v in with_map_input.items() if k[-1] == 0} == plain
    # ... and its instantiation lines are the ones of variants 0..2
    assert sum(line.startswith("I ") for line in runs[1].stdout.splitlines()) == 5 * 2 * 3


def test_what_the_launches_rely_on(runs):
    for case, (stage, variant, scope_on, to_plane, ext_variant, streams, fused, ext, dense) in _rows(runs[0]).items():
        c = dict(zip(INPUTS, case))
        assert (variant == GAIN_MAP) == bool(c["gain_map"]), c
        if variant == GAIN_MAP:
            assert not fused and not streams and ext_variant == 0, c                 # erosion + final pass; the plain first pass
            assert stage in (R.CROSS_CHECK, R.WINDOW, R.EXT_STAGE), c                # never a streaming kernel
            if c["algorithm"] == R.DISPERSION:
                assert stage == (R.CROSS_CHECK if to_plane == 2 else R.WINDOW), c    # k_window at every window; threshold_path 2: the gather
            assert scope_on == int(c["scope"] == R.WINDOW_SCOPE and c["max_valid"] >= 0), c   # nb_limit follows the scope as in a gain batch


def test_the_instantiation_rule_of_variant_3(runs):
    got = {}
    for line in runs[0].stdout.splitlines():
        if line.startswith("I "):
            key, val = line[2:].split("|")
            got[tuple(int(v) for v in key.split())] = tuple(int(v) for v in val.split())
    assert len(got) == 5 * 2
    for family, pixel_bytes in itertools.product(range(5), (2, 4)):
        limit_is_argument = pixel_bytes == 4 and family in (R.K_WINDOW, R.EXT_FIRST)
        # instantiated as itself (nothing folds into it); carries the neighbour limit exactly as kGain does; the gain form, from the map
        assert got[(family, pixel_bytes, GAIN_MAP)] == (GAIN_MAP, int(not limit_is_argument), 1, 1)
