"""GPU: ffs_ctx_predict on the cases of predict_cases.scan_cases(), bit for bit against tests/predict_oracle.py fed the library's own
scan-point settings.  The candidate boxes have 1023, 1024, 1025, 1435 and 2065 workgroups of 256: k_predict_scan, one workgroup of 1024
threads, takes one, two and three counts a thread, cuts the last thread's range at n_blocks and leaves the threads behind it empty -- every
record's position in the output follows from its offsets.  cap next to the offset of a workgroup that is the second of its scan thread's,
cap inside one candidate's run of two records, two calls.  tests/test_predict_scan.py asserts without a GPU that the cases are what they
are named for.

The first workgroups of every candidate box hold the layer h = -h_max, which lies outside the resolution sphere (h_max = floor(|a| / dmin)
+ 1): the workgroups scan thread 1 owns have the offset 0, and a cap one below it does not exist; cap = 1, one above it, is checked."""
import numpy as np
import pytest

import predict_cases as K
import predict_oracle as O
from test_gpu_predict import args, assert_same

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in K.scan_cases()}
_oracle = {}


def expected(ffs, c):
    if c["name"] not in _oracle:
        census = {}
        settings = ffs.predict_scan_settings(c["g"], c["A"], c["n_images"])
        rec = O.predict(c["g"], c["A"], c["n_images"], c["dmin"], c["delta_b"], c["delta_m"], K.W, K.H, c["centring"], settings, census)
        census["facts"] = K.assert_scan_census(c, census)
        _oracle[c["name"]] = (rec, census)
    return _oracle[c["name"]]


@pytest.fixture(scope="module")
def ctx(ffs):
    return ffs.Context(K.W, K.H, np.uint16, max_batch=1)


@pytest.mark.parametrize("name", list(CASES))
def test_the_records_equal_the_oracles_bit_for_bit(ffs, ctx, name):
    c = CASES[name]
    want, _ = expected(ffs, c)
    assert_same(ctx.predict(*args(c)), want, name)


def capped(ffs, ctx, c, want, cap):
    with pytest.raises(ffs.FfsError) as e:
        ctx.predict(*args(c), cap=cap)
    assert e.value.code == -4 and e.value.n == len(want), (c["name"], cap)
    assert e.value.records.tobytes() == want[:cap].tobytes(), (c["name"], cap)


@pytest.mark.parametrize("name", ["scan-1025", "scan-2065"])
def test_a_cap_next_to_a_workgroups_offset_and_inside_a_lanes_run(ffs, ctx, name):
    c = CASES[name]
    want, census = expected(ffs, c)
    per = census["facts"]["per"]
    block = census["q"] // 256
    offset = lambda b: int(np.sum(block < b))
    # the workgroups scan thread 1 owns: per .. 2 per - 1
    assert all(offset(b) == 0 for b in range(per, 2 * per))
    capped(ffs, ctx, c, want, 1)
    # the second predicting workgroup of a scan thread: its offset is the thread's running sum, one count in
    blocks = np.unique(block)
    second = [int(b) for b in blocks[1:] if b % per != 0 and (b - 1) in blocks and (b - 1) // per == b // per]
    assert second and offset(second[0]) > 1 and second[0] // per >= 1
    for b in (second[0], second[-1]):
        capped(ffs, ctx, c, want, offset(b) - 1)
        capped(ffs, ctx, c, want, offset(b) + 1)
    # a candidate with two records: cap between them
    q, first, count = np.unique(census["q"], return_index=True, return_counts=True)
    twice = np.flatnonzero(count >= 2)
    assert len(twice) > 0
    capped(ffs, ctx, c, want, int(first[twice[len(twice) // 2]]) + 1)


def test_two_calls_give_identical_bytes(ffs, ctx):
    c = CASES["scan-2065"]
    a = ctx.predict(*args(c))
    b = ctx.predict(*args(c))
    assert a.tobytes() == b.tobytes() and len(a) == len(expected(ffs, c)[0])
