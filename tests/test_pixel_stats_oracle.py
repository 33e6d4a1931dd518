"""CPU: tests/pixel_stats_oracle.py, the truth of the per-pixel statistics, against a plain loop over frames and pixels in Python integers."""
import numpy as np
import pytest

import pixel_stats_oracle as P


def _case(dtype, B, W, H, seed):
    rng = np.random.default_rng(seed)
    f = rng.poisson(4.0, (B, H, W)).astype(np.uint64)
    hot = rng.random((B, H, W)) < 0.1
    f[hot] = rng.integers(500, 65536, int(hot.sum()))
    if np.dtype(dtype) == np.dtype(np.uint32):
        edge = rng.random((B, H, W)) < 0.1
        f[edge] = rng.choice(np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 7, 0xFFFFFFFF], np.uint64), int(edge.sum()))
    return f.astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("shape", [(40, 31), (37, 29), (8, 1), (2, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("max_valid", [-1, 0, 1000, 65535, (1 << 24) + 100])
def test_oracle_equals_the_pixel_loop(dtype, shape, max_valid):
    W, H = shape
    frames = _case(dtype, 5, W, H, seed=W + 100 * H)
    if np.dtype(dtype) == np.dtype(np.uint32) and W * H > 100:
        for v in ((1 << 24) - 1, 1 << 24, (1 << 24) + 7):
            assert (frames == v).any()
    got = P.pixel_stats(frames, max_valid)
    P.assert_equal(got, P.pixel_stats_loop(frames, max_valid))
    assert got[0] == 5 and int(got[1].sum()) == int(P.counted(frames, max_valid).sum())
    assert not got[4][got[1] == 0].any()                       # max is 0 where count is 0
    # in pieces, and merged from two halves: the same state
    P.assert_equal(P.fold(P.fold(P.empty(H, W), frames[:2], max_valid), frames[2:], max_valid), got)
    P.assert_equal(P.merge(P.pixel_stats(frames[:3], max_valid), P.pixel_stats(frames[3:], max_valid)), got)


def test_the_rule_piece_by_piece():
    frames = np.array([[[5, 7, 2000, 9]], [[6, 0, 2001, 65535]]], np.uint16)
    n, c, s, q, m = P.pixel_stats(frames)
    assert n == 2 and c.tolist() == [[2, 2, 2, 2]] and s.tolist() == [[11, 7, 4001, 65544]] and m.tolist() == [[6, 7, 2001, 65535]]
    assert q.tolist() == [[61, 49, 2000 * 2000 + 2001 * 2001, 81 + 65535 * 65535]]
    n, c, s, q, m = P.pixel_stats(frames, max_valid=2000)      # p <= max_valid counts
    assert n == 2 and c.tolist() == [[2, 2, 1, 1]] and s.tolist() == [[11, 7, 2000, 9]] and m.tolist() == [[6, 7, 2000, 9]]
    n, c, s, q, m = P.pixel_stats(frames, max_valid=0)
    assert c.tolist() == [[0, 1, 0, 0]] and not s.any() and not q.any() and not m.any()
    f32 = np.array([[[(1 << 24) - 1, 1 << 24, (1 << 24) + 7, 0xFFFFFFFF]]], np.uint32)
    n, c, s, q, m = P.pixel_stats(f32, max_valid=(1 << 24) + 100)          # the p < 2^24 rule, whatever max_valid says
    assert c.tolist() == [[1, 0, 0, 0]] and int(s[0, 0]) == (1 << 24) - 1 and int(q[0, 0]) == ((1 << 24) - 1) ** 2 and m.tolist() == [[(1 << 24) - 1, 0, 0, 0]]


def test_sum_sq_wraps_modulo_2_64_and_sums_keep_every_bit():
    top = (1 << 24) - 1
    state = P.empty(1, 2)
    frames = np.full((1000, 1, 2), top, np.uint32)
    for _ in range(66):                       # 66 000 frames near 2^24: beyond 2^64
        state = P.fold(state, frames)
    exact = 66000 * top * top
    assert exact >= 1 << 64 and int(state[3][0, 0]) == exact % (1 << 64) and int(state[2][0, 1]) == 66000 * top and int(state[1][0, 0]) == 66000
    n, c, s, q, m = P.pixel_stats(np.full((3, 1, 1), 65535, np.uint16))
    assert int(q[0, 0]) == 3 * 65535 ** 2 > 1 << 32 and int(s[0, 0]) == 3 * 65535
