"""CPU: tests/radial_oracle.py, the truth of the per-frame radial profile, against a plain loop over the pixels in Python integers."""
import numpy as np
import pytest

import radial_oracle as R


def _case(dtype, W, H, seed):
    rng = np.random.default_rng(seed)
    img = rng.poisson(4.0, (H, W)).astype(np.uint64)
    hot = rng.random((H, W)) < 0.1
    img[hot] = rng.integers(500, 65536, int(hot.sum()))
    if np.dtype(dtype) == np.dtype(np.uint32):
        edge = rng.random((H, W)) < 0.1
        img[edge] = rng.choice(np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 7], np.uint64), int(edge.sum()))
    bins = rng.integers(0, 9, (H, W)).astype(np.uint16)
    bins[rng.random((H, W)) < 0.15] = R.NO_BIN
    mask = (rng.random((H, W)) < 0.8).astype(np.uint8)
    return img.astype(dtype), bins, mask


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("shape", [(40, 31), (37, 29), (8, 1), (2, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("max_valid", [-1, 0, 1000, 65535, (1 << 24) + 100])
def test_oracle_equals_the_pixel_loop(dtype, shape, max_valid):
    W, H = shape
    img, bins, mask = _case(dtype, W, H, seed=W + 100 * H)
    if np.dtype(dtype) == np.dtype(np.uint32) and W * H > 100:
        for v in ((1 << 24) - 1, 1 << 24, (1 << 24) + 7):
            assert (img == v).any()
    for m in (None, mask):
        got = R.radial_profile(img, bins, 9, m, max_valid)
        want = R.radial_profile_loop(img, bins, 9, m, max_valid)
        assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64 and got[2].dtype == np.uint64
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        assert int(got[0].sum()) == int(R.included(img, bins, m, max_valid).sum())


def test_the_rule_piece_by_piece():
    img = np.array([[5, 7, 2000, 9]], np.uint16)
    bins = np.array([[0, R.NO_BIN, 1, 1]], np.uint16)
    assert [a.tolist() for a in R.radial_profile(img, bins, 3)] == [[1, 2, 0], [5, 2009, 0], [25, 2000 * 2000 + 81, 0]]
    assert [a.tolist() for a in R.radial_profile(img, bins, 3, max_valid=1999)] == [[1, 1, 0], [5, 9, 0], [25, 81, 0]]
    assert [a.tolist() for a in R.radial_profile(img, bins, 3, max_valid=2000)][0] == [1, 2, 0]      # p <= max_valid counts
    assert [a.tolist() for a in R.radial_profile(img, bins, 3, mask=np.array([[0, 1, 1, 0]], np.uint8))] == [[0, 1, 0], [0, 2000, 0], [0, 4000000, 0]]
    img32 = np.array([[(1 << 24) - 1, 1 << 24, (1 << 24) + 7]], np.uint32)
    c, s, q = R.radial_profile(img32, np.zeros((1, 3), np.uint16), 1)
    assert c.tolist() == [1] and int(s[0]) == (1 << 24) - 1 and int(q[0]) == ((1 << 24) - 1) ** 2      # the oracle's p < 2^24 rule


def test_sum_sq_wraps_modulo_2_64_and_sums_keep_every_bit():
    # 90 000 pixels at 2^24 - 1: float64 weights would lose the low bits of both sums
    img = np.full((300, 300), (1 << 24) - 1, np.uint32)
    c, s, q = R.radial_profile(img, np.zeros((300, 300), np.uint16), 1)
    exact = 90000 * ((1 << 24) - 1) ** 2
    assert exact >= 1 << 64 and int(q[0]) == exact % (1 << 64) and int(s[0]) == 90000 * ((1 << 24) - 1) and int(c[0]) == 90000
    # 2^25 - ... a 16-bit frame cannot wrap: its largest sum_sq for 300 x 300 pixels is exact
    c, s, q = R.radial_profile(np.full((300, 300), 65535, np.uint16), np.zeros((300, 300), np.uint16), 1)
    assert int(q[0]) == 90000 * 65535 ** 2 and int(s[0]) == 90000 * 65535
    odd = np.array([[(1 << 24) - 1, 3, (1 << 24) - 2]], np.uint32)
    c, s, q = R.radial_profile(odd, np.zeros((1, 3), np.uint16), 1)
    assert int(q[0]) == ((1 << 24) - 1) ** 2 + 9 + ((1 << 24) - 2) ** 2      # odd: a float64 sum near 2^49 would still hold it, uint64 certainly does


def test_shell_bins_are_shells():
    b = R.shell_bins(37, 29, 6)
    assert b.dtype == np.uint16 and b.shape == (29, 37) and sorted(np.unique(b)) == list(range(6))
    assert b[14, 18] == 0 and b[0, 0] == 5
