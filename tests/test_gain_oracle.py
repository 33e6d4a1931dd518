"""CPU: tests/gain_oracle.py -- the NumPy restatement of the reference's gain arithmetic that the GPU tests of ffs_ctx_set_gain are
held to -- tied to the committed oracle: equal to it at gain 1.0 (debug planes included), exactly invariant under scaling frame and
gain by a power of two, equal to a pixel loop, and different from the no-gain oracle on frames in ADU."""
import numpy as np
import pytest

import gain_oracle as G
import tie_windows as T
import window_ties as WT
from oracle import oracle as O

WINDOWS = [(3, 3), (2, 5), (7, 1)]


def _disp(kx, ky, min_count=2):
    return O.DispParams(kx, ky, min_count, 0.0, 6.0, 3.0)


def _seeded(dtype, seed, masked):
    photons, mask = G.photon_frame(seed, masked=masked)
    img = photons.astype(dtype)
    if dtype == np.uint32:   # neighbours and centres at and above 2^24 (standalone.cc:78,90)
        rng = np.random.default_rng(seed + 50)
        big = rng.random(img.shape) < 0.02
        img[big] = rng.choice([(1 << 24) - 1, 1 << 24, (1 << 24) + 7], size=big.sum())
    return img, mask


@pytest.mark.parametrize("kx,ky", WINDOWS, ids=["3x3", "2x5", "7x1"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
def test_gain_1_equals_the_oracle(kx, ky, dtype, masked):
    for seed in (1, 2, 3):
        img, mask = _seeded(dtype, seed, masked)
        want = O.dispersion(img, mask, _disp(kx, ky))
        assert want.sum() > 100
        assert np.array_equal(G.dispersion_gain(img, mask, 1.0, kx, ky), want)


@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5), (5, 5)], ids=["3x3", "2x5", "5x5"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_gain_1_on_tie_frames(kx, ky, dtype):
    prm = T.Params(min_count=(2 * kx + 1) * (2 * ky + 1) // 2)
    img, mask, cells = WT.frame(kx, ky, dtype, prm)
    got = G.dispersion_gain(img, mask, 1.0, kx, ky, min_count=prm.min_count)
    assert np.array_equal(got, O.dispersion(img, mask, _disp(kx, ky, prm.min_count)))
    assert len(cells) > 50
    for c in cells:   # every tie cell as exact arithmetic decides it
        assert bool(got[c.row, c.col]) == c.exact, (c.family, c.side, c.m, c.x, c.y, c.p)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_extended_gain_1_equals_the_oracle(dtype):
    for seed, masked in ((5, True), (6, False)):
        img, mask = G.blob_photons(seed, masked=masked)
        img = img.astype(dtype)
        for max_valid in (-1, 3000):
            want = O.dispersion_extended(img, mask, None, 0, float(max_valid), debug=True)
            got = G.dispersion_extended_gain(img, mask, 1.0, max_valid=max_valid)
            assert want[0].sum() > 0 and want[2].sum() > 100
            for g, w, name in zip(got, want, ("strong", "first pass", "eroded")):
                assert np.array_equal(g, w), name


@pytest.mark.parametrize("scale", [2, 4])
def test_scaling_by_a_power_of_two_is_exact(scale):
    """Frame x 2^k with gain 2^k: a and c both scale by 4^k, b and d by 2^k, the local test by 2^k -- every operation exactly."""
    for seed in (1, 2, 3):
        for kx, ky in WINDOWS:
            photons, mask = G.photon_frame(seed)
            img = photons.astype(np.uint16)
            assert np.array_equal(G.dispersion_gain(img * scale, mask, float(scale), kx, ky), G.dispersion_gain(img, mask, 1.0, kx, ky))
    img, mask = G.blob_photons(5)
    for g, w in zip(G.dispersion_extended_gain(img * scale, mask, float(scale)), G.dispersion_extended_gain(img, mask, 1.0)):
        assert np.array_equal(g, w)


# ---- a pixel loop, in the style of _numpy_dispersion of tests/test_window_params.py
def _loop_dispersion_gain(img, mask, gain, kx, ky, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0):
    H, W = img.shape
    v = img.astype(np.int64)
    ok = (mask != 0) & (v < (1 << 24))
    pv = np.where(ok, v, 0)
    out = np.zeros((H, W), np.uint8)
    g = np.float64(gain)
    for yy in range(H):
        for xx in range(W):
            y0, y1 = max(yy - ky, 0), min(yy + ky, H - 1)
            x0, x1 = max(xx - kx, 0), min(xx + kx, W - 1)
            m = int(ok[y0:y1 + 1, x0:x1 + 1].sum())
            x = int(pv[y0:y1 + 1, x0:x1 + 1].sum())
            y = int((pv[y0:y1 + 1, x0:x1 + 1] ** 2).sum())
            src = np.float64(v[yy, xx])
            if not (mask[yy, xx] and m >= min_count and x >= 0 and src > threshold):
                continue
            md, xd, yd = np.float64(m), np.float64(x), np.float64(y)
            a = md * yd - xd * xd
            b = md * src - xd
            c = (g * xd) * ((md - 1.0) + np.float64(nsig_b) * np.sqrt(2.0 * (md - 1.0)))
            d = np.float64(nsig_s) * np.sqrt((g * xd) * md)
            out[yy, xx] = 1 if (a > c and b > d) else 0
    return out


@pytest.mark.parametrize("W,H", [(2, 2), (40, 5), (3, 33)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_vectorised_form_against_a_pixel_loop(W, H, dtype):
    rng = np.random.default_rng(W * 7 + H)
    img = rng.poisson(3.0, size=(H, W))
    hot = rng.random((H, W)) < 0.06
    img[hot] = rng.integers(20, 900, size=hot.sum())
    if dtype == np.uint32:
        img[rng.random((H, W)) < 0.04] = 1 << 24
    img = img.astype(dtype)
    mask = (rng.random((H, W)) > 0.12).astype(np.uint8)
    total = 0
    for gain in (1.0, 2.5, 0.3):
        for kx, ky in WINDOWS:
            got = G.dispersion_gain(img, mask, gain, kx, ky)
            assert np.array_equal(got, _loop_dispersion_gain(img, mask, gain, kx, ky))
            total += int(got.sum())
    assert total > 0 or W * H < 10


# ---- the gain matters: a frame in ADU through the photon-count predicate is full of false strong pixels
@pytest.mark.parametrize("gain", [7.0, 2.5])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_adu_frames_give_the_photon_frames_strong_set(gain, seed):
    photons, mask = G.photon_frame(seed)
    want = O.dispersion(photons.astype(np.uint16), mask)
    img = G.adu(photons, gain, np.uint16)
    assert 300 < want.sum() < 700
    assert np.array_equal(G.dispersion_gain(img, mask, gain), want)
    assert O.dispersion(img, mask).sum() > 2 * want.sum()
