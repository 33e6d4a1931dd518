"""CPU: tests/gain_map_oracle.py -- the NumPy restatement of the reference's gain arithmetic with a per-pixel gain ARRAY that the
GPU tests of ffs_ctx_set_gain_map are held to -- tied to tests/gain_oracle.py (and through it to the committed oracle): equal to
it on constant maps, equal to a pixel loop that reads the CENTRE's entry, and different from a scalar at the map's mean."""
import numpy as np
import pytest

import gain_map_oracle as M
import gain_oracle as G

WINDOWS = [(3, 3), (2, 5), (7, 1)]
CONSTANTS = [7.0, 2.5, float(np.float32(0.3))]


def _seeded(dtype, seed, masked, gain):
    photons, mask = G.photon_frame(seed, masked=masked)
    img = G.adu(photons, gain, dtype)
    if dtype == np.uint32:   # neighbours and centres at and above 2^24 (standalone.cc:78,90)
        rng = np.random.default_rng(seed + 50)
        big = rng.random(img.shape) < 0.02
        img[big] = rng.choice([(1 << 24) - 1, 1 << 24, (1 << 24) + 7], size=big.sum())
    return img, mask


@pytest.mark.parametrize("kx,ky", WINDOWS, ids=["3x3", "2x5", "7x1"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
def test_constant_map_equals_the_scalar(kx, ky, dtype, masked):
    for c in CONSTANTS:
        img, mask = _seeded(dtype, 1, masked, c)
        want = G.dispersion_gain(img, mask, c, kx, ky)
        assert want.sum() > 100
        assert np.array_equal(M.dispersion_gain_map(img, mask, np.full(img.shape, c, np.float32), kx, ky), want)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
def test_extended_constant_map_equals_the_scalar(dtype, masked):
    photons, mask = G.blob_photons(5, masked=masked)
    for c in CONSTANTS:
        img = G.adu(photons.astype(np.int64), c, dtype)
        for max_valid in (-1, int(3000 * c)):
            want = G.dispersion_extended_gain(img, mask, c, max_valid=max_valid)
            got = M.dispersion_extended_gain_map(img, mask, np.full(img.shape, c, np.float32), max_valid=max_valid)
            assert want[0].sum() > 0 and want[2].sum() > 100
            for g, w, name in zip(got, want, ("strong", "first pass", "eroded")):
                assert np.array_equal(g, w), name


def test_a_float64_constant_is_taken_as_its_float32():
    """The map is float32: 0.3 arrives as float32(0.3), and that is what the scalar must be given to agree."""
    img, mask = _seeded(np.uint16, 2, True, 0.3)
    got = M.dispersion_gain_map(img, mask, np.full(img.shape, 0.3))
    assert np.array_equal(got, G.dispersion_gain(img, mask, float(np.float32(0.3))))


# ---- a pixel loop: the gain is the CENTRE's entry, never a neighbour's
def _loop(img, mask, gmap, kx, ky, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0):
    H, W = img.shape
    v = img.astype(np.int64)
    ok = (mask != 0) & (v < (1 << 24))
    pv = np.where(ok, v, 0)
    out = np.zeros((H, W), np.uint8)
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
            g = np.float64(np.float32(gmap[yy, xx]))   # gain[k], k the centre
            md, xd, yd = np.float64(m), np.float64(x), np.float64(y)
            a = md * yd - xd * xd
            b = md * src - xd
            c = (g * xd) * ((md - 1.0) + np.float64(nsig_b) * np.sqrt(2.0 * (md - 1.0)))
            d = np.float64(nsig_s) * np.sqrt((g * xd) * md)
            out[yy, xx] = 1 if (a > c and b > d) else 0
    return out


def _loop_extended(img, mask, gmap, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0):
    H, W = img.shape
    v = img.astype(np.int64)
    ok = (mask != 0) & (v < (1 << 24))
    pv = np.where(ok, v, 0)
    first = np.zeros((H, W), np.uint8)
    for yy in range(H):
        for xx in range(W):
            win = (slice(max(yy - 3, 0), min(yy + 3, H - 1) + 1), slice(max(xx - 3, 0), min(xx + 3, W - 1) + 1))
            m, x, y = int(ok[win].sum()), int(pv[win].sum()), int((pv[win] ** 2).sum())
            if not (mask[yy, xx] and m >= min_count):
                continue
            g = np.float64(np.float32(gmap[yy, xx]))
            md, xd, yd = np.float64(m), np.float64(x), np.float64(y)
            a = md * yd - xd * xd
            c = (g * xd) * ((md - 1.0) + np.float64(nsig_b) * np.sqrt(2.0 * (md - 1.0)))
            first[yy, xx] = a > c
    eroded = G.erode(first, mask)
    bg = ok & (eroded == 0)
    strong = np.zeros((H, W), np.uint8)
    for yy, xx in zip(*np.nonzero(eroded)):
        win = (slice(max(yy - 5, 0), min(yy + 5, H - 1) + 1), slice(max(xx - 5, 0), min(xx + 5, W - 1) + 1))
        m2, x2 = int(bg[win].sum()), int(v[win][bg[win]].sum())
        mean = np.float64(x2) / np.float64(m2) if m2 >= 2 else np.float64(0.0)
        g = np.float64(np.float32(gmap[yy, xx]))
        src = np.float64(v[yy, xx])
        strong[yy, xx] = src > threshold and src >= mean + np.float64(nsig_s) * np.sqrt(g * mean)
    return strong, first, eroded


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_vectorised_form_against_a_pixel_loop(dtype):
    W, H = 40, 30
    rng = np.random.default_rng(W * 7 + H)
    gmap = M.random_map(3, W, H)
    photons = rng.poisson(3.0, size=(H, W)).astype(np.int64)
    hot = rng.random((H, W)) < 0.06
    photons[hot] = rng.integers(20, 900, size=hot.sum())
    img = M.adu_under_map(photons, gmap, dtype)
    if dtype == np.uint32:
        img[rng.random((H, W)) < 0.04] = 1 << 24
    mask = (rng.random((H, W)) > 0.12).astype(np.uint8)
    total = 0
    for kx, ky in WINDOWS:
        got = M.dispersion_gain_map(img, mask, gmap, kx, ky)
        assert np.array_equal(got, _loop(img, mask, gmap, kx, ky))
        # (a neighbour's entry in the centre's place decides differently on this frame: the loop does tell them apart)
        assert not np.array_equal(got, _loop(img, mask, np.roll(gmap, 1, axis=1), kx, ky))
        total += int(got.sum())
    assert total > 0


def test_extended_against_a_pixel_loop():
    W, H = 40, 30
    photons, mask = G.blob_photons(3, W, H, masked=False)
    mask = mask.copy()
    mask[:, 17] = 0
    gmap = M.random_map(4, W, H)
    img = M.adu_under_map(photons.astype(np.int64), gmap, np.uint16)
    got = M.dispersion_extended_gain_map(img, mask, gmap)
    want = _loop_extended(img, mask, gmap)
    assert want[2].sum() > 0 and want[0].sum() > 0
    for g, w, name in zip(got, want, ("strong", "first pass", "eroded")):
        assert np.array_equal(g, w), name


# ---- the map matters: a scalar at the map's mean is wrong on every module that differs from the mean
@pytest.mark.parametrize("kx,ky", WINDOWS, ids=["3x3", "2x5", "7x1"])
def test_module_map_differs_from_the_scalar_at_its_mean(kx, ky):
    photons, mask = G.photon_frame(1)
    gmap = M.module_map()
    assert gmap.shape == (97, 530) and gmap[0, 499] == np.float32(2.5) and gmap[0, 500] == np.float32(0.3) and gmap[48, 0] == 1.0
    img = M.adu_under_map(photons, gmap, np.uint16)
    want = M.dispersion_gain_map(img, mask, gmap, kx, ky)
    scalar = G.dispersion_gain(img, mask, float(gmap.mean(dtype=np.float64)), kx, ky)
    assert want.sum() > 0
    assert (want != scalar).sum() > 100 and scalar.sum() > want.sum()


def test_the_shared_maps_scale_to_other_shapes():
    for W, H in ((300, 200), (1, 1), (9, 5), (700, 130)):
        g = M.module_map(W, H)
        assert g.shape == (H, W) and g.dtype == np.float32 and set(np.unique(g)) <= {np.float32(v) for v in (7.0, 2.5, 0.3, 1.0)}
        r = M.random_map(2, W, H)
        assert r.shape == (H, W) and r.dtype == np.float32 and r.min() >= 0.5 and r.max() < 8.0
    assert len(np.unique(M.module_map(300, 200))) == 4
