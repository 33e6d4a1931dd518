"""Rings for the robust Poisson GLM background: a seeded list of (name, pixel values), the planted ones first, then random rings --
Poisson(0.02 .. 240), 5 .. 404 pixels, 0 .. 29 % of them thrown far up.  A random ring in which the Python oracle sees some step's error
within 1 % of the tolerance is dropped at generation: whether one more step follows there is a matter of the last bit of an `exp`.  At most
2 % of the random rings may go that way, and none of the planted ones.  tests/golden/spot_background_glm_ref.json holds what the
reference's glm_constant_background returns for every case of this list, in this order."""
import functools

import numpy as np

import spot_background_glm_oracle as G

N_RANDOM = 1500
SEED = 20161912


def planted():
    rng = np.random.default_rng(SEED + 1)
    P = {}
    P["nine_pixels"] = rng.poisson(4.0, 9)
    P["ten_pixels"] = rng.poisson(4.0, 10)
    P["no_pixels"] = np.zeros(0, np.int64)
    v = rng.poisson(6.0, 40)
    v[:10] = 4000
    P["overflow_quarter"] = v.copy()                      # 4 * overflow = N: still fitted
    P["overflow_quarter_plus_one"] = v[:-1].copy()        # 4 * 10 = N + 1: refused
    P["all_zero"] = np.zeros(72, np.int64)
    v = np.zeros(72, np.int64)
    v[5] = 9000
    P["all_zero_one_overflow"] = v
    v = np.zeros(120, np.int64)
    v[:40] = rng.poisson(3.0, 40) + 1
    P["median_zero_pixels_above"] = v
    P["poisson_0_05"] = rng.poisson(0.05, 400)
    P["poisson_200"] = rng.poisson(200.0, 300)
    P["poisson_235"] = rng.poisson(235.0, 300)
    P["one_bin"] = np.full(64, 7, np.int64)
    P["one_bin_255"] = np.full(64, 255, np.int64)
    P["poisson_3_of_100000"] = rng.poisson(3.0, 100_000)
    P["poisson_3_clean"] = rng.poisson(3.0, 400)
    P["poisson_40_clean"] = rng.poisson(40.0, 400)
    P["far_seed"] = np.concatenate([np.full(49, 250, np.int64), np.zeros(51, np.int64)])    # median 0, mean 122: many steps
    assert (P["poisson_0_05"] > 0).any() and (P["poisson_235"] > 255).any()
    return {k: np.asarray(v, np.uint64) for k, v in P.items()}


def random_ring(rng):
    n = int(rng.integers(5, 405))
    v = rng.poisson(float(np.exp(rng.uniform(np.log(0.02), np.log(240.0)))), n).astype(np.uint64)
    thrown = rng.random(n) < rng.uniform(0.0, 0.29)
    v[thrown] += rng.integers(300, 60000, n).astype(np.uint64)[thrown]
    return v


@functools.lru_cache(maxsize=1)
def cases():
    """[(name, values as uint64)], the same list on every call; the oracle's result for each is in results()."""
    out, res = [], []
    for name, v in planted().items():
        r = G.from_values(v)
        assert not G.near_the_tolerance(r), name
        out.append((name, v))
        res.append(r)
    rng = np.random.default_rng(SEED)
    dropped = 0
    for i in range(N_RANDOM):
        v = random_ring(rng)
        r = G.from_values(v)
        if G.near_the_tolerance(r):
            dropped += 1
            continue
        out.append(("random_%04d" % i, v))
        res.append(r)
    assert dropped <= 0.02 * N_RANDOM, dropped
    cases.results = res
    return out


def results():
    cases()
    return cases.results


def histogram_text(rings):
    """The rings as the input of the check program and of `ffs_hosttool spotbgglm`: 257 integers a line."""
    lines = []
    for v in rings:
        bins, tail = G.histogram(v)
        lines.append(" ".join(str(int(c)) for c in bins) + " %d\n" % tail)
    return "".join(lines)


W, H = 37, 29


def planted_frames():
    """name -> dict(frame, mask (None: all valid), border, box (x_min, x_max, y_min, y_max), status, and for some n_pixels, n_iter, mean): frames
    built so that the spot finder returns the box and the ring around it brings one planted situation onto the device.  The CPU test holds
    the committed oracle to them, the GPU test the library."""
    rng = np.random.default_rng(SEED + 2)
    out = {}
    box = (17, 19, 13, 15)
    f = np.zeros((H, W), np.uint16)
    f[13:16, 17:20] = 1000
    out["all_zero_ring"] = dict(frame=f, mask=None, border=3, box=box, status=G.OK, n_pixels=72, n_iter=0, mean=0.0)
    for n_ring in (9, 10):              # 8 x 8, a 2 x 2 block, border 1: a ring of 12 pixels, 3 or 2 of them masked
        f = np.full((8, 8), 2, np.uint16)
        f[3:5, 3:5] = 800
        m = np.ones((8, 8), np.uint8)
        for x, y in [(2, 2), (5, 5), (2, 5)][:12 - n_ring]:
            m[y, x] = 0
        out["ring_of_%d" % n_ring] = dict(frame=f, mask=m, border=1, box=(3, 4, 3, 4), status=G.FEW_PIXELS if n_ring < 10 else G.OK, n_pixels=n_ring)
    f = rng.poisson(200.0, (H, W)).astype(np.uint16)
    f[13:16, 17:20] = 20000
    out["poisson_200"] = dict(frame=f, mask=None, border=3, box=box, status=G.OK, n_pixels=72)
    f = rng.poisson(0.05, (H, W)).astype(np.uint16)
    f[13:16, 17:20] = 1000
    out["poisson_0_05"] = dict(frame=f, mask=None, border=3, box=box, status=G.OK, n_pixels=72)
    f = np.zeros((H, W), np.uint16)     # two levels far apart, the median on the lower one: the step swings for some sixty steps before it settles
    f[:, 19:] = 250
    f[10, 18] = f[18, 18] = 250        # (the ring of border 3: 37 pixels at 0 and 35 at 250)
    f[13:16, 17:20] = 9000
    out["two_levels"] = dict(frame=f, mask=None, border=3, box=box, status=G.OK, n_pixels=72, n_iter_at_least=50)
    return out
