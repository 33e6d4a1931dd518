"""The robust Poisson GLM background of a spot's ring (ffs_stream_spot_backgrounds_glm, include/ffs_hip.h) in Python float64, in the
reference's per-pixel form: psi of every pixel's residual, the Poisson pdf through lgamma, the cdf as the finite sum of pdfs, math.exp and
math.log.  It deliberately uses neither the four integers nor the recurrence of csrc/spot_background_glm_model.hpp, so that it is an
independent partner of that header; it follows the header's order of status checks, its all-zero rule and its bound on mu.  The checker,
never the thing tested.  Ring extraction and the histogram are tests/spot_background_oracle.py's."""
import math

import numpy as np

from spot_background_oracle import N_BINS, histogram, ring_values  # noqa: F401  (ring_values: for the callers)

OK, NO_PIXELS, OVERFLOW, FEW_PIXELS, DEGENERATE, NOT_CONVERGED = 0, 1, 2, 5, 6, 7
C = 1.345
TOLERANCE = 1e-3
MAX_ITER = 100
MIN_PIXELS = 10
MAX_MU = 512.0
DT = np.dtype([("n_pixels", "<u4"), ("n_overflow", "<u4"), ("median", "<i4"), ("n_iter", "<u4"), ("status", "<u4"), ("reserved", "<u4"),
               ("beta", "<f8"), ("mean", "<f8")])
INTEGER_FIELDS = ["n_pixels", "n_overflow", "median", "n_iter", "status"]

_LGAMMA = np.array([math.lgamma(k + 1.0) for k in range(700)])


def _pdf(mu, k):
    if k < 0:
        return 0.0
    return math.exp(k * math.log(mu) - mu - math.lgamma(k + 1.0))


def _cdf(mu, k):
    if k < 0:
        return 0.0
    ks = np.arange(k + 1, dtype=np.float64)
    return float(np.exp(ks * math.log(mu) - mu - _LGAMMA[:k + 1]).sum())


def _expectation(mu, s):
    j1, j2 = math.floor(mu - C * s), math.floor(mu + C * s)
    p1, p2, p3, p4, p5 = _pdf(mu, j1), _pdf(mu, j2), _cdf(mu, j1), _pdf(mu, j2 + 1), _cdf(mu, j2 + 1)
    p6 = 1.0 - p5 + p4
    p7, p8, p9 = _pdf(mu, j1 - 1), _pdf(mu, j2 - 1), _cdf(mu, j2 - 1)
    p10 = p9 - p3 + p1
    epsi1 = C * (p6 - p3) + (mu / s) * (p1 - p2)
    epsi2 = C * (p1 + p2) + (mu * mu / (s * s * s)) * (p10 / mu + p7 - p1 - p8 + p2)
    return epsi1, epsi2, j1, j2


def from_values(values):
    """dict(n_pixels, n_overflow, median, n_iter, status, beta, mean) of a ring's valid pixel values, and what the census asks about the
    run: errors (every step's), j1_min, j2_max, seed_from_zero."""
    v = np.asarray(values, np.uint64)
    N = len(v)
    over = int((v >= N_BINS).sum())
    r = dict(n_pixels=N, n_overflow=over, median=-1, n_iter=0, status=OK, beta=0.0, mean=0.0, errors=[], j1_min=None, j2_max=None, seed_from_zero=False)
    if N == 0:
        r["status"] = NO_PIXELS
        return r
    if N < MIN_PIXELS:
        r["status"] = FEW_PIXELS
        return r
    if 4 * over > N:
        r["status"] = OVERFLOW
        return r
    r["median"] = median = int(np.sort(v)[N // 2])
    assert median < N_BINS
    if over == 0 and not v.any():
        r["beta"] = -math.inf
        return r
    r["seed_from_zero"] = median == 0
    beta = math.log(float(median) if median > 0 else 1.0)
    y = v.astype(np.float64)
    clipped = v >= N_BINS            # a pixel of the tail enters at psi = +c, whatever its value
    for it in range(MAX_ITER):
        r["beta"], r["n_iter"] = beta, it
        if not -700.0 < beta < 700.0:
            r["status"] = DEGENERATE
            return r
        mu = math.exp(beta)
        s = math.sqrt(mu)
        if not mu > 0.0 or not s > 0.0 or not mu < MAX_MU:
            r["status"] = DEGENERATE
            return r
        epsi1, epsi2, j1, j2 = _expectation(mu, s)
        r["j1_min"] = j1 if r["j1_min"] is None else min(r["j1_min"], j1)
        r["j2_max"] = j2 if r["j2_max"] is None else max(r["j2_max"], j2)
        b = epsi2 * mu * mu / s
        res = (y - mu) / s
        psi = np.where(np.abs(res) < C, res, np.where(res > 0.0, C, -C))
        psi[clipped] = C
        U = float(((psi - epsi1) * mu / s).sum())
        delta = U / (N * b) if b != 0.0 else math.inf
        if not math.isfinite(b) or not math.isfinite(delta):
            r["status"] = DEGENERATE
            return r
        error = math.sqrt(delta * delta / max(beta * beta, 1e-10))
        beta += delta
        r["beta"], r["n_iter"] = beta, it + 1
        r["errors"].append(error)
        if error < TOLERANCE:
            break
    else:
        r["status"] = NOT_CONVERGED
        return r
    if not -300.0 < beta < 300.0:
        r["status"] = DEGENERATE
        return r
    r["mean"] = math.exp(beta)
    return r


def near_the_tolerance(result, within=0.01):
    """Some step's error lies within 1 % of the tolerance: whether another step follows is a matter of the last bit."""
    return any(abs(e - TOLERANCE) < within * TOLERANCE for e in result["errors"])


def record(values):
    """The seven fields of ffs_spot_background_glm as a tuple, the doubles as floats."""
    r = from_values(values)
    return tuple(r[k] for k in INTEGER_FIELDS) + (r["beta"], r["mean"])
