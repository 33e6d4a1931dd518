"""GPU: the fp64 square root the exact predicate uses, over what windows up to 15 x 15 (m <= 225) feed it -- 16-bit frames give
n = x*m <= 225*225*65535 (about 3.3e9).  Exhaustive up to m <= 121 (n <= 121*121*65535, about 9.6e8: the host's libm sums
take about half a minute there), sampled blocks of 2^22 from there to the top; and sqrt(2 (m - 1)) for every m <= 225."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _host_sum(begin, end, chunk=1 << 24):
    tot = np.uint64(0)
    with np.errstate(over="ignore"):
        for b in range(begin, end, chunk):
            e = min(end, b + chunk)
            r = np.sqrt(np.arange(b, e, dtype=np.uint64).astype(np.float64))
            tot += r.view(np.uint64).sum(dtype=np.uint64)
    return int(tot)


def test_fp64_sqrt_exhaustive_to_m121(ffs):
    ctx = ffs.Context(64, 64)
    top = 121 * 121 * 65535 + 1
    step = 1 << 27
    for b in range(0, top, step):
        e = min(top, b + step)
        assert ctx.selftest_sqrt(b, e) == _host_sum(b, e), f"sqrt differs somewhere in [{b},{e})"


def test_fp64_sqrt_sampled_to_m225(ffs):
    ctx = ffs.Context(64, 64)
    lo, top = 121 * 121 * 65535 + 1, 225 * 225 * 65535 + 1
    rng = np.random.default_rng(225)
    starts = [lo, top - (1 << 22)] + [int(v) for v in rng.integers(lo, top - (1 << 22), size=30)]
    for b in starts:
        e = b + (1 << 22)
        assert ctx.selftest_sqrt(b, e) == _host_sum(b, e), f"sqrt differs somewhere in [{b},{e})"


def test_fp64_sqrt_of_two_m_minus_one(ffs):
    ctx = ffs.Context(64, 64)
    for m in range(1, 226):
        n = 2 * (m - 1)
        assert ctx.selftest_sqrt(n, n + 1) == _host_sum(n, n + 1), m
