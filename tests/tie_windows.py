"""Frames built so that the dispersion threshold's decisions sit at, and one step either side of, its ties (a helper module for
tests/test_tie_windows.py and tests/test_gpu_ties.py; not a test).

A frame is tiled with 7 x 7 cells: the 7 x 7 window of a cell's centre pixel is exactly that cell, so each centre gets a chosen
(m, sum p, sum p^2, p).  m is set by masking pixels of the cell (never its centre); masked pixels carry junk (65535, or >= 2^24
for 32-bit pixels), so a kernel that reads them is caught.  The grid starts at an offset, so that the centres fall on every
lane position mod 8 (7 and 8 are coprime) and cells straddle the strip edges of the streaming kernels (496 px for 16-bit pixels,
240 px for 32-bit ones, 56 px for the extended first pass).  Windows that straddle cells are whatever they hold: the tests
compare every pixel, the cells only guarantee that the ties are there.

Every cell records the family and the side it was built for, and its expected decision twice: in exact arithmetic (integers and
fractions) and with the oracle's own float64 operation sequence (baseline/spotfinder/standalone.cc:163-170).

Families (nsig_b, nsig_s, threshold, min_count, max_valid are parameters; each family is built for the given set):
  a  signal ties b == d (m = 49, x = 49 j^2) and windows with b^2 - d^2 in [-17, 17] \\ {0}; the dispersion test passes widely
  b  dispersion ties a == c (2 (m - 1) a perfect square) and a = c +- 2m; the signal test passes widely
  c  both at once, and the windows of m = 49, 48 closest to a == c
  d  the float32 screens' bands: |b^2 - d^2| <= 2^-16 d^2 (row-loop and drain screens), |a - c| around 2^-20 m y (extended drain)
  e  threshold: p == threshold, p == threshold +- 1 (floor and floor + 1 when the threshold is not an integer)
  f  min_count: m == min_count, m == min_count - 1
  g  max_valid: p == max_valid, p == max_valid + 1
  h  16-bit pixels: sum p in {65535, 65536, 65537} at ties; 65536 <= sum p < 2^17 with sum p^2 >= 2^32
  i  32-bit pixels: pixels 2^24 - 1 and 2^24 (inside windows and as centres), ties with sum p^2 around 2^46 and m sum p^2
     around 2^53
  j  the extended algorithm's final test src >= mean + nsig_s sqrt(mean) at its tie (a flat background k^2 round a block that
     the first pass marks as signal): p = k^2 + nsig_s k and p - 1

Generation is deterministic (integer construction, seeded PCG64 for the masks and the background) and cached per process.
"""
from __future__ import annotations

import functools
import hashlib
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

CELL = 7
BIG = 1 << 24
VMAX = {np.dtype(np.uint16): 65535, np.dtype(np.uint32): BIG - 1}
JUNK = {np.dtype(np.uint16): 65535, np.dtype(np.uint32): BIG + 12345}


@dataclass(frozen=True)
class Params:
    nsig_b: float = 6.0
    nsig_s: float = 3.0
    threshold: float = 0.0
    min_count: int = 2
    max_valid: int = -1

    def disp(self):
        """The oracle's DispParams for this set."""
        from oracle import oracle as O
        p = O.DispParams()
        O.lib().ffs_oracle_default_disp_params(O.C.byref(p))
        p.min_count, p.nsig_b, p.nsig_s, p.threshold = self.min_count, self.nsig_b, self.nsig_s, self.threshold
        return p

    def ctx_params(self):
        """ffs_amd.Context.set_params keywords for this set."""
        return dict(min_count=self.min_count, nsig_b=self.nsig_b, nsig_s=self.nsig_s, threshold=self.threshold,
                    max_valid=self.max_valid)


DEFAULT = Params()
# the parameter sets of tests/test_gpu_ties.py: the integer form, min_count with max_valid, the float64 square-root-free form,
# an integer nsig_b above 32 (float form), nsig = 0, thresholds that are not and that are integers
PARAM_SETS = {
    "default": DEFAULT,
    "mincount3_maxvalid": Params(min_count=3, max_valid=2000),
    "nsig_2.5_1.5": Params(nsig_b=2.5, nsig_s=1.5),
    "nsig_b33": Params(nsig_b=33.0),
    "nsig_0": Params(nsig_b=0.0, nsig_s=0.0),
    "threshold_40.5": Params(threshold=40.5),
    "threshold_41": Params(threshold=41.0),
}


# ---------------------------------------------------------------------------------------------------------------- decisions
def window_stats(vals, valid):
    """(m, x, y) over the valid pixels below 2^24 (standalone.cc:90)."""
    m = x = y = 0
    for v, ok in zip(vals, valid):
        if ok and v < BIG:
            m += 1
            x += v
            y += v * v
    return m, x, y


def _gt_sqrt(lhs, k2):
    """lhs > sqrt(k2) exactly (lhs a Fraction or int, k2 >= 0 a Fraction)."""
    if lhs <= 0:
        return False if k2 > 0 or lhs < 0 else False
    return lhs * lhs > k2


def exact_standard(prm: Params, m, x, y, p, centre_valid=True):
    """standalone.cc:163-170 in exact arithmetic: a > c and b > d with real square roots."""
    if not (centre_valid and m >= prm.min_count and x >= 0 and p > Fraction(prm.threshold)):
        return False
    nb, ns = Fraction(prm.nsig_b), Fraction(prm.nsig_s)
    a = m * y - x * x - x * (m - 1)
    b = m * p - x
    return _gt_sqrt(Fraction(a), nb * nb * x * x * 2 * (m - 1)) and _gt_sqrt(Fraction(b), ns * ns * x * m)


def exact_first_pass(prm: Params, m, x, y, p, centre_valid=True):
    """The extended algorithm's first pass (baseline.cpp:468-473, with the device kernels' max_valid rule)."""
    if not (centre_valid and m >= prm.min_count and x >= 0):
        return False
    if prm.max_valid >= 0 and p > prm.max_valid:
        return False
    nb = Fraction(prm.nsig_b)
    return _gt_sqrt(Fraction(m * y - x * x - x * (m - 1)), nb * nb * x * x * 2 * (m - 1))


def f64_standard(prm: Params, m, x, y, p, centre_valid=True):
    """The oracle's operation sequence on doubles (one rounding per operation)."""
    m, x, y, src = (np.float64(v) for v in (m, x, y, p))
    if not (centre_valid and m >= prm.min_count and x >= 0 and src > np.float64(prm.threshold)):
        return False
    a = m * y - x * x - x * (m - 1.0)
    b = m * src - x
    c = x * np.float64(prm.nsig_b) * np.sqrt(2.0 * (m - 1.0))
    d = np.float64(prm.nsig_s) * np.sqrt(x * m)
    return bool(a > c and b > d)


def f64_first_pass(prm: Params, m, x, y, p, centre_valid=True):
    m, x, y = (np.float64(v) for v in (m, x, y))
    if not (centre_valid and m >= prm.min_count and x >= 0):
        return False
    if prm.max_valid >= 0 and p > prm.max_valid:
        return False
    a = m * y - x * x - x * (m - 1.0)
    c = x * np.float64(prm.nsig_b) * np.sqrt(2.0 * (m - 1.0))
    return bool(a > c)


# --------------------------------------------------------------------------------------------------------------------- fill
def fill(k, X, Y, vmax):
    """k values in [0, vmax] with sum X and sum of squares Y, or None.  Starts from the most even split and moves units from a
    small value to a large one: t units from v_i to v_j add 2 t (v_j - v_i + t) to the sum of squares."""
    if k == 0:
        return [] if X == 0 and Y == 0 else None
    if X < 0 or Y < 0 or X > k * vmax:
        return None
    q, r = divmod(X, k)
    v = [q + 1] * r + [q] * (k - r)
    y0 = r * (q + 1) ** 2 + (k - r) * q * q
    if Y < y0 or (Y - y0) % 2:
        return None
    D = (Y - y0) // 2
    for _ in range(20 * k + 200):
        if D == 0:
            return v
        order = sorted(range(k), key=lambda t: v[t])
        i = next((t for t in order if v[t] > 0), None)
        j = next((t for t in reversed(order) if v[t] < vmax and t != i), None)
        if i is None or j is None:
            return None
        g = v[j] - v[i]
        if g >= 0:
            # largest t with t (g + t) <= D
            t = (math.isqrt(g * g + 4 * D) - g) // 2
            t = min(t, v[i], vmax - v[j])
            if t >= 1:
                v[i] -= t
                v[j] += t
                D -= t * (g + t)
                continue
        # the biggest single-unit move is too big: a pair whose gap makes it exactly, else the largest that fits
        best = None
        for a_ in range(k):
            if v[a_] == 0:
                continue
            for b_ in range(k):
                if b_ == a_ or v[b_] >= vmax:
                    continue
                inc = v[b_] - v[a_] + 1
                if inc == D:
                    best = (inc, a_, b_)
                    break
                if 1 <= inc < D and (best is None or inc > best[0]):
                    best = (inc, a_, b_)
            if best is not None and best[0] == D:
                break
        if best is None:
            return None
        inc, a_, b_ = best
        v[a_] -= 1
        v[b_] += 1
        D -= inc
    return None


def y_range(k, X, p, vmax):
    """The reachable sums of squares of a window with centre p and k other pixels summing to X (same parity steps of 2)."""
    if k == 0 or X < 0 or X > k * vmax:
        return None
    q, r = divmod(X, k)
    lo = r * (q + 1) ** 2 + (k - r) * q * q
    nf, rest = divmod(X, vmax)
    hi = nf * vmax * vmax + rest * rest
    return p * p + lo, p * p + hi


# --------------------------------------------------------------------------------------------------------------------- cells
@dataclass
class Cell:
    family: str
    side: str                  # "below" (not strong side), "at" (the tie itself), "above"; or a family's own label
    vals: list                 # 49 values, row-major; [24] is the centre
    valid: list                # 49 mask bits
    m: int = 0
    x: int = 0
    y: int = 0
    p: int = 0
    row: int = -1              # centre in the frame
    col: int = -1
    exact: bool = False        # standard algorithm, exact arithmetic
    f64: bool = False          # ... the oracle's float64 operations
    first_exact: bool = False  # extended first pass
    first_f64: bool = False


class Builder:
    def __init__(self, prm: Params, dtype, seed):
        self.prm, self.dtype = prm, np.dtype(dtype)
        self.vmax, self.junk = VMAX[self.dtype], JUNK[self.dtype]
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.cells = []

    def cell(self, family, side, m, x, y, p, extra=None):
        """A cell whose centre window has exactly (m, x, y) and centre p; False when no fill reaches it."""
        if not (1 <= m <= 49) or p < 0 or p > self.vmax or x < p:
            return False
        if m == 1:
            others = [] if (x == p and y == p * p) else None
        else:
            others = fill(m - 1, x - p, y - p * p, self.vmax)
        if others is None:
            return False
        vals = [self.junk] * 49
        valid = [False] * 49
        pos = [t for t in range(49) if t != 24]
        keep = sorted(self.rng.permutation(pos)[: m - 1].tolist())
        order = self.rng.permutation(len(others)).tolist()
        for t, o in zip(keep, order):
            vals[t], valid[t] = others[o], True
        vals[24], valid[24] = p, True
        if extra:
            extra(vals, valid)
        self.add(family, side, vals, valid)
        return True

    def add(self, family, side, vals, valid):
        m, x, y = window_stats(vals, valid)
        p = vals[24]
        c = Cell(family, side, list(vals), list(valid), m, x, y, p)
        c.exact = exact_standard(self.prm, m, x, y, p, valid[24])
        c.f64 = f64_standard(self.prm, m, x, y, p, valid[24])
        c.first_exact = exact_first_pass(self.prm, m, x, y, p, valid[24])
        c.first_f64 = f64_first_pass(self.prm, m, x, y, p, valid[24])
        self.cells.append(c)

    # a y for (m, x, p) whose dispersion passes widely (a >= 3 c + 8 m), inside the reachable range
    def y_wide(self, m, x, p):
        rg = y_range(m - 1, x - p, p, self.vmax)
        if rg is None:
            return None
        c = float(self.prm.nsig_b) * x * math.sqrt(2 * (m - 1))
        y = max(rg[0], (x * x + x * (m - 1) + int(3 * c) + 8 * m) // m + 1)
        y += (y - x) % 2
        for _ in range(6):
            if y <= rg[1]:
                return y
            y = (y + rg[0]) // 2
            y += (y - x) % 2
        return None


def _side(diff):
    return "at" if diff == 0 else ("above" if diff > 0 else "below")


def _ns2(prm):
    ns = Fraction(prm.nsig_s)
    return ns * ns


def _nb(prm):
    return Fraction(prm.nsig_b)


def fam_a(B: Builder, n_near=12):
    """Signal ties b == d (m = 49, x = 49 j^2, p = j^2 + nsig_s j) and windows with b^2 - d^2 in [-17, 17] \\ {0}."""
    prm, ns = B.prm, Fraction(B.prm.nsig_s)
    m = 49
    for j in range(1, 30):
        x = m * j * j
        for dp in (0, -1, 1):
            p = j * j + ns * j + dp
            if p.denominator != 1 or p < 0:
                continue
            p = int(p)
            y = B.y_wide(m, x, p)
            if y is not None:
                B.cell("a", _side(m * p - x - ns * m * j), m, x, y, p)
    # b^2 - d^2 = (m p - x)^2 - nsig_s^2 x m small and not zero
    ns2 = _ns2(prm)
    got = {"below": 0, "above": 0}
    for m in (49, 48, 45, 40):
        xs = np.arange(1, min(65536, 49 * B.vmax), dtype=np.int64)
        d = np.sqrt(float(ns2) * xs * m)
        for off in (0, 1):
            ps = np.floor((xs + d) / m).astype(np.int64) + off
            b = m * ps - xs
            num, den = ns2.numerator, ns2.denominator
            diff = b * b * den - num * xs * m          # (b^2 - d^2) den
            sel = np.flatnonzero((diff != 0) & (np.abs(diff) <= 17 * den) & (b > 0) & (ps <= B.vmax))
            for t in sel:
                side = "above" if diff[t] > 0 else "below"
                if got[side] >= n_near:
                    continue
                x, p = int(xs[t]), int(ps[t])
                y = B.y_wide(m, x, p)
                if y is not None and B.cell("a", side, m, x, y, p):
                    got[side] += 1


def _disp_tie_y(prm, m, x):
    """y with a == c exactly for 2 (m - 1) = r^2, or None."""
    r = math.isqrt(2 * (m - 1))
    if r * r != 2 * (m - 1):
        return None
    c = _nb(prm) * r * x
    if c.denominator != 1:
        return None
    num = x * x + x * (m - 1) + int(c)
    if num % m:
        return None
    y = num // m
    return y if (y - x) % 2 == 0 else None


def _signal_wide_p(B, m, x, y, lo_factor=1.15):
    """Centre values whose signal test passes widely and whose window fills: the first that works."""
    d = math.sqrt(float(_ns2(B.prm)) * x * m)
    p0 = max(int((x + lo_factor * d + 2) / m) + 1, 0)
    for p in list(range(p0, p0 + 6)) + [p0 + 10, p0 + 25, p0 + 60]:
        if p > B.vmax or p * p > y:
            break
        rg = y_range(m - 1, x - p, p, B.vmax)
        if rg and rg[0] <= y <= rg[1] and fill(m - 1, x - p, y - p * p, B.vmax) is not None:
            return p
    return None


def fam_b(B: Builder, per_m=10, xs=None):
    """Dispersion ties a == c and a = c +- 2m (y +- 2), the signal test passing widely."""
    for m in (3, 9, 19, 33):
        got = 0
        for x in (xs if xs is not None else range(40, 60000, 7)):
            y = _disp_tie_y(B.prm, m, x)
            if y is None:
                continue
            p = _signal_wide_p(B, m, x, y)
            if p is None:
                continue
            ok = [B.cell("b", side, m, x, y + dy, p) for side, dy in (("at", 0), ("below", -2), ("above", 2))]
            got += all(ok)
            if got >= per_m:
                break


def fam_c(B: Builder, n=6):
    """a == c and b == d in one window (x = m j^2); and the m = 49, 48 windows closest to a == c (c irrational there)."""
    ns, nb = Fraction(B.prm.nsig_s), _nb(B.prm)
    got = 0
    for m in (3, 9, 19, 33):
        r = math.isqrt(2 * (m - 1))
        for j in range(1, 200):
            x = m * j * j
            p = j * j + ns * j
            if p.denominator != 1:
                continue
            y = _disp_tie_y(B.prm, m, x)
            if y is None:
                continue
            if B.cell("c", "at", m, x, y, int(p)):
                got += 1
                B.cell("c", "below", m, x, y - 2, int(p))
                B.cell("c", "above", m, x, y + 2, int(p) + 1)
            if got >= n * 4:
                break
    # m = 49, 48: for each x the y with a just above and just below c; the closest few (relative to c) kept
    for m in (49, 48):
        cand = []
        for x in range(50, 20000, 3):
            c = float(nb) * x * math.sqrt(2 * (m - 1))
            base = x * x + x * (m - 1)
            y_lo = (base + int(c)) // m
            for y in (y_lo - 1, y_lo, y_lo + 1, y_lo + 2):
                if (y - x) % 2:
                    continue
                a = m * y - base
                cand.append((abs(a - c) / max(c, 1.0), x, y))
        cand.sort()
        kept = {"below": 0, "above": 0}
        for _, x, y in cand:
            a = m * y - x * x - x * (m - 1)
            side = "above" if a > 0 and Fraction(a) ** 2 > nb * nb * x * x * 2 * (m - 1) else "below"
            if kept[side] >= n:
                continue
            p = _signal_wide_p(B, m, x, y)
            if p is not None and B.cell("c", side, m, x, y, p):
                kept[side] += 1
            if min(kept.values()) >= n:
                break


def fam_d(B: Builder, n=10):
    """Inside the float32 screens' bands: 0 < |b^2 - d^2| <= 2^-16 d^2 (dispersion passing widely), and |a - c| at half and one
    and a half times 2^-20 m y on both sides (the extended drain's sure / maybe band)."""
    ns2 = _ns2(B.prm)
    if ns2 > 0:
        got = {"below": 0, "above": 0}
        for m in (49, 44, 37, 30, 25):
            xs = np.arange(100, min(65536, 40 * B.vmax), 13, dtype=np.int64)
            d2 = float(ns2) * xs * m
            for off in (0, 1):
                ps = np.floor((xs + np.sqrt(d2)) / m).astype(np.int64) + off
                b = (m * ps - xs).astype(np.float64)
                rel = (b * b - d2) / d2
                sel = np.flatnonzero((np.abs(rel) <= 2.0 ** -16) & (b > 0) & (ps <= B.vmax))
                for t in sel:
                    x, p = int(xs[t]), int(ps[t])
                    num = (m * p - x) ** 2 - ns2 * x * m
                    if num == 0 or abs(num) > ns2 * x * m / 65536:
                        continue
                    side = "above" if num > 0 else "below"
                    if got[side] >= n:
                        continue
                    y = B.y_wide(m, x, p)
                    if y is not None and B.cell("d16", side, m, x, y, p):
                        got[side] += 1
    # the extended first pass: a - c = f 2^-20 m y
    nb = float(B.prm.nsig_b)
    got = {}
    for m in (49, 33, 19, 9):
        for x in range(3000, 60000, 997):
            if B.dtype == np.uint16 and x >= 65536:
                break
            c = nb * x * math.sqrt(2 * (m - 1))
            base = x * x + x * (m - 1)
            y_tie = (base + c) / m
            for f, side in ((-1.5, "out_below"), (-0.5, "in_below"), (0.5, "in_above"), (1.5, "out_above")):
                y = int(round(y_tie + f * 2.0 ** -20 * y_tie))
                y += (y - x) % 2
                p = x // m
                if got.get(side, 0) < n and B.cell("d20", side, m, x, y, p):
                    got[side] = got.get(side, 0) + 1


def _strong_template(B, p, m):
    """A window with centre p and m pixels that is strong by a wide margin when p passes the other tests (others near 0)."""
    k = m - 1
    X = min(k, p // 50)
    q, r = divmod(X, k) if k else (0, 0)
    y = p * p + (r * (q + 1) ** 2 + (k - r) * q * q if k else 0)
    return p + X, y


def fam_e(B: Builder):
    """threshold: p == t, t +- 1; t not an integer: floor(t), floor(t) + 1."""
    t = B.prm.threshold
    ps = [int(t) - 1, int(t), int(t) + 1] if t == int(t) else [math.floor(t), math.floor(t) + 1]
    for p in ps:
        if p < 1:
            continue
        for m in (49, 25, 9):
            x, y = _strong_template(B, p, m)
            side = "at" if p == t else ("above" if p > t else "below")
            B.cell("e", side, m, x, y, p)


def fam_f(B: Builder):
    """min_count: m == min_count and m == min_count - 1, the window otherwise strong."""
    mc = B.prm.min_count
    for m, side in ((mc, "at"), (mc - 1, "below"), (mc + 1, "above")):
        if m < 1:
            continue
        for p in (200, 3000, min(60000, B.vmax)):
            x, y = _strong_template(B, max(p, int(B.prm.threshold) + 1), m)
            B.cell("f", side, m, x, y, max(p, int(B.prm.threshold) + 1))


def fam_g(B: Builder):
    """max_valid: p == max_valid and max_valid + 1 (strong windows otherwise)."""
    mv = B.prm.max_valid
    if mv < 0:
        return
    for p, side in ((mv - 1, "below"), (mv, "at"), (mv + 1, "above")):
        for m in (49, 30, 9):
            x, y = _strong_template(B, p, m)
            B.cell("g", side, m, x, y, p)


def fam_h(B: Builder):
    """16-bit pixels: sum p in {65535, 65536, 65537} at and next to ties; 65536 <= sum p < 2^17 with sum p^2 >= 2^32."""
    ns = Fraction(B.prm.nsig_s)
    for x in (65535, 65536, 65537):
        fam_b_at = 0
        for m in (3, 9, 19, 33):
            y = _disp_tie_y(B.prm, m, x)
            if y is None:
                continue
            p = _signal_wide_p(B, m, x, y)
            if p is None:
                continue
            for side, dy in (("at", 0), ("below", -2), ("above", 2)):
                fam_b_at += B.cell("h", side, m, x, y + dy, p)
        # signal ties: x m a perfect square, p = (x + nsig_s sqrt(x m)) / m an integer
        for m in range(2, 50):
            s = math.isqrt(x * m)
            if s * s != x * m:
                continue
            for dp in (0, -1, 1):
                p = (x + ns * s) / m + dp
                if p.denominator != 1 or not (0 <= p <= B.vmax):
                    continue
                p = int(p)
                y = B.y_wide(m, x, p)
                if y is not None:
                    B.cell("h", _side(m * p - x - ns * s), m, x, y, p)
    # sum p^2 just above 2^32 (a 32-bit sum would wrap to almost nothing): a saturated centre and a few more
    for extra2 in (131071, 131072, 131769, 200000, 1 << 20):
        for m in (9, 25, 49):
            p = 65535
            Y = (1 << 32) + (extra2 - 131071) - p * p
            for X in range(math.isqrt(Y), math.isqrt(Y) + (m - 1) * 40):
                if (Y - X) % 2 == 0 and fill(m - 1, X, Y, B.vmax) is not None:
                    B.cell("h", "y_over_2^32", m, p + X, p * p + Y, p)
                    break
    # dispersion ties with sum p^2 > 2^32 (m = 3, x around 120000)
    got = 0
    for x in range(114000, 131071, 37):
        y = _disp_tie_y(B.prm, 3, x)
        if y is None or y < (1 << 32):
            continue
        p = _signal_wide_p(B, 3, x, y)
        if p is not None and B.cell("h", "tie_y_over_2^32", 3, x, y, p):
            got += 1
            B.cell("h", "tie_y_over_2^32", 3, x, y + 2, p)
        if got >= 6:
            break


def fam_i(B: Builder):
    """32-bit pixels: 2^24 - 1 and 2^24 inside windows and as centres; ties with y around 2^46 and m y around 2^53."""
    for v in (BIG - 1, BIG, BIG + 1):
        def put(vals, valid, v=v):
            vals[10], valid[10] = v, True
        for p in (5, 400, 3000):
            x, y = _strong_template(B, p, 30)
            B.cell("i", f"pixel_{v}", 30, x, y, p, extra=put)
        # as the centre (the oracle tests src itself; its window leaves it out when it is >= 2^24)
        for m in (49, 20):
            x, y = _strong_template(B, v if v < BIG else 3000, m)
            if v < BIG:
                B.cell("i", f"centre_{v}", m, x, y, v)
            else:
                def centre(vals, valid, v=v):
                    vals[24] = v
                B.cell("i", f"centre_{v}", m, x, y, 3000, extra=centre)
    # y around 2^46 and m y around 2^53 (dispersion ties and their neighbours)
    # (the frame's sum of p^2 has to stay below 2^53: a few of each)
    for m, target, label, n in ((33, 1 << 46, "y_2^46", 1), (19, 1 << 46, "y_2^46", 1), (33, (1 << 53) // 33, "my_2^53", 1)):
        x0 = math.isqrt(target * m)
        got = {"lo": 0, "hi": 0}
        for dx in range(0, 400000, 7):
            for x in (x0 - dx, x0 + dx):
                y = _disp_tie_y(B.prm, m, x)
                if y is None:
                    continue
                half = "lo" if y < target else "hi"
                if got[half] >= n:
                    continue
                p = _signal_wide_p(B, m, x, y)
                if p is None:
                    continue
                if B.cell("i", f"{label}_{half}_at", m, x, y, p):
                    got[half] += 1
                    B.cell("i", f"{label}_{half}_below", m, x, y - 2, p)
                    B.cell("i", f"{label}_{half}_above", m, x, y + 2, p)
            if min(got.values()) >= n:
                break


# --------------------------------------------------------------------------------------------------------------------- frames
@dataclass
class TieFrame:
    image: np.ndarray
    mask: np.ndarray
    cells: list
    params: Params
    ext_cells: list            # family j: (row, col, family, side, expected)
    background: np.ndarray     # the frame without its cells and blocks

    def split(self, n):
        """n frames (same mask) that hold every n-th cell each on the background, no family j: sparse enough for the 16-bit
        streaming kernel's wave logs, which a whole tie frame overflows.  -> (frames, cells of each frame)"""
        frames, cells = [], []
        for i in range(n):
            img = self.background.copy()
            own = self.cells[i::n]
            for c in own:
                img[c.row - 3:c.row + 4, c.col - 3:c.col + 4] = self.image[c.row - 3:c.row + 4, c.col - 3:c.col + 4]
            frames.append(img)
            cells.append(own)
        return np.stack(frames), cells

    def digest(self):
        h = hashlib.sha256()
        h.update(np.ascontiguousarray(self.image).tobytes())
        h.update(np.ascontiguousarray(self.mask).tobytes())
        return h.hexdigest()


GRID_OFFSET = (2, 5)            # (rows, columns) of plain background before the first cell


def _ext_block(k, p, nsig_s, cellmask=None):
    """21 x 21 region: flat k^2, a 5 x 5 block of bright pixels whose centre is p."""
    r = np.full((21, 21), k * k, np.int64)
    r[8:13, 8:13] = k * k + 40 * k + 100
    r[10, 10] = p
    return r


def _fam_j(prm, dtype, n_blocks):
    """(p, k, side) of the extended final-pass ties: p = k^2 + nsig_s k (>= holds) and p - 1."""
    out = []
    ns = Fraction(prm.nsig_s)
    vmax = VMAX[np.dtype(dtype)] if prm.max_valid < 0 else prm.max_valid      # (the block must stay valid)
    for k in range(4, 250, 7 if prm.max_valid < 0 else 1):
        t = k * k + ns * k
        if t.denominator != 1 or t + 1 > vmax or k * k + 40 * k + 100 > vmax:
            continue
        out.append((int(t), k, "at"))
        out.append((int(t) - 1, k, "below"))
        if len(out) >= n_blocks:
            break
    return out


@functools.lru_cache(maxsize=None)
def frame(dtype_name="uint16", prm: Params = DEFAULT, width=1100, spread=1, ext_blocks=True):
    """The tie frame of a pixel type and parameter set; spread = 2 leaves every other cell of the grid (in both directions) to
    the background, which keeps the strong pixels sparser; ext_blocks=False leaves out family j (whose flat blocks have strong
    edges)."""
    dtype = np.dtype(dtype_name)
    B = Builder(prm, dtype, seed=20261016 + (dtype.itemsize << 8))
    fam_a(B)
    fam_b(B)
    fam_c(B)
    fam_d(B)
    fam_e(B)
    fam_f(B)
    fam_g(B)
    if dtype == np.uint16:
        fam_h(B)
    else:
        fam_i(B)
    cells = B.cells
    order = B.rng.permutation(len(cells)).tolist()      # families spread over lane positions and strips
    cells = [cells[t] for t in order]

    oy, ox = GRID_OFFSET
    ncol = (width - ox - 2) // (CELL * spread)
    nrow = -(-len(cells) // ncol) * spread
    blocks = _fam_j(prm, dtype, n_blocks=(width - 2) // 21) if ext_blocks else []
    H = oy + nrow * CELL + 3 + (21 + 2 if blocks else 0) + 2
    W = width
    img = B.rng.poisson(1.0, (H, W)).astype(np.int64)
    background = img.astype(dtype)
    mask = np.ones((H, W), np.uint8)
    for t, c in enumerate(cells):
        r0, c0 = oy + (t // ncol) * CELL * spread, ox + (t % ncol) * CELL * spread
        img[r0:r0 + CELL, c0:c0 + CELL] = np.array(c.vals, np.int64).reshape(CELL, CELL)
        mask[r0:r0 + CELL, c0:c0 + CELL] = np.array(c.valid, np.uint8).reshape(CELL, CELL)
        c.row, c.col = r0 + 3, c0 + 3
    ext_cells = []
    if blocks:
        r0 = oy + nrow * CELL + 3
        img[r0 - 1:r0 + 22, :] = 0
        for t, (p, k, side) in enumerate(blocks):
            c0 = 1 + 21 * t
            img[r0:r0 + 21, c0:c0 + 21] = _ext_block(k, p, prm.nsig_s)
            ext_cells.append((r0 + 10, c0 + 10, "j", side,
                              p >= k * k + Fraction(prm.nsig_s) * k and p > Fraction(prm.threshold)))
    assert img.max() <= np.iinfo(dtype).max and img.min() >= 0
    img = img.astype(dtype)
    # the oracle's summed-area table is exact only while its sums stay below 2^53: a window's y adds two entries
    # of the table before it subtracts, so the frame's sum of p^2 has to stay below 2^52
    ok = (mask != 0) & (img.astype(np.int64) < BIG)
    v = img.astype(object)[ok]
    assert int(sum(int(t) * int(t) for t in v.tolist())) < (1 << 52)
    return TieFrame(img, mask, cells, prm, ext_cells, background)


def families(tf: TieFrame):
    """{(family, side): count} of a frame's cells."""
    out = {}
    for c in tf.cells:
        out[(c.family, c.side)] = out.get((c.family, c.side), 0) + 1
    for _, _, fam, side, _ in tf.ext_cells:
        out[(fam, side)] = out.get((fam, side), 0) + 1
    return out


def dense_frame(shape, dtype, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    top = 65535 if np.dtype(dtype) == np.uint16 else BIG - 1
    return np.minimum(rng.poisson(300.0, shape) + (rng.random(shape) < 0.01) * 20000, top).astype(dtype)
