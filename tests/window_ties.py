"""Tie frames at any window size (a helper module for tests/test_gpu_window.py; not a test).

tests/tie_windows.py tiles a frame with 7 x 7 cells; this builds the same kind of frame with (2kx+1) x (2ky+1) cells, so that the
window of a cell's centre pixel is exactly that cell.  Three of its families, at every size:
  a  signal ties b == d (m = n, x = n j^2, p = j^2 + nsig_s j) and p -+ 1; the dispersion test passes widely
  b  dispersion ties a == c (2 (m - 1) a perfect square, x = m t) and a = c -+ 2m; the signal test passes widely
  f  min_count: m == min_count and m == min_count - 1 round a centre that is otherwise strong
Masked pixels carry junk (65535, or >= 2^24 for 32-bit pixels).  The cells' own decisions (exact arithmetic and the oracle's
float64 sequence) come from tie_windows' helpers, which are generic in m, x, y.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import tie_windows as T


@dataclass
class WCell:
    family: str
    side: str
    m: int
    x: int
    y: int
    p: int
    row: int
    col: int
    exact: bool
    f64: bool


class WinBuilder:
    def __init__(self, kx, ky, prm: T.Params, dtype, seed):
        self.kx, self.ky, self.prm, self.dtype = kx, ky, prm, np.dtype(dtype)
        self.cw, self.ch = 2 * kx + 1, 2 * ky + 1
        self.n = self.cw * self.ch
        self.centre = ky * self.cw + kx
        self.vmax, self.junk = T.VMAX[self.dtype], T.JUNK[self.dtype]
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.cells = []   # (family, side, vals, valid)

    def cell(self, family, side, m, x, y, p):
        if not (1 <= m <= self.n) or p < 0 or p > self.vmax or x < p:
            return False
        others = ([] if (x == p and y == p * p) else None) if m == 1 else T.fill(m - 1, x - p, y - p * p, self.vmax)
        if others is None:
            return False
        vals = [self.junk] * self.n
        valid = [False] * self.n
        pos = [t for t in range(self.n) if t != self.centre]
        keep = sorted(self.rng.permutation(pos)[: m - 1].tolist())
        order = self.rng.permutation(len(others)).tolist()
        for t, o in zip(keep, order):
            vals[t], valid[t] = others[o], True
        vals[self.centre], valid[self.centre] = p, True
        self.cells.append((family, side, vals, valid))
        return True

    def y_wide(self, m, x, p):
        rg = T.y_range(m - 1, x - p, p, self.vmax)
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


def fam_a(B: WinBuilder):
    ns = B.prm.nsig_s
    assert ns == int(ns)
    m = B.n
    for j in range(2, 60, 3):
        x = m * j * j
        p0 = j * j + int(ns) * j
        for dp, side in ((-1, "below"), (0, "at"), (1, "above")):
            p = p0 + dp
            y = B.y_wide(m, x, p)
            if y is not None:
                B.cell("a", side, m, x, y, p)


def fam_b(B: WinBuilder):
    nb = B.prm.nsig_b
    assert nb == int(nb)
    ms = [s * s // 2 + 1 for s in range(2, 22, 2) if s * s // 2 + 1 <= B.n]
    for m in ms[-2:]:
        s = math.isqrt(2 * (m - 1))
        for t in range(3, 40, 4):
            x = m * t
            y0 = m * t * t + t * (m - 1) + int(nb) * t * s   # a == c
            for dy, side in ((-2, "below"), (0, "at"), (2, "above")):
                y = y0 + dy
                if (y - x) % 2:
                    continue
                # the smallest centres whose signal test passes (b > d + m): the window's spread leaves little room above the mean
                p_lo = t + int(B.prm.nsig_s * math.sqrt(t)) + 2
                for p in range(p_lo, p_lo + 12):
                    if B.cell("b", side, m, x, y, p):
                        break


def fam_f(B: WinBuilder):
    mc = B.prm.min_count
    for m, side in ((mc - 1, "below"), (mc, "at")):
        for p in (400, 1500, 5000):
            x = p + 5 * (m - 1)
            y = B.y_wide(m, x, p)
            if y is not None:
                B.cell("f", side, m, x, y, p)


def frame(kx, ky, dtype, prm: T.Params, width=620, seed=5):
    """(image, mask, [WCell]): cells on a grid that starts at an offset, background elsewhere."""
    B = WinBuilder(kx, ky, prm, dtype, seed)
    fam_a(B)
    fam_b(B)
    fam_f(B)
    cols = (width - 3) // B.cw
    rows = (len(B.cells) + cols - 1) // cols
    H = rows * B.ch + 5
    rng = np.random.default_rng(seed + 1)
    img = rng.poisson(3.0, size=(H, width)).astype(B.dtype)
    mask = np.ones((H, width), np.uint8)
    out = []
    for i, (family, side, vals, valid) in enumerate(B.cells):
        r0, c0 = 2 + (i // cols) * B.ch, 3 + (i % cols) * B.cw
        v = np.array(vals, dtype=np.int64).reshape(B.ch, B.cw)
        ok = np.array(valid, dtype=bool).reshape(B.ch, B.cw)
        img[r0:r0 + B.ch, c0:c0 + B.cw] = v.astype(B.dtype)
        mask[r0:r0 + B.ch, c0:c0 + B.cw] = ok.astype(np.uint8)
        m, x, y = T.window_stats(vals, valid)
        p = vals[B.centre]
        out.append(WCell(family, side, m, x, y, p, r0 + ky, c0 + kx,
                         T.exact_standard(prm, m, x, y, p), T.f64_standard(prm, m, x, y, p)))
    return img, mask, out
