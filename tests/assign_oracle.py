"""The rule of index assignment (csrc/assign_model.hpp) in NumPy float64 and Python integers: every float64 operation
is one ufunc call, in the header's order with the header's parentheses; no np.linalg.inv, no `@`, no np.round.  The tests hold the check
program, the host-only entries and the GPU to these results byte for byte."""
import itertools
import math

import numpy as np

F = np.float64
ABSENCE_TESTS = 111
SINGULAR = 1
LIMIT = 524288.0          # 2^19: |hf| at or beyond it is out of range
BIAS = 1 << 19
Q40 = 1099511627776.0     # 2^40
PI_4 = math.pi / 4
ASSIGNMENT_DT = np.dtype([("status", "<u4"), ("n_accepted", "<u4"), ("n_indexed", "<u4"), ("n_out_of_range", "<u4"), ("sum_lsq_q40", "<u8"),
                          ("absent0", "<u4", (ABSENCE_TESTS,)), ("reserved", "<u4")])
ABSENCE_TEST_DT = np.dtype([("v", "<i4", (3,)), ("modularity", "<i4"), ("transform", "<i4", (9,)), ("reserved", "<i4")])
SETTING_DT = np.dtype([("triple", "<u4", (3,)), ("reserved", "<u4"), ("axes", "<f8", (9,)), ("A", "<f8", (9,))])
assert ASSIGNMENT_DT.itemsize == 472 and ABSENCE_TEST_DT.itemsize == 56 and SETTING_DT.itemsize == 160


def inverse(A):
    """(Ai, ok) by cofactors in the header's order; ok False when det == 0 or an entry is not finite (Ai is then zeros)"""
    a = [F(x) for x in np.asarray(A, F).reshape(9)]
    with np.errstate(all="ignore"):
        c00 = a[4] * a[8] - a[5] * a[7]
        c01 = a[5] * a[6] - a[3] * a[8]
        c02 = a[3] * a[7] - a[4] * a[6]
        det = (a[0] * c00 + a[1] * c01) + a[2] * c02
        if det == 0.0:
            return np.zeros(9, F), False
        o = np.array([c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                      c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                      c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det], F)
    if not np.all(np.isfinite(o)):
        return np.zeros(9, F), False
    return o, True


def round_half_away(hf):
    t = np.trunc(hf)
    d = hf - t
    return np.where(d >= 0.5, t + 1.0, np.where(d <= -0.5, t - 1.0, t))


def absence_table():
    pts = [p for p in itertools.product(range(-5, 6), repeat=3)]
    pts.sort(key=lambda p: (p[0] * p[0] + p[1] * p[1] + p[2] * p[2], -(p[0] + p[1] + p[2]), (-p[0], -p[1], -p[2])))
    assert pts[0] == (0, 0, 0)
    pts = pts[1:]

    def cross(a, b):
        return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    reps = []
    for p in pts:
        if dot(p, p) > 6:
            break
        if not any(cross(p, r) == (0, 0, 0) for r in reps):
            reps.append(p)
    out = np.zeros(len(reps) * 3, ABSENCE_TEST_DT)
    k = 0
    for v in reps:
        for m in (2, 3, 5):
            cand = [p for p in pts if dot(p, v) % m == 0]
            first = cand[0]
            i = 1
            while cross(cand[i], first) == (0, 0, 0):
                i += 1
            second = cand[i]
            i += 1
            while dot(cross(second, first), cand[i]) == 0:
                i += 1
            third = cand[i]
            rows = [first, second, third]
            if dot(cross(first, second), third) < 0:
                rows = [second, first, third]
            out[k]["v"], out[k]["modularity"], out[k]["transform"] = v, m, [c for r in rows for c in r]
            k += 1
    return out


_TABLE = {}


def table():
    if "t" not in _TABLE:
        _TABLE["t"] = absence_table()
    return _TABLE["t"]


def select(rlp, phi, dmin, osc_start_deg):
    r = np.asarray(rlp, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        norm = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        out = ~((F(1.0) / norm <= F(dmin)) | (np.asarray(phi, F) * F(180.0 / math.pi) > F(osc_start_deg) + F(360.0)))
    return out.astype(np.uint8)


def assign(rlp, phi, A, tolerance=0.3, selected=None):
    """One setting: (record of ASSIGNMENT_DT, hkl (n, 3) int32, lsq (n) float64)"""
    r = np.ascontiguousarray(np.asarray(rlp, F).reshape(-1, 3))
    phi = np.asarray(phi, F).reshape(-1)
    n = len(r)
    sel = np.ones(n, bool) if selected is None else np.asarray(selected).astype(bool)
    rec = np.zeros((), ASSIGNMENT_DT)
    hkl = np.zeros((n, 3), np.int32)
    lsq = np.full(n, -1.0, F)
    Ai, ok = inverse(A)
    if not ok:
        rec["status"] = SINGULAR
        return rec, hkl, lsq
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    hf = [(Ai[3 * j] * r0 + Ai[3 * j + 1] * r1) + Ai[3 * j + 2] * r2 for j in range(3)]
    oor = sel & ((np.abs(hf[0]) >= LIMIT) | (np.abs(hf[1]) >= LIMIT) | (np.abs(hf[2]) >= LIMIT))
    use = sel & ~oor
    h = [np.where(use, round_half_away(np.where(use, x, 0.0)), 0.0) for x in hf]
    d = [h[j] - np.where(use, hf[j], 0.0) for j in range(3)]
    l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    tol = F(tolerance)
    hi = np.stack(h, 1).astype(np.int32)
    accepted = use & (l2 <= tol * tol) & np.any(hi != 0, axis=1)
    lsq[use] = l2[use]
    rec["n_out_of_range"] = int(oor.sum())
    rec["n_accepted"] = int(accepted.sum())
    dead = np.zeros(n, bool)
    groups = {}
    for i in np.flatnonzero(accepted):
        groups.setdefault(tuple(hi[i]), []).append(int(i))
    for members in groups.values():
        for x, a in enumerate(members):
            for b in members[x + 1:]:
                if dead[a] or dead[b]:
                    continue
                if abs(phi[a] - phi[b]) > PI_4:
                    continue
                if l2[b] < l2[a]:
                    dead[a] = True
                else:
                    dead[b] = True
    indexed = accepted & ~dead
    hkl[indexed] = hi[indexed]
    rec["n_indexed"] = int(indexed.sum())
    rec["sum_lsq_q40"] = int(sum(int(x) for x in (l2[indexed] * F(Q40)).astype(np.uint64)))
    t = table()
    hh = hi[indexed].astype(np.int64)
    for k in range(ABSENCE_TESTS):
        rec["absent0"][k] = int(np.count_nonzero((hh @ t[k]["v"].astype(np.int64)) % int(t[k]["modularity"]) == 0))
    return rec, hkl, lsq


def assign_many(rlp, phi, A, tolerance=0.3, selected=None):
    A = np.asarray(A, F).reshape(-1, 9)
    n = len(np.asarray(rlp, F).reshape(-1, 3))
    recs, hkl, lsq = np.zeros(len(A), ASSIGNMENT_DT), np.zeros((len(A), n, 3), np.int32), np.zeros((len(A), n), F)
    for k in range(len(A)):
        recs[k], hkl[k], lsq[k] = assign(rlp, phi, A[k], tolerance, selected)
    return recs, hkl, lsq


def detect(rec, threshold=0.9):
    if int(rec["n_indexed"]) == 0:
        return -1
    for k in range(ABSENCE_TESTS):
        if F(int(rec["absent0"][k])) / F(int(rec["n_indexed"])) > F(threshold):
            return k
    return -1


def matmul(M, D):
    return np.array([(M[3 * i] * D[j] + M[3 * i + 1] * D[3 + j]) + M[3 * i + 2] * D[6 + j] for i in range(3) for j in range(3)], F)


def reindex(A, t):
    """A' (9) after absence test t's transform, or None when an inverse on the way is singular"""
    direct, ok = inverse(A)
    if not ok:
        return None
    Ti, ok = inverse(table()[t]["transform"].astype(F))
    if not ok:
        return None
    M = np.array([Ti[0], Ti[3], Ti[6], Ti[1], Ti[4], Ti[7], Ti[2], Ti[5], Ti[8]], F)
    out, ok = inverse(matmul(M, direct))
    return out if ok else None


def correct(rlp, phi, A, tolerance=0.3, selected=None, threshold=0.9):
    """(A', record, hkl, rounds): assign, detect, reindex, assign again until nothing is detected"""
    A = np.asarray(A, F).reshape(9)
    for rounds in range(17):
        rec, hkl, _ = assign(rlp, phi, A, tolerance, selected)
        t = detect(rec, threshold)
        if t < 0:
            return A, rec, hkl, rounds
        A = reindex(A, t)
    raise RuntimeError("no end after 16 rounds")


def angle_deg(a, b):
    def norm(v):
        return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    nd = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (norm(a) * norm(b))
    if abs(nd - 1.0) < 1e-6:
        return 0.0
    if abs(nd + 1.0) < 1e-6:
        return 180.0
    return math.acos(nd) * 180.0 / math.pi


def settings(vectors, max_combinations=1000, min_angle=20.0):
    """Candidate settings (SETTING_DT) from basis vectors (m, 3), combinations.cc without the Niggli reduction"""
    v = [[float(x) for x in row] for row in np.asarray(vectors, F).reshape(-1, 3)][:100]
    triples = [(i, j, k) for i in range(len(v)) for j in range(i + 1, len(v)) for k in range(j + 1, len(v))]
    triples.sort(key=lambda t: t[0] * t[0] + t[1] * t[1] + t[2] * t[2])   # (stable)
    out = []
    for (i, j, k) in triples[:max_combinations]:
        v1, v2, v3 = list(v[i]), list(v[j]), list(v[k])
        gamma = angle_deg(v1, v2)
        if gamma < min_angle or (180.0 - gamma) < min_angle:
            continue
        cp = [v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]]
        if gamma < 90.0:
            v2 = [-1.0 * x for x in v2]
            cp = [-1.0 * x for x in cp]
        if abs(90.0 - angle_deg(cp, v3)) < min_angle:
            continue
        if angle_deg(v2, v3) < 90.0:
            v3 = [-1.0 * x for x in v3]
        if (cp[0] * v3[0] + cp[1] * v3[1]) + cp[2] * v3[2] < 0.0:
            v1, v2, v3 = [-1.0 * x for x in v1], [-1.0 * x for x in v2], [-1.0 * x for x in v3]
        axes = np.array(v1 + v2 + v3, F)
        A, ok = inverse(axes)
        if not ok:
            continue
        a = [math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) for w in (v1, v2, v3)]
        c00 = axes[4] * axes[8] - axes[5] * axes[7]
        c01 = axes[5] * axes[6] - axes[3] * axes[8]
        c02 = axes[3] * axes[7] - axes[4] * axes[6]
        vol = abs(float((axes[0] * c00 + axes[1] * c01) + axes[2] * c02))
        if not vol > a[0] * a[1] * a[2] / 100.0:
            continue
        s = np.zeros((), SETTING_DT)
        s["triple"], s["axes"], s["A"] = (i, j, k), axes, A
        out.append(s)
    return np.array(out, SETTING_DT) if out else np.zeros(0, SETTING_DT)
