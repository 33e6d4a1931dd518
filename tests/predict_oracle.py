"""The rule of scan prediction (csrc/predict_model.hpp) in NumPy float64, in the header's operation order: every + - * / sqrt floor ceil is
one NumPy operation on float64 arrays, so each is rounded on its own as the header's are.  The scan-point settings are an INPUT (the
library hands its own out through ffs_predict_scan_settings): no trigonometric function is evaluated in predict().  rodrigues_settings()
is NumPy's own statement of those matrices, for the test that bounds the difference."""
import numpy as np

DEG = np.pi / 180.0
ENTERING, CORNER_LOST, ZETA_SMALL, BOX_REFUSED = 1, 2, 4, 8
CENTRINGS = {"P": 0, "I": 1, "F": 2, "A": 3, "B": 4, "C": 5, "R": 6}
ZETA_TOLERANCE = 1e-10
LEAVE_MARGIN = 1.000001
MAX_SIDE = PAD = 1024
PREDICTION_DT = np.dtype([("s1", "<f8", (3,)), ("phi", "<f8"), ("x_min", "<i4"), ("x_max", "<i4"), ("y_min", "<i4"), ("y_max", "<i4"),
                          ("z_min", "<i4"), ("z_max", "<i4"), ("x_px", "<f8"), ("y_px", "<f8"), ("z", "<f8"), ("h", "<i4"), ("k", "<i4"),
                          ("l", "<i4"), ("flags", "<u4")])
assert PREDICTION_DT.itemsize == 96


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def normalized(v):
    n = np.sqrt(dot(v, v))
    return [v[0] / n, v[1] / n, v[2] / n]


def inverse(m):
    """By cofactors, in the header's order; m: 9 floats row-major."""
    m = [np.float64(v) for v in np.asarray(m, np.float64).reshape(-1)]
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    det = (m[0] * c00 + m[1] * c01) + m[2] * c02
    with np.errstate(all="ignore"):
        return np.array([c00 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                         c01 / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                         c02 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det], np.float64)


def h_max(a_matrix, dmin):
    real = inverse(a_matrix).reshape(3, 3)
    return [int(np.floor(np.sqrt(dot(real[i], real[i])) / np.float64(dmin))) + 1 for i in range(3)]


def absent(centring, h, k, l):
    """Integers only; arrays or scalars."""
    if centring == 1:
        return (h + k + l) % 2 != 0
    if centring == 2:
        return ((h - k) % 2 != 0) | ((k - l) % 2 != 0)
    if centring == 3:
        return (k + l) % 2 != 0
    if centring == 4:
        return (h + l) % 2 != 0
    if centring == 5:
        return (h + k) % 2 != 0
    if centring == 6:
        return (-h + k + l) % 3 != 0
    return np.zeros(np.shape(h), bool) if np.ndim(h) else False


def candidate_number(hm, h, k, l):
    return ((h + hm[0]) * (2 * hm[1] + 1) + (k + hm[1])) * (2 * hm[2] + 1) + (l + hm[2])


def candidate_index(hm, q):
    nk, nl = 2 * hm[1] + 1, 2 * hm[2] + 1
    hk, l = q // nl, q % nl
    return hk // nk - hm[0], hk % nk - hm[1], l - hm[2]


def rodrigues_settings(g, a_matrix, n_images):
    """NumPy's own A_k = R(phi_k) A, k = 0 .. n_images: R = I cos + K sin + (1 - cos) u u^T as matrices."""
    u = np.asarray(g["rot_axis"], np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]], np.float64)
    A = np.asarray(a_matrix, np.float64).reshape(3, 3)
    out = np.zeros((n_images + 1, 9))
    for k in range(n_images + 1):
        phi = (np.float64(g["osc_start_deg"]) + np.float64(k) * np.float64(g["osc_width_deg"])) * DEG
        R = np.eye(3) * np.cos(phi) + K * np.sin(phi) + (1.0 - np.cos(phi)) * np.outer(u, u)
        out[k] = (R @ A).reshape(-1)
    return out


def _r(A, h, k, l):
    return [(A[3 * i] * h + A[3 * i + 1] * k) + A[3 * i + 2] * l for i in range(3)]


def _to_pixels(d_inv, px, s):
    v0 = (d_inv[0] * s[0] + d_inv[1] * s[1]) + d_inv[2] * s[2]
    v1 = (d_inv[3] * s[0] + d_inv[4] * s[1]) + d_inv[5] * s[2]
    v2 = (d_inv[6] * s[0] + d_inv[7] * s[1]) + d_inv[8] * s[2]
    return v2 > 0.0, (v0 / v2) / px[0], (v1 / v2) / px[1]


def _root(a, b, d):
    q = np.sqrt(d)
    first, second = (-b - q) / a, (-b + q) / a
    ok1, ok2 = (0.0 <= first) & (first <= 1.0), (0.0 <= second) & (second <= 1.0)
    return ok1 | ok2, np.where(ok1, first, second)


def _to_int(v):
    return np.clip(v, -1073741824.0, 1073741824.0).astype(np.int32)


def predict(g, a_matrix, n_images, dmin, delta_b, delta_m, W, H, centring, settings, census=None):
    """The records (PREDICTION_DT) in the order of candidate number, then image.  settings: (n_images + 1, 9) scan-point settings.
    census (a dict, optional) receives what the walk met: candidates, walked, crossings, negative_d, rootless, kept."""
    f = np.float64
    settings = np.asarray(settings, np.float64).reshape(n_images + 1, 9)
    s0 = [f(v) for v in g["s0"]]
    axis = [f(v) for v in g["rot_axis"]]
    px = [f(v) for v in g["pixel_size_mm"]]
    start, width = f(g["osc_start_deg"]), f(g["osc_width_deg"])
    delta_b, delta_m, dmin = f(delta_b), f(delta_m), f(dmin)
    d_inv = inverse(g["d_matrix"])
    hm = h_max(a_matrix, dmin)
    s0s0 = dot(s0, s0)
    limit = f(1.0) / (dmin * dmin)
    leave = limit * f(LEAVE_MARGIN)
    n_cand = (2 * hm[0] + 1) * (2 * hm[1] + 1) * (2 * hm[2] + 1)
    q = np.arange(n_cand, dtype=np.int64)
    h, k, l = candidate_index(hm, q)
    live = ~((h == 0) & (k == 0) & (l == 0)) & ~absent(centring, h, k, l)
    q, h, k, l = q[live], h[live], k[live], l[live]
    hd, kd, ld = h.astype(np.float64), k.astype(np.float64), l.astype(np.float64)
    r1 = _r(settings[0], hd, kd, ld)
    rr1 = dot(r1, r1)
    stay = ~(rr1 > leave)
    q, h, k, l, hd, kd, ld, rr1 = q[stay], h[stay], k[stay], l[stay], hd[stay], kd[stay], ld[stay], rr1[stay]
    r1 = [c[stay] for c in r1]

    def outside(r):
        t = [s0[i] + r[i] for i in range(3)]
        return dot(t, t) >= s0s0
    out1 = outside(r1)
    tally = dict(candidates=n_cand, walked=len(q), crossings=0, negative_d=0, rootless=0, kept=0)
    parts = []
    with np.errstate(all="ignore"):
        for n in range(n_images):
            r2 = _r(settings[n + 1], hd, kd, ld)
            rr2 = dot(r2, r2)
            out2 = outside(r2)
            sel = np.nonzero((out1 != out2) & ~(rr1 > limit))[0]
            if len(sel):
                tally["crossings"] += len(sel)
                a1, a2 = [c[sel] for c in r1], [c[sel] for c in r2]
                dr = [a2[i] - a1[i] for i in range(3)]
                t1 = [s0[i] + a1[i] for i in range(3)]
                t2 = [s0[i] + a2[i] for i in range(3)]
                a = dot(dr, dr)
                b = dot(t1, dr)
                c = rr1[sel] + 2.0 * dot(s0, a1)
                d = b * b - a * c
                ok_d1 = ~(d < 0.0)
                ok_r1, alpha1 = _root(a, b, d)
                b = -dot(t2, dr)
                c = rr2[sel] + 2.0 * dot(s0, a2)
                d = b * b - a * c
                ok_d2 = ~(d < 0.0)
                ok_r2, alpha2 = _root(a, b, d)
                tally["negative_d"] += int(np.sum(~ok_d1 | (ok_d1 & ok_r1 & ~ok_d2)))
                tally["rootless"] += int(np.sum((ok_d1 & ~ok_r1) | (ok_d1 & ok_r1 & ok_d2 & ~ok_r2)))
                alpha = alpha1 / (alpha1 + alpha2)
                s1 = [(a1[i] + alpha * dr[i]) + s0[i] for i in range(3)]
                angle = (start + f(n) * width) + alpha * width
                phi = angle * DEG
                front, x_px, y_px = _to_pixels(d_inv, px, s1)
                keep = ok_d1 & ok_r1 & ok_d2 & ok_r2 & front & (0.0 <= x_px) & (x_px < f(W)) & (0.0 <= y_px) & (y_px < f(H))
                if np.any(keep):
                    parts.append(_records(keep, sel, q, h, k, l, n, s1, phi, alpha, x_px, y_px, out1, s0, axis, d_inv, px, start, width, delta_b,
                                          delta_m, n_images, W, H))
            r1, rr1, out1 = r2, rr2, out2
    rec = np.concatenate(parts) if parts else np.zeros(0, np.dtype(PREDICTION_DT.descr + [("q", "<i8"), ("n", "<i8")]))
    rec = rec[np.lexsort((rec["n"], rec["q"]))]
    tally["kept"] = len(rec)
    if census is not None:
        census.update(tally)
        census["q"], census["n"] = rec["q"].copy(), rec["n"].copy()
    out = np.zeros(len(rec), PREDICTION_DT)
    for name in PREDICTION_DT.names:
        out[name] = rec[name]
    return out


def _records(keep, sel, q, h, k, l, n, s1, phi, alpha, x_px, y_px, out1, s0, axis, d_inv, px, start, width, delta_b, delta_m, n_images, W, H):
    f = np.float64
    idx = sel[keep]
    s1 = [c[keep] for c in s1]
    phi, alpha, x_px, y_px = phi[keep], alpha[keep], x_px[keep], y_px[keep]
    m = len(idx)
    rec = np.zeros(m, np.dtype(PREDICTION_DT.descr + [("q", "<i8"), ("n", "<i8")]))
    rec["q"], rec["n"] = q[idx], n
    rec["h"], rec["k"], rec["l"] = h[idx], k[idx], l[idx]
    for i in range(3):
        rec["s1"][:, i] = s1[i]
    rec["phi"], rec["x_px"], rec["y_px"], rec["z"] = phi, x_px, y_px, f(n) + alpha
    flags = np.where(out1[idx], ENTERING, 0).astype(np.uint32)
    e1 = normalized(cross(s1, s0))
    e2 = normalized(cross(s1, e1))
    length = np.sqrt(dot(s1, s1))
    x_lo, x_hi, y_lo, y_hi = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    survived = np.zeros(m, np.int64)
    for ci in range(4):
        sa, sb = (f(-1.0) if ci & 2 else f(1.0)), (f(-1.0) if ci & 1 else f(1.0))
        fa, fb = sa * delta_b, sb * delta_b
        p = [(fa * e1[i]) * length + (fb * e2[i]) * length for i in range(3)]
        b = length * length - dot(p, p)
        lost = b < 0.0
        d = -(dot(p, s1) / length) + np.sqrt(b)
        sp = [(d * s1[i]) / length + p[i] for i in range(3)]
        front, x, y = _to_pixels(d_inv, px, sp)
        lost = lost | ~front | ~np.isfinite(x) | ~np.isfinite(y)
        flags = flags | np.where(lost, CORNER_LOST, 0).astype(np.uint32)
        first, later = ~lost & (survived == 0), ~lost & (survived > 0)
        x_lo = np.where(first | (later & (x < x_lo)), x, x_lo)
        x_hi = np.where(first | (later & (x > x_hi)), x, x_hi)
        y_lo = np.where(first | (later & (y < y_lo)), y, y_lo)
        y_hi = np.where(first | (later & (y > y_hi)), y, y_hi)
        survived = survived + (~lost).astype(np.int64)
    rec["x_min"], rec["x_max"] = _to_int(np.floor(x_lo)), _to_int(np.ceil(x_hi))
    rec["y_min"], rec["y_max"] = _to_int(np.floor(y_lo)), _to_int(np.ceil(y_hi))
    zeta = dot(axis, e1)
    normal = (zeta > ZETA_TOLERANCE) | (zeta < -ZETA_TOLERANCE)
    phi_plus, phi_minus = phi + delta_m / zeta, phi - delta_m / zeta
    z_plus, z_minus = ((phi_plus * 180.0 / np.pi) - start) / width, ((phi_minus * 180.0 / np.pi) - start) / width
    lo = np.floor(np.where(z_plus < z_minus, z_plus, z_minus))
    hi = np.ceil(np.where(z_plus > z_minus, z_plus, z_minus))
    lo = np.where(normal, np.clip(lo, 0.0, f(n_images) - 1.0), 0.0)
    hi = np.where(normal, np.clip(hi, 1.0, f(n_images)), f(n_images))
    lo, hi = np.nan_to_num(lo), np.nan_to_num(hi)   # (only where normal is false and the division gave no number)
    rec["z_min"], rec["z_max"] = lo.astype(np.int32), hi.astype(np.int32)
    flags = flags | np.where(~normal, ZETA_SMALL, 0).astype(np.uint32)
    refused = (survived == 0) | box_refused(rec, W, H)
    rec["flags"] = flags | np.where(refused, BOX_REFUSED, 0).astype(np.uint32)
    return rec


def box_refused(rec, W, H):
    x0, x1, y0, y1 = (rec[n].astype(np.int64) for n in ("x_min", "x_max", "y_min", "y_max"))
    empty = ~(x0 < x1) | ~(y0 < y1) | ~(rec["z_min"] < rec["z_max"])
    return empty | (x1 - x0 > MAX_SIDE) | (y1 - y0 > MAX_SIDE) | (x1 <= -PAD) | (x0 >= W + PAD) | (y1 <= -PAD) | (y0 >= H + PAD)
