"""Summation integration of shoeboxes in Kabsch space (ffs_ctx_shoebox_begin / ffs_stream_shoebox_fold / ffs_ctx_get_shoebox_sums,
include/ffs_hip.h) in NumPy float64, operation by operation as csrc/shoebox_model.hpp states the rule: every + - * / sqrt in the header's
order, on arrays of corners.  The checker, never the thing tested; tests/test_shoebox_oracle.py ties it to a per-pixel, per-corner loop in
Python floats, to the header compiled as a plain C++ program, and to hand-checkable cases.

The background of a box's histogram comes from the two histogram models' own checkers: the Tukey fence from
tests/spot_background_oracle.py (integers; the mean is one float64 division), the robust Poisson GLM from `ffs_hosttool spotbgglm`, the
header every GLM test holds the library to bit for bit (the independent Python GLM of tests/spot_background_glm_oracle.py agrees with it
to rounding only, and the records here are compared as bits)."""
import os
import subprocess

import numpy as np

import spot_background_oracle as T

ELLIPSOID, DIALS = 0, 1
FG_INVALID = 1
N_BINS = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTTOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
BOX_DT = np.dtype([("s1", "<f8", (3,)), ("phi", "<f8"), ("x_min", "<i4"), ("x_max", "<i4"), ("y_min", "<i4"), ("y_max", "<i4"),
                   ("z_min", "<i4"), ("z_max", "<i4")])
SUM_DT = np.dtype([("fg_sum", "<u8"), ("m_x", "<u8"), ("m_y", "<u8"), ("m_z", "<u8"), ("fg_count", "<u4"), ("n_background", "<u4"),
                   ("n_overflow", "<u4"), ("flags", "<u4"), ("bg_status", "<u4"), ("reserved", "<u4"), ("bg_mean", "<f8"),
                   ("intensity", "<f8"), ("variance", "<f8")])
INTEGER_FIELDS = ["fg_sum", "m_x", "m_y", "m_z", "fg_count", "n_background", "n_overflow", "flags", "bg_status"]
FLOAT_FIELDS = ["bg_mean", "intensity", "variance"]
F = np.float64
DEG = F(np.pi) / F(180.0)


def geometry(d_matrix, pixel_size_mm, wavelength, s0, rot_axis, osc_start_deg, osc_width_deg):
    return dict(d_matrix=np.asarray(d_matrix, F).reshape(9), pixel_size_mm=np.asarray(pixel_size_mm, F), wavelength=F(wavelength),
                s0=np.asarray(s0, F), rot_axis=np.asarray(rot_axis, F), osc_start_deg=F(osc_start_deg), osc_width_deg=F(osc_width_deg))


def flat_geometry(distance_mm, beam_x_px, beam_y_px, pixel_x_mm, pixel_y_mm, wavelength, osc_start_deg, osc_width_deg):
    """The driver's flat single panel (host/shoebox_geometry.hpp): fast +x, slow -y, s0 = (0, 0, -1/lambda), axis (1, 0, 0)."""
    bx, by, px, py, lam = F(beam_x_px), F(beam_y_px), F(pixel_x_mm), F(pixel_y_mm), F(wavelength)
    return geometry([1, 0, -bx * px, 0, -1, by * py, 0, 0, -F(distance_mm)], [px, py], lam, [0, 0, F(-1.0) / lam], [1, 0, 0], osc_start_deg, osc_width_deg)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def normalized(v):
    n = np.sqrt(dot(v, v))
    return [v[0] / n, v[1] / n, v[2] / n]


def corner_s(g, cx, cy):
    """s of corners (integer arrays cx, cy), a list of three arrays."""
    x, y = np.asarray(cx).astype(F) * g["pixel_size_mm"][0], np.asarray(cy).astype(F) * g["pixel_size_mm"][1]
    D = g["d_matrix"]
    L = [(D[3 * i] * x + D[3 * i + 1] * y) + D[3 * i + 2] for i in range(3)]
    n = np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
    return [(L[i] / n) / g["wavelength"] for i in range(3)]


def kabsch_frame(g, s1, phi):
    s1 = [F(v) for v in s1]
    e1 = normalized(cross(s1, g["s0"]))
    e2 = normalized(cross(s1, e1))
    return dict(s1=s1, e1=e1, e2=e2, len=np.sqrt(dot(s1, s1)), zeta=dot(g["rot_axis"], e1), phi=F(phi))


def corner_xy(g, fr, cx, cy, ib):
    s = corner_s(g, cx, cy)
    d = [s[i] - fr["s1"][i] for i in range(3)]
    eps1, eps2 = dot(fr["e1"], d) / fr["len"], dot(fr["e2"], d) / fr["len"]
    return (eps1 * eps1 + eps2 * eps2) * ib


def image_terms(g, fr, n, im):
    """(z_low, z_high, z_centre, centre) of image n."""
    phi_low = (g["osc_start_deg"] + F(n) * g["osc_width_deg"]) * DEG
    phi_high = (g["osc_start_deg"] + F(n + 1) * g["osc_width_deg"]) * DEG
    e_low, e_high = fr["zeta"] * (phi_low - fr["phi"]), fr["zeta"] * (phi_high - fr["phi"])
    return (e_low * e_low) * im, (e_high * e_high) * im, (F(0.0) * F(0.0)) * im, bool(fr["phi"] >= phi_low and fr["phi"] <= phi_high)


def corner_foreground(algorithm, xy, terms):
    with np.errstate(invalid="ignore"):
        if algorithm == DIALS:
            return xy <= 1.0
        z_low, z_high, z_centre, centre = terms
        fg = (xy + z_low <= 1.0) | (xy + z_high <= 1.0)
        return fg | (xy + z_centre <= 1.0) if centre else fg


def inverse_square(delta):
    with np.errstate(all="ignore"):
        return F(1.0) / (F(delta) * F(delta))


def foreground_maps(g, box, algorithm, delta_b, delta_m, images):
    """{n: bool array (y_max - y_min, x_max - x_min)}: the foreground decision of every pixel of the box on each image n of `images`."""
    ib, im = inverse_square(delta_b), inverse_square(delta_m)
    fr = kabsch_frame(g, box["s1"], box["phi"])
    cx, cy = np.meshgrid(np.arange(int(box["x_min"]), int(box["x_max"]) + 1), np.arange(int(box["y_min"]), int(box["y_max"]) + 1))
    with np.errstate(all="ignore"):
        xy = corner_xy(g, fr, cx, cy, ib)
        out = {}
        for n in images:
            c = corner_foreground(algorithm, xy, image_terms(g, fr, n, im))
            out[n] = c[:-1, :-1] | c[:-1, 1:] | c[1:, :-1] | c[1:, 1:]
    return out


def new_accumulators(n):
    return dict(fg_sum=[0] * n, m_x=[0] * n, m_y=[0] * n, m_z=[0] * n, fg_count=[0] * n, n_overflow=[0] * n, flags=[0] * n,
                hist=np.zeros((n, N_BINS), np.int64))


def fold(g, boxes, algorithm, delta_b, delta_m, frames, first_image, mask, max_valid, acc, census=None):
    """Folds frames (n, H, W) as images first_image .. into acc (new_accumulators); returns acc.  census (a dict, optional) receives what
    the fixtures are asked to contain: pixel counts "foreground", "background", "overflow", and the sets of boxes whose foreground met a
    pixel that does not count, by cause: "edge", "mask", "max_valid", "ge_2_24"."""
    n_frames, H, W = frames.shape
    wide = frames.dtype.itemsize == 4
    for i, b in enumerate(boxes):
        images = range(max(int(b["z_min"]), first_image), min(int(b["z_max"]), first_image + n_frames))
        if not len(images):
            continue
        x0, x1, y0, y1 = int(b["x_min"]), int(b["x_max"]), int(b["y_min"]), int(b["y_max"])
        px, py = np.meshgrid(np.arange(x0, x1, dtype=np.int64), np.arange(y0, y1, dtype=np.int64))
        in_image = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        cx, cy = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
        masked_out = in_image & (mask[cy, cx] == 0) if mask is not None else np.zeros(px.shape, bool)
        for n, fg in foreground_maps(g, b, algorithm, delta_b, delta_m, images).items():
            p = np.where(in_image, frames[n - first_image][cy, cx].astype(np.int64), 0)
            too_high = in_image & (p > max_valid) if max_valid >= 0 else np.zeros(px.shape, bool)
            too_wide = in_image & (p >= (1 << 24)) if wide else np.zeros(px.shape, bool)
            counts = in_image & ~masked_out & ~too_high & ~too_wide
            take, bad, bg = fg & counts, fg & ~counts, ~fg & counts
            if bad.any():
                acc["flags"][i] |= FG_INVALID
            acc["fg_sum"][i] += int(p[take].sum())
            acc["fg_count"][i] += int(take.sum())
            acc["m_x"][i] += int((p * (2 * px + 1))[take].sum())
            acc["m_y"][i] += int((p * (2 * py + 1))[take].sum())
            acc["m_z"][i] += int(p[take].sum()) * (2 * n + 1)
            bgv = p[bg]
            acc["hist"][i] += np.bincount(bgv[bgv < N_BINS], minlength=N_BINS)
            acc["n_overflow"][i] += int((bgv >= N_BINS).sum())
            if census is not None:
                census["foreground"] = census.get("foreground", 0) + int(take.sum())
                census["background"] = census.get("background", 0) + int(bg.sum())
                census["overflow"] = census.get("overflow", 0) + int((bgv >= N_BINS).sum())
                for name, why in (("edge", ~in_image), ("mask", masked_out), ("max_valid", too_high & ~masked_out), ("ge_2_24", too_wide & ~masked_out)):
                    if (fg & why).any():
                        census.setdefault(name, set()).add(i)
    return acc


def glm_records(hists, tails):
    """(status, mean as float64) per histogram from `ffs_hosttool spotbgglm`."""
    text = "".join(" ".join(str(int(v)) for v in h) + f" {int(t)}\n" for h, t in zip(hists, tails))
    if not text:
        return []
    r = subprocess.run([HOSTTOOL, "spotbgglm"], input=text, capture_output=True, text=True, check=True)
    out = []
    for ln in r.stdout.splitlines():
        t = ln.split()
        out.append((int(t[0]), int(t[4]), np.array([int(t[6], 16)], np.uint64).view(F)[0]))
    assert len(out) == len(tails)
    return out


def sums(acc, background="tukey"):
    """The records of ffs_ctx_get_shoebox_sums (SUM_DT) from accumulators."""
    n = len(acc["fg_sum"])
    out = np.zeros(n, SUM_DT)
    for k in ("fg_sum", "m_x", "m_y", "m_z", "fg_count", "n_overflow", "flags"):
        out[k] = acc[k]
    glm = glm_records(acc["hist"], acc["n_overflow"]) if background == "glm" else None
    for i in range(n):
        if glm is not None:
            n_bg, status, mean = glm[i]
            mean = mean if status == 0 else F(0.0)
        else:
            rec = T.from_histogram(acc["hist"][i], acc["n_overflow"][i])
            n_bg, status = rec[0], rec[7]
            mean = F(rec[6]) / F(rec[5]) if status == T.OK and rec[5] else F(0.0)
        out["n_background"][i], out["bg_status"][i], out["bg_mean"][i] = n_bg, status, mean
        fg_count = int(acc["fg_count"][i])
        if fg_count == 0:
            out["intensity"][i], out["variance"][i] = 0.0, -1.0
            continue
        B = F(mean) * F(fg_count)
        I = F(acc["fg_sum"][i]) - B
        ratio = F(fg_count) / F(n_bg) if n_bg > 0 else F(0.0)
        out["intensity"][i] = I
        out["variance"][i] = abs(I) + abs(B) * (F(1.0) + ratio)
    return out


def summary_counts(records):
    """(boxes, with foreground, FG_INVALID, background failures) as the driver's summary line counts them."""
    fg = records["fg_count"] > 0
    return len(records), int(fg.sum()), int(((records["flags"] & FG_INVALID) != 0).sum()), int((fg & (records["bg_status"] != 0)).sum())


def assert_records_equal(got, want, what=""):
    for k in INTEGER_FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    for k in FLOAT_FIELDS:
        a, b = got[k].view(np.uint64), want[k].view(np.uint64)
        assert np.array_equal(a, b), (what, k, np.flatnonzero(a != b)[:8])
