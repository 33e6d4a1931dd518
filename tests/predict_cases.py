"""Inputs of the prediction tests: a flat-panel geometry, orthogonal cells in orientations that follow from a seed, and the list of cases
the CPU and GPU tests share.  Nothing here decides what is right (tests/predict_oracle.py does)."""
import numpy as np

F = np.float64
W, H = 300, 200


def geometry(pixel_mm=0.5, distance_mm=100.0, beam_px=(141.3, 97.6), wavelength=1.0, osc_start=0.0, osc_width=0.5, axis=(1.0, 0.0, 0.0)):
    """A panel perpendicular to the beam: lab = D (x_mm, y_mm, 1), fast axis +x, slow axis -y, the beam along -z."""
    D = np.array([[1, 0, -beam_px[0] * pixel_mm], [0, -1, beam_px[1] * pixel_mm], [0, 0, -distance_mm]], F)
    return dict(d_matrix=D.reshape(9), pixel_size_mm=np.array([pixel_mm, pixel_mm], F), wavelength=F(wavelength),
                s0=np.array([0.0, 0.0, -1.0 / wavelength], F), rot_axis=np.array(axis, F), osc_start_deg=F(osc_start), osc_width_deg=F(osc_width))


def orientation(seed):
    """A proper rotation from a seed (QR of a normal matrix)."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def a_matrix(cell, seed=None):
    """A = U B for an orthogonal cell (a, b, c) in Angstrom; seed None: aligned with the laboratory axes."""
    B = np.diag([1.0 / cell[0], 1.0 / cell[1], 1.0 / cell[2]])
    U = np.eye(3) if seed is None else orientation(seed)
    return (U @ B).reshape(9).astype(F)


def case(name, g=None, cell=(40.0, 45.0, 50.0), seed=7, n_images=16, dmin=2.0, delta_b=0.01, delta_m=0.004, centring=0, A=None):
    return dict(name=name, g=g if g is not None else geometry(), A=A if A is not None else a_matrix(cell, seed), n_images=n_images, dmin=dmin,
                delta_b=delta_b, delta_m=delta_m, centring=centring, W=W, H=H)


MAIN = case("main")


def cases():
    """The cases the check program and the GPU are held to the oracle on."""
    out = [MAIN]
    # h_max (1, 5, 5): 3 x 11 x 11 = 363 candidates in two workgroups of 256; only the slab h = 0 lies inside the sphere, and it is
    # candidates 121 .. 241: every survivor sits in the first workgroup, the second has none.  A full turn, so that some of them predict
    out.append(case("one-workgroup", g=geometry(osc_width=2.0), cell=(5.0, 63.0, 63.0), dmin=14.0, n_images=180, seed=9))
    out.append(case("nothing", dmin=60.0, n_images=4))                 # no index inside the sphere but (0,0,0)
    # h_max (1, 1, 3): 3 * 3 * 7 = 63 candidates, one wave with one lane to spare (no product of odd numbers is 64); a full turn
    out.append(case("one-wave", g=geometry(osc_width=2.0), cell=(3.0, 3.0, 7.5), dmin=3.5, seed=3, n_images=180))
    out.append(case("one-image", n_images=1))
    out.append(case("full-turn", g=geometry(osc_width=1.0), cell=(20.0, 20.0, 20.0), n_images=360, dmin=2.5, seed=11))
    # 135 x 5 x 5 candidates, fourteen workgroups of 256, and over a full turn some candidate of each of them predicts
    out.append(case("every-seam", g=geometry(osc_width=2.0), cell=(200.0, 5.0, 5.0), seed=1, n_images=180, dmin=3.0))
    for name, code in (("I", 1), ("F", 2), ("A", 3), ("B", 4), ("C", 5), ("R", 6)):
        out.append(case("centring-" + name, centring=code, dmin=3.0, seed=20 + code))
    out.append(case("corner-beam", g=geometry(beam_px=(2.5, 1.5)), dmin=2.5))           # rays leave the panel on two sides ...
    out.append(case("far-corner-beam", g=geometry(beam_px=(297.5, 198.5)), dmin=2.5))   # ... and on the other two
    out.append(case("wide-boxes", delta_b=0.2, delta_m=0.05, dmin=1.8))                # boxes hang over the edge, delta_m / zeta passes both ends
    out.append(case("corner-lost", delta_b=0.9, dmin=4.0, n_images=4))                  # 2 delta_b^2 > 1: b < 0 at every corner
    # +-30 mm of 0.05 mm pixels: boxes above 1024 pixels (the panel is 15 x 10 mm: a third of a turn for a few low-order reflections)
    out.append(case("box-refused", g=geometry(pixel_mm=0.05, osc_width=2.0), delta_b=0.3, dmin=10.0, n_images=60))
    out.append(ZETA_SMALL)
    return out


# ---- the scan launch at its seams ------------------------------------------------------------------------------------------------------
# k_predict_scan is ONE workgroup of 1024 threads over the counts of all the workgroups of 256 candidates: thread t takes the
# per = ceil(n_blocks / 1024) counts from t * per on, cut at n_blocks.  The cases of cases() have at most 14 workgroups: per = 1 and one count
# a thread.  These have 1023, 1024 and 1025 workgroups (the last one: per = 2, thread 512 cut to one count, the threads behind it empty),
# 1435 (per = 2, thread 717 cut, 306 threads empty) and 2065 (per = 3, thread 688 cut to one count).  The candidate count is a product of
# three odd numbers 2 h_max + 1; an orthogonal cell with axes (h_max - 0.5) dmin has h_max = floor(|a_i| / dmin) + 1.
SCAN_THREADS, SCAN_DMIN = 1024, 3.0
#             name              2 h_max + 1     workgroups  per
SCAN_SHAPES = [("scan-1023", (23, 55, 207), 1023, 1),
               ("scan-1024", (21, 57, 219), 1024, 1),
               ("scan-1025", (21, 55, 227), 1025, 2),
               ("scan-1435", (19, 51, 379), 1435, 2),
               ("scan-2065", (19, 73, 381), 2065, 3)]


def scan_cases():
    """A dozen images of 15 degrees, so that hundreds of the workgroups predict."""
    out = []
    for name, odd, n_blocks, per in SCAN_SHAPES:
        cell = tuple(((n - 1) // 2 - 0.5) * SCAN_DMIN for n in odd)
        c = case(name, g=geometry(osc_width=15.0), cell=cell, n_images=12, dmin=SCAN_DMIN)
        c["scan"] = dict(h_max=[(n - 1) // 2 for n in odd], n_blocks=n_blocks, per=per)
        out.append(c)
    return out


def assert_scan_census(c, census):
    """On the oracle's census alone: the case has the workgroup count and the `per` it is named for, its predicting workgroups lie hundreds
    apart, some scan thread with more than one count has records in two of its workgroups, the last thread with counts is cut short where
    the case says so and the threads behind it are empty."""
    want = c["scan"]
    n_cand = census["candidates"]
    assert n_cand == (2 * want["h_max"][0] + 1) * (2 * want["h_max"][1] + 1) * (2 * want["h_max"][2] + 1), (c["name"], n_cand)
    n_blocks = (n_cand + 255) // 256
    per = (n_blocks + SCAN_THREADS - 1) // SCAN_THREADS
    assert (n_blocks, per) == (want["n_blocks"], want["per"]), (c["name"], n_blocks, per)
    blocks = np.unique(census["q"] // 256)
    assert len(blocks) > 300 and blocks[-1] - blocks[0] > 300 and blocks[-1] < n_blocks, (c["name"], len(blocks))
    threads, in_thread = np.unique(blocks // per, return_counts=True)
    if per >= 2:
        assert np.max(in_thread) >= 2, c["name"]
        used = (n_blocks + per - 1) // per
        assert used < SCAN_THREADS and n_blocks - (used - 1) * per < per, (c["name"], "the last thread with counts is cut short, the threads behind it are empty")
    assert np.any(threads >= 1) and census["kept"] > 10000
    return dict(n_blocks=n_blocks, per=per, predicting_blocks=len(blocks), threads_with_two=int(np.sum(in_thread >= 2)), records=census["kept"])


# zeta = axis . e1 vanishes when s1 lies in the plane of s0 and the axis.  A rotation only touches the sphere there (d|s0 + r|^2 / dphi =
# 2 |s1 x s0| zeta), so no narrow image predicts such a ray; ONE IMAGE OF 180 DEGREES does: an aligned cubic cell, the axis along x, the beam
# along -z -- (h, 0, l) with l > 0 starts at (h/a, 0, l/a) and ends at (h/a, ~1e-17, -l/a), the linear step runs inside the x-z plane, and
# when it crosses the sphere s1 has a y component of some 1e-17: e1 = (~1e-16, +-1, 0), zeta ~ 1e-16.
ZETA_SMALL = case("zeta-small", g=geometry(osc_width=180.0), cell=(20.0, 20.0, 20.0), seed=None, n_images=2, dmin=3.0)
