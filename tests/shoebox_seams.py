"""Shoebox tables built to sit where the fold's launch can go wrong without the random tables noticing: foreground edges on the seams between
a wave's strips of 63 pixel columns, on a box's last corner column and its first and last corner row, boxes of the largest allowed size and
boxes in the pad outside the image, corners whose decision is an exact tie (xy, or xy + z, equal to 1.0 bit for bit), and launch lists
shorter than a workgroup.  The image, its frames, mask and geometry helpers are tests/shoebox_cases.py's; tests/shoebox_oracle.py decides
what is right, here as everywhere.  Each builder runs the oracle once and asserts ON THE ORACLE ALONE that its table contains what it was
built for (tests/test_shoebox_seams.py runs the builders without a GPU); everything follows from seeds.

A job is a dict as tests/test_gpu_shoebox.py's `case`: g, dtype, algorithm, max_valid, frames, mask, boxes, delta_b, delta_m, n_images.
The seam, size and tie jobs have at most 4 images; the short lists have 12, for the batches of 1, 3 and 8 frames they are folded in."""
import numpy as np

import shoebox_cases as K
import shoebox_oracle as O

W, H = K.W, K.H
F = np.float64
STRIP = 63          # pixel columns a strip of 64 corner columns covers (kShoeboxStrip of csrc/kernels_shoebox.hpp)
MAX_SIDE = 1024     # kShoeboxMaxSide and kShoeboxPad of csrc/shoebox_plan.hpp
RADIUS = 2.0        # delta_b in pixel angles: the foreground of a box is roughly a disc of this radius around s1
_CACHE = {}


def job(name, seed, dtype, algorithm, n_images, table, max_valid=-1):
    """table: a function (g, rng, job) -> boxes, called once the geometry and the deltas are in the job."""
    rng = np.random.default_rng(seed)
    g = K.random_geometry(rng)
    j = dict(name=name, g=g, dtype=dtype, algorithm=algorithm, max_valid=max_valid, n_images=n_images, frames=K.frames(rng, dtype, n_images), mask=K.mask(rng),
             delta_b=RADIUS * K.pixel_angle(g), delta_m=float(g["osc_width_deg"] * O.DEG))
    j["boxes"] = np.array(table(g, rng, j), O.BOX_DT)
    return j


def oracle_fold(j, images=None):
    images = list(range(j["n_images"]) if images is None else images)
    return O.fold(j["g"], j["boxes"], j["algorithm"], j["delta_b"], j["delta_m"], j["frames"][images[0]:images[-1] + 1], images[0], j["mask"], j["max_valid"],
                  O.new_accumulators(len(j["boxes"])))


def acc_of(j):
    """The oracle's accumulators over all the job's images, computed once."""
    if "acc" not in j:
        j["acc"] = oracle_fold(j)
    return j["acc"]


def corner_maps(j, b, images):
    """{n: bool array (y_max - y_min + 1, x_max - x_min + 1)}: the oracle's decision of every corner of the box on image n."""
    g = j["g"]
    ib, im = O.inverse_square(j["delta_b"]), O.inverse_square(j["delta_m"])
    fr = O.kabsch_frame(g, b["s1"], b["phi"])
    cx, cy = np.meshgrid(np.arange(int(b["x_min"]), int(b["x_max"]) + 1), np.arange(int(b["y_min"]), int(b["y_max"]) + 1))
    with np.errstate(all="ignore"):
        xy = O.corner_xy(g, fr, cx, cy, ib)
        return {n: O.corner_foreground(j["algorithm"], xy, O.image_terms(g, fr, n, im)) for n in images}


def maps_of(j, b):
    """(pixel maps, corner maps) of a box over the job's images inside its z-range; the pixel maps are foreground_maps', and the corner
    maps are asserted to give them."""
    images = range(max(int(b["z_min"]), 0), min(int(b["z_max"]), j["n_images"]))
    fg = O.foreground_maps(j["g"], b, j["algorithm"], j["delta_b"], j["delta_m"], images)
    c = corner_maps(j, b, images)
    for n in images:
        assert np.array_equal(fg[n], c[n][:-1, :-1] | c[n][:-1, 1:] | c[n][1:, :-1] | c[n][1:, 1:])
    return fg, c


# ---- seams ---------------------------------------------------------------------------------------------------------------------------------
# (x_min, k): the seam is corner column x_min + 63 k -- lane 63 of strip k - 1 and lane 0 of strip k; pixel column seam - 1 is lane 62 of the
# one strip, pixel column seam lane 0 of the next
SEAMS = {"first": (5, 1), "second": (-40, 2), "left-overhang": (-60, 1), "right-edge": (W - 1 - STRIP, 1)}
SEAM_OFFSETS = [-3.3 + 0.5 * i for i in range(14)]   # s1's x against the seam: the disc's edges and its two extreme columns cross it
SEAM_ROWS = (30, 37)


def seam_group(g, name):
    x_min, k = SEAMS[name]
    seam = x_min + STRIP * k
    y0, y1 = SEAM_ROWS
    return [K.box(g, seam + d, y0 + 3.4, 1.5, x_min, seam + 7, y0, y1, 0, 4) for d in SEAM_OFFSETS]


def assert_seam_group(j, name, boxes):
    """Some pixel of column seam - 1 is foreground while column seam is not in the same row; some pixel the reverse; and some foreground pixel
    has its only foreground corner on corner column seam."""
    x_min, k = SEAMS[name]
    at = STRIP * k   # the seam's column inside the box
    left_only = right_only = single = False
    for b in boxes:
        assert int(b["x_min"]) == x_min and int(b["x_max"]) > x_min + at + 1
        fg, corners = maps_of(j, b)
        for n in fg:
            p, c = fg[n], corners[n]
            left_only |= bool(np.any(p[:, at - 1] & ~p[:, at]))
            right_only |= bool(np.any(~p[:, at - 1] & p[:, at]))
            for col in (at - 1, at):        # the two pixel columns that touch corner column `at`
                others = c[:-1, col if col == at - 1 else col + 1] | c[1:, col if col == at - 1 else col + 1]
                on_seam = c[:-1, at].astype(int) + c[1:, at].astype(int)
                single |= bool(np.any((on_seam == 1) & ~others))
    assert left_only and right_only and single, (name, left_only, right_only, single)
    assert 0 <= x_min + at - 1 and x_min + at < W, "both pixel columns of the seam lie in the image"


# widths at which the last corner column is lane 63 of a strip, lane 0 of the next, and the same after two strips; all end at x_max = 90
WIDTHS = (63, 64, 126, 127)
LAST_COLUMN_X_MAX = 90


def last_column_group(g, width):
    x_max = LAST_COLUMN_X_MAX
    return [K.box(g, x_max + d, 12.4, 1.5, x_max - width, x_max, 10, 16, 0, 4) for d in (1.2, 1.7, 1.95)]


def assert_last_column_group(j, width, boxes):
    """Some pixel of the last pixel column is foreground with foreground corners in column x_max only."""
    found = False
    for b in boxes:
        assert int(b["x_max"]) - int(b["x_min"]) == width
        fg, corners = maps_of(j, b)
        for n in fg:
            c = corners[n]
            found |= bool(np.any(fg[n][:, -1] & ~(c[:-1, -2] | c[1:, -2])))
    assert found, width


def edge_row_group(g):
    """70 x 6 (two strips, s1 next to the seam) and 5 x 6: the disc dips into the box from above and from below, so that only the rolling
    pair's first corner row (y_min) and only its last (y_max) carry foreground."""
    out = []
    for x0, x1 in ((20, 90), (60, 65)):
        x = 82.6 if x1 - x0 > STRIP else 62.4
        for d in (1.2, 1.7, 1.95):
            out.append(K.box(g, x, 20 - d, 1.5, x0, x1, 20, 26, 0, 4))
            out.append(K.box(g, x, 26 + d, 1.5, x0, x1, 20, 26, 0, 4))
    return out


def assert_edge_row_group(j, boxes):
    top = bottom = False
    for b in boxes:
        fg, corners = maps_of(j, b)
        for n in fg:
            c = corners[n]
            top |= bool(np.any(fg[n][0, :] & ~(c[1, :-1] | c[1, 1:])))
            bottom |= bool(np.any(fg[n][-1, :] & ~(c[-2, :-1] | c[-2, 1:])))
    assert top and bottom, (top, bottom)


def one_pixel_group(g):
    """1 x 1, 1 x 64 and 64 x 1 (wide x high), s1 off one corner of each."""
    return [K.box(g, 50 - 1.3, 30 - 1.1, 1.5, 50, 51, 30, 31, 0, 4), K.box(g, 50 - 1.7, 8.4, 1.5, 50, 51, 8, 72, 0, 4), K.box(g, 20.4, 30 - 1.7, 1.5, 20, 84, 30, 31, 0, 4)]


def assert_one_pixel_group(j, boxes):
    assert [(int(b["x_max"] - b["x_min"]), int(b["y_max"] - b["y_min"])) for b in boxes] == [(1, 1), (1, 64), (64, 1)]
    for b in boxes:
        _, corners = maps_of(j, b)
        split = [int(c[0, 0]) + int(c[0, -1]) + int(c[-1, 0]) + int(c[-1, -1]) for c in corners.values()]
        assert any(0 < s < 4 for s in split), split


def seam_table(g, rng, j):
    parts = {}
    for name in SEAMS:
        parts["seam-" + name] = seam_group(g, name)
    for w in WIDTHS:
        parts[f"width-{w}"] = last_column_group(g, w)
    parts["edge-rows"] = edge_row_group(g)
    parts["one-pixel"] = one_pixel_group(g)
    j["groups"], out = {}, []
    for name, boxes in parts.items():
        j["groups"][name] = range(len(out), len(out) + len(boxes))
        out += boxes
    return out


SEAM_COMBOS = [(np.uint16, O.ELLIPSOID), (np.uint16, O.DIALS), (np.uint32, O.ELLIPSOID), (np.uint32, O.DIALS)]


def combo_id(dtype, algorithm):
    return f"{np.dtype(dtype).name}-{'dials' if algorithm == O.DIALS else 'ellipsoid'}"


def seam_job(dtype, algorithm):
    key = "seams-" + combo_id(dtype, algorithm)
    if key not in _CACHE:
        j = job(key, 6300 + 2 * np.dtype(dtype).itemsize + algorithm, dtype, algorithm, 4, seam_table, max_valid=60000 if np.dtype(dtype).itemsize == 2 else -1)
        group = lambda name: j["boxes"][list(j["groups"][name])]
        for name in SEAMS:
            assert_seam_group(j, name, group("seam-" + name))
        for w in WIDTHS:
            assert_last_column_group(j, w, group(f"width-{w}"))
        assert_edge_row_group(j, group("edge-rows"))
        assert_one_pixel_group(j, group("one-pixel"))
        _CACHE[key] = j
    return _CACHE[key]


# ---- the largest boxes ---------------------------------------------------------------------------------------------------------------------
def largest_table(g, rng, j):
    m = MAX_SIDE
    out = [
        K.box(g, 66.3, 31.4, 1.5, -500, -500 + m, 30, 33, 0, 3),     # 1024 x 3, 17 strips, seams at image columns 4 and 67: s1 at the one ...
        K.box(g, 4.4, 31.4, 1.5, -500, -500 + m, 30, 33, 0, 3),      # ... and at the other
        K.box(g, 51.3, 33.7, 1.5, 50, 53, -500, -500 + m, 0, 3),     # 3 x 1024
        # wholly in the pad, as far out as a box may lie (x_max = -1023, and x_min = W + 1023), the full 1024 columns wide; s1 inside them
        K.box(g, -1025.5, 31.5, 1.5, -1023 - m, -1023, 30, 33, 0, 3),
        K.box(g, W + 1025.5, 31.5, 1.5, W + 1023, W + 1023 + m, 30, 33, 0, 3),
        K.box(g, 40.5, -1025.5, 1.5, 39, 42, -1023 - m, -1023, 0, 3),
        K.box(g, 40.5, H + 1025.5, 1.5, 39, 42, H + 1023, H + 1023 + m, 0, 3),
        # from x_min = -1023 over 1024 columns: the last one is the image's column 0, background there, the foreground far outside
        K.box(g, -1000.5, 31.5, 1.5, -1023, 1, 30, 33, 0, 3),
        K.box(g, W + 1000.5, 31.5, 1.5, W - 1, W - 1 + m, 30, 33, 0, 3),
    ]
    j["in_image"], j["in_pad"], j["one_column"] = [0, 1, 2], [3, 4, 5, 6], [7, 8]
    return out


def largest_job(dtype, algorithm):
    key = "largest-" + combo_id(dtype, algorithm)
    if key not in _CACHE:
        j = job(key, 10240 + 2 * np.dtype(dtype).itemsize + algorithm, dtype, algorithm, 3, largest_table)
        acc, b = acc_of(j), j["boxes"]
        assert [int(v) for v in b["x_max"][:2] - b["x_min"][:2]] == [MAX_SIDE] * 2 and int(b["y_max"][2] - b["y_min"][2]) == MAX_SIDE
        assert (-500 + 8 * STRIP, -500 + 9 * STRIP) == (4, 67)
        for i in j["in_image"]:
            assert acc["fg_count"][i] > 0 and acc["hist"][i].sum() > 0, i
        for i in j["in_pad"]:
            assert (acc["flags"][i], acc["fg_count"][i], acc["fg_sum"][i], acc["n_overflow"][i], int(acc["hist"][i].sum())) == (O.FG_INVALID, 0, 0, 0, 0), i
        for i in j["one_column"]:
            assert acc["flags"][i] == O.FG_INVALID and acc["fg_count"][i] == 0 and acc["hist"][i].sum() + acc["n_overflow"][i] > 0, i
        _CACHE[key] = j
    return _CACHE[key]


def square_job(dtype, algorithm):
    """1024 x 1024 around the image, over 2 images."""
    key = "square-" + combo_id(dtype, algorithm)
    if key not in _CACHE:
        j = job(key, 20480 + algorithm, dtype, algorithm, 2, lambda g, rng, j: [K.box(g, 47.3, 41.6, 1.0, -500, -500 + MAX_SIDE, -470, -470 + MAX_SIDE, 0, 2)])
        acc = acc_of(j)
        assert acc["fg_count"][0] > 0 and acc["hist"][0].sum() + acc["n_overflow"][0] + acc["fg_count"][0] <= 2 * W * H and acc["hist"][0].sum() > W * H
        _CACHE[key] = j
    return _CACHE[key]


def refused_boxes(g):
    """(box, the word of the refusal): one column and one row more than a box may have."""
    return [(K.box(g, 40.0, 31.0, 1.5, -500, -500 + MAX_SIDE + 1, 30, 33, 0, 3), "wider"), (K.box(g, 51.0, 33.0, 1.5, 50, 53, -500, -500 + MAX_SIDE + 1, 0, 3), "higher")]


# ---- ties ------------------------------------------------------------------------------------------------------------------------------------
# A corner's decision is `value <= 1.0` with value = xy (DIALS, and the ellipsoid on an image whose edge phi lies on: z = 0) or xy + z_low or
# xy + z_high (ELLIPSOID).  The search moves s1 of a box by units in the last place until the oracle's value at a chosen corner is 1.0 bit
# for bit: s1[0] over a range of steps and, for each, s1[2] to the step that brings the value next to 1.0 -- near the beam centre a unit
# in the last place of s1[2] moves the value by a few of its own, so one in a few of those lands on it.
TIE_IMAGE = 2    # the image whose decision the tie is on (ELLIPSOID)


def tie_value(j, s1, phi, cx, cy, which):
    g = j["g"]
    fr = O.kabsch_frame(g, s1, phi)
    xy = O.corner_xy(g, fr, np.int64(cx), np.int64(cy), O.inverse_square(j["delta_b"]))
    if which == "xy":
        return xy
    z_low, z_high, _, centre = O.image_terms(g, fr, TIE_IMAGE, O.inverse_square(j["delta_m"]))
    assert not centre or which == "edge"
    return xy + {"low": z_low, "high": z_high, "edge": z_low}[which]


def _steps(x, n):
    """x moved by n units in the last place (n: an integer or an array of them)."""
    return x + np.asarray(n, F) * np.spacing(abs(x))


def tie_search(j, s1, phi, cx, cy, which, span=1500):
    """(below, on, above): three s1 that differ in s1[2] alone, with the oracle's value at corner (cx, cy) below 1.0, equal to 1.0 and above
    it; None when the range holds no exact 1.0."""
    value = lambda a, c: tie_value(j, [a, F(s1[1]), c], phi, cx, cy, which)
    a0, c0 = F(s1[0]), F(s1[2])
    for _ in range(40):   # s1[2] as a real number first: the secant brings the value to 1.0 within 1e-13
        v = value(a0, c0)
        if abs(v - 1.0) < 1e-13:
            break
        h = 4096 * np.spacing(abs(c0))
        c0 = c0 - (v - 1.0) * h / (value(a0, c0 + h) - v)
    else:
        return None
    slope = (value(a0, _steps(c0, 64)) - value(a0, _steps(c0, -64))) / 128.0   # of the value per unit in the last place of s1[2]
    if not np.isfinite(slope) or slope == 0.0:
        return None
    a = _steps(a0, np.arange(-span, span + 1))
    n = np.rint((1.0 - value(a, np.full(a.shape, c0))) / slope)
    for extra in (0, -1, 1, -2, 2):
        c = _steps(c0, n + extra)
        hit = np.flatnonzero(value(a, c) == 1.0)
        if len(hit):
            a_on, c_on = a[hit[0]], c[hit[0]]
            lower = upper = c_on
            for _ in range(16):
                lower = np.nextafter(lower, F(-np.inf) if slope > 0 else F(np.inf))
                if value(a_on, lower) < 1.0:
                    break
            for _ in range(16):
                upper = np.nextafter(upper, F(np.inf) if slope > 0 else F(-np.inf))
                if value(a_on, upper) > 1.0:
                    break
            if value(a_on, lower) < 1.0 < value(a_on, upper):
                return tuple(np.array([a_on, s1[1], c], F) for c in (lower, c_on, upper))
    return None


def beam_centre(g):
    """The pixel position where the panel's normal through the crystal meets it, to a pixel or so: where s1[2] moves xy least."""
    D, px = g["d_matrix"], g["pixel_size_mm"]
    return float(-D[2] / px[0]), float(D[5] / px[1])


def tie_table(g, rng, j):
    """At least 12 ties, each as three boxes (below, on, above), each kept only when the oracle shows the box on the tie and the one above
    it differing in a pixel's foreground on TIE_IMAGE.  The first three kinds are asked for by name: a tie on corner column x_min + 63, one
    on corner column x_max, and (ELLIPSOID) one with phi bitwise on the image's phi_low, where xy + 0 <= 1 decides."""
    ellipsoid = j["algorithm"] == O.ELLIPSOID
    bx, by = beam_centre(g)
    out, ties = [], []
    wanted = ["seam", "x_max"] + (["edge"] if ellipsoid else [])
    attempts = 0
    while len(ties) < 14 or wanted:
        attempts += 1
        assert attempts < 400, (len(ties), wanted)
        kind = wanted[0] if wanted else "free"
        cx, cy = int(round(bx)) + int(rng.integers(-12, 13)), int(round(by)) + int(rng.integers(-12, 13))
        quadrant = int(rng.integers(0, 4))
        which = "xy"
        z = 1.5
        if ellipsoid:
            which = "edge" if kind == "edge" else ("low", "high")[len(ties) % 2]
            z = {"edge": float(TIE_IMAGE), "low": TIE_IMAGE - rng.uniform(0.2, 0.5), "high": TIE_IMAGE + 1 + rng.uniform(0.2, 0.5)}[which]
        if kind == "seam":     # the corner is lane 63 of the first strip and lane 0 of the second
            x0, x1 = cx - STRIP, cx + 5
        elif kind == "x_max":  # the corner is on the last corner column: s1 to its right, so that it decides the last pixel column
            x0, x1, quadrant = cx - 9, cx, 0
        else:
            x0, x1 = cx - 4, cx + 5
        theta = quadrant * np.pi / 2 + rng.uniform(-0.2, 0.2)
        phi = K.phi_at(g, z)
        # s1 at the distance from the corner (some RADIUS pixels, less where z takes its share) that brings the value to 1.0 within 1e-9
        at = lambda r: K.s1_at(g, cx + r * np.cos(theta), cy + r * np.sin(theta))
        r = RADIUS
        for _ in range(30):
            v = float(tie_value(j, at(r), phi, cx, cy, which))
            if abs(v - 1.0) < 1e-9:
                break
            r -= (v - 1.0) * 1e-4 / (float(tie_value(j, at(r + 1e-4), phi, cx, cy, which)) - v)
        else:
            continue
        found = tie_search(j, at(r), phi, cx, cy, which)
        if found is None:
            continue
        three = []
        for s1 in found:
            b = K.box(g, 0.0, 0.0, 0.0, x0, x1, cy - 4, cy + 5, 0, 4)
            b["s1"], b["phi"] = s1, phi
            three.append(b)
        maps = [O.foreground_maps(g, b, j["algorithm"], j["delta_b"], j["delta_m"], [TIE_IMAGE])[TIE_IMAGE] for b in three]
        if np.array_equal(maps[1], maps[2]):
            continue   # the tied corner decides no pixel
        ties.append(dict(kind=kind, which=which, corner=(cx, cy), first=len(out)))
        out += three
        if wanted:
            wanted.pop(0)
    j["ties"] = ties
    return out


def tie_job(algorithm):
    key = "ties-" + ("dials" if algorithm == O.DIALS else "ellipsoid")
    if key not in _CACHE:
        j = job(key, 7100 + algorithm, np.uint16 if algorithm == O.DIALS else np.uint32, algorithm, 4, tie_table)
        g, boxes = j["g"], j["boxes"]
        assert len(j["ties"]) >= 12 and len(boxes) == 3 * len(j["ties"])
        kinds = [t["kind"] for t in j["ties"]]
        assert "seam" in kinds and "x_max" in kinds and (algorithm == O.DIALS or "edge" in kinds)
        for t in j["ties"]:
            cx, cy = t["corner"]
            below, on, above = (boxes[t["first"] + i] for i in range(3))
            values = [float(tie_value(j, b["s1"], b["phi"], cx, cy, t["which"])) for b in (below, on, above)]
            assert values[0] < 1.0 and values[1] == 1.0 and values[2] > 1.0, (t, values)
            assert abs(values[0] - 1.0) < 1e-14 and abs(values[2] - 1.0) < 1e-14, (t, values)
            fg = [O.foreground_maps(g, b, algorithm, j["delta_b"], j["delta_m"], [TIE_IMAGE])[TIE_IMAGE] for b in (on, above)]
            assert not np.array_equal(fg[0], fg[1]), t
            _, corners = maps_of(j, on)
            assert corners[TIE_IMAGE][cy - int(on["y_min"]), cx - int(on["x_min"])], "the tied corner is foreground: <= 1.0"
            if t["kind"] == "seam":
                assert cx == int(on["x_min"]) + STRIP and int(on["x_max"]) > cx
            if t["kind"] == "x_max":
                assert cx == int(on["x_max"])
            if t["kind"] == "edge":
                fr = O.kabsch_frame(g, on["s1"], on["phi"])
                z_low, _, _, centre = O.image_terms(g, fr, TIE_IMAGE, O.inverse_square(j["delta_m"]))
                phi_low = (g["osc_start_deg"] + F(TIE_IMAGE) * g["osc_width_deg"]) * O.DEG
                assert F(on["phi"]).tobytes() == F(phi_low).tobytes() and z_low == 0.0 and centre
        if algorithm == O.ELLIPSOID:
            whiches = [t["which"] for t in j["ties"]]
            assert whiches.count("low") >= 4 and whiches.count("high") >= 4
        _CACHE[key] = j
    return _CACHE[key]


# ---- short lists -----------------------------------------------------------------------------------------------------------------------------
SHORT_IMAGES = 12
SHORT_BATCHES = [(0, 1), (1, 4), (4, 12)]   # batches of 1, 3 and 8 frames


def list_lengths(boxes, batches=SHORT_BATCHES):
    return [int(np.sum((boxes["z_min"] < b) & (boxes["z_max"] > a))) for a, b in batches]


def short_job(n, dtype, algorithm):
    """n boxes that every image meets: each fold's launch list has n entries, in ceil(n / 4) workgroups of four waves."""
    key = f"short-{n}-" + combo_id(dtype, algorithm)
    if key not in _CACHE:
        def table(g, rng, j):
            # (centres inside the image, so that every box has foreground)
            return [K.box(g, 10.3 + 17.1 * i, 14.6 + 11.3 * i, 2.0 + 2.0 * i, 10 + 17 * i - 4, 10 + 17 * i + 6, 14 + 11 * i - 5, 14 + 11 * i + 5, 0, SHORT_IMAGES) for i in range(n)]
        j = job(key, 8800 + n, dtype, algorithm, SHORT_IMAGES, table)
        assert list_lengths(j["boxes"]) == [n] * 3 and all(c > 0 for c in acc_of(j)["fg_count"])
        _CACHE[key] = j
    return _CACHE[key]


def short_145_job(dtype, algorithm):
    """Five boxes whose z-ranges give the three folds lists of 1, 4 and 5."""
    key = "short-145-" + combo_id(dtype, algorithm)
    if key not in _CACHE:
        def table(g, rng, j):
            ranges = [(0, 12), (1, 12), (2, 6), (3, 5), (4, 9)]
            return [K.box(g, 12.3 + 16.1 * i, 20.6 + 9.3 * i, (a + b) / 2 + 0.1, int(12 + 16 * i) - 5, int(12 + 16 * i) + 5, int(20 + 9 * i) - 4, int(20 + 9 * i) + 6, a, b)
                    for i, (a, b) in enumerate(ranges)]
        j = job(key, 8900, dtype, algorithm, SHORT_IMAGES, table)
        assert list_lengths(j["boxes"]) == [1, 4, 5] and all(c > 0 for c in acc_of(j)["fg_count"])
        _CACHE[key] = j
    return _CACHE[key]


SHORT_COMBOS = {1: (np.uint16, O.ELLIPSOID), 2: (np.uint32, O.DIALS), 3: (np.uint16, O.DIALS), 5: (np.uint32, O.ELLIPSOID)}


def short_jobs():
    return [short_job(n, *SHORT_COMBOS[n]) for n in (1, 2, 3, 5)] + [short_145_job(np.uint16, O.ELLIPSOID)]


# ---- every job -------------------------------------------------------------------------------------------------------------------------------
LARGEST_COMBOS = [(np.uint16, O.ELLIPSOID), (np.uint32, O.DIALS)]
SQUARE_COMBO = (np.uint16, O.ELLIPSOID)


def seam_and_tie_jobs():
    return [seam_job(d, a) for d, a in SEAM_COMBOS] + [tie_job(O.DIALS), tie_job(O.ELLIPSOID)]


def all_jobs():
    return seam_and_tie_jobs() + [largest_job(d, a) for d, a in LARGEST_COMBOS] + [square_job(*SQUARE_COMBO)] + short_jobs()
