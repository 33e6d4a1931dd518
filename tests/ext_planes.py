"""Frames built to break the extended algorithm's erosion and final pass, an independent restatement of both, and a census.

A plain helper module (no fixtures, no pytest settings).  Every generator returns (img, mask, note), deterministic from its
arguments; tests/test_ext_planes.py ties the restatement to the oracle and holds every fixture to the census conditions,
tests/test_gpu_ext_planes.py runs the kernels on them.

The idea: uniform noise makes the first-pass plane D ("not background") 1 almost everywhere, because any 7x7 window that holds
noise has an enormous index of dispersion.  A window that holds only zeros has a = 0 > c = 0 false, so D = 0: a flat zero patch
cuts a hole into D three pixels inside its outline (none at all if it is narrower than 7, unless the image edge clips the window),
and the 5x5 erosion widens the hole by two.  Moving the patches moves the edges of D and of the signal region E to any bit, word,
strip or row wanted, while E stays dense enough to overflow the final pass's per-tile list.  `islands` is the complement: a quiet
Poisson background where D is almost empty, and noise patches at the same places.

The numbers below are the kernels' (kernels_extended.hpp, kernels_threshold.hpp, tuning.hpp); a change there moves them here.
"""
import numpy as np

TILE_ROWS = 8            # kTileRows: rows of an exact_tile
LIST_CAP = 2048          # kExactListCap: list entries of a tile before it takes the dense-tile branch
STRIP_WORDS = 62         # word columns a wave of k_ext_erode_strips owns
SEAM = STRIP_WORDS * 32  # 1984: first pixel column of the second strip
PITCH_ALIGN = 128        # pitch_px = W rounded up to this
BIG = 1 << 24            # 32-bit pixels at or above it are no background (compute_sat, standalone.cc:78,90)

NOISE_MAX = {2: 60000, 4: 900000}
# tests on frames wider than 1024 pass this as `threshold` (half the 16-bit noise range): see test_gpu_ext_planes.py
WIDE_THRESHOLD = 30000.0

SHAPES = [
    (np.uint16, 2080, 40),   # two strips; dense tiles in MODE 2 / 3; bands of 16 and 32 rows with a short last one
    (np.uint16, 2000, 33),   # word 62 half beyond the width, word 63 wholly beyond; one row into a new band and a new tile
    (np.uint16, 1985, 17),   # one pixel in the second strip
    (np.uint16, 2048, 24),   # W = pitch_px: the quad path's right-hand fall-back and the bx clamp, at the seam's width class
    (np.uint16, 128, 24),    # the same fall-back, small
    (np.uint16, 125, 24),    # ... and at an odd width
    (np.uint16, 97, 40),     # one strip, narrow
    (np.uint32, 330, 40),    # dense tiles in MODE 1
    (np.uint32, 128, 24),    # right edge
]


def shape_id(s):
    return "%s-%dx%d" % (np.dtype(s[0]).name, s[1], s[2])


def pitch_px(W):
    return (W + PITCH_ALIGN - 1) // PITCH_ALIGN * PITCH_ALIGN


# ---- where things are placed -----------------------------------------------------------------------------------------

SEAM_ZONE = (SEAM - 24, SEAM + 16)   # columns the walking patches leave to the patches placed at the strip seam
# the masked singles beside the seam, (row, column): see _mask.  Rows 0 .. 13 (0 .. 10 where the frame ends before column 1986) are
# theirs; the seam patches start below
SEAM_MASKS = dict(at_1984=(0, SEAM), at_1983=(4, SEAM - 1), at_1981=(8, SEAM - 3), at_1986=(11, SEAM + 2))


def _walk(W, H):
    """Patches every 37 columns (37 is coprime to 32: the left edges walk over every x mod 32 once there are 32 of them), the top
    row stepping by 5; sizes between 7x7 and 11x9.  (x, y, w, h)"""
    out = []
    for i, x in enumerate(range(5, W - 11, 37)):
        w, h = 7 + i % 5, 7 + (i // 5) % 3
        if W > SEAM and x + w > SEAM_ZONE[0] and x < SEAM_ZONE[1]:
            continue
        out.append((x, (5 * i) % max(H - h + 1, 1), w, h))
    return out


def _seam_slots(W, H):
    """Top rows of the patches at the strip seam, which overlap in x and so take turns in y: every 8 rows below the rows of SEAM_MASKS,
    while at least 6 rows are left (a patch that the bottom edge clips still cuts its hole)."""
    return list(range(14 if SEAM + 2 < W else 11, H - 5, 8))


def _seam_patches(W, H):
    """Zero patches at x = 1983 | 1984, 7 rows each, as many as the height has room for (one at H = 17 and 24, two at 33, three at
    40), in this order.  The first two are what the erosion's carried words are for: a wave's lanes 0 and 63 hold the neighbouring
    strips' words, and a hole of D on ONE side of the seam, within two columns of it, erodes E on the other side through them."""
    want = [(SEAM - 3, 7),     # 1981 .. 1987, across the seam: D's hole is column 1984 alone, E's is 1982 .. 1986
            (SEAM - 4, 7),     # 1980 .. 1986, across the seam: D's hole is column 1983 alone, E's is 1981 .. 1985
            (SEAM - 9, 9)]     # ends at 1983: E's hole ends at 1982 and nothing crosses
    return [(x, y, w, 7) for (x, w), y in zip(want, _seam_slots(W, H))]


def _targets(W, H):
    """The patches placed on purpose, as (x, y, w, h), clipped to the frame later.  In the frame's interior a patch [x, x + w) cuts
    the hole [x + 3, x + w - 3) into D and [x + 1, x + w - 1) into E; at an image edge the window is clipped, and the hole reaches
    the edge.  The first four are the corners."""
    t = []
    # corners: 6 x 6 (the clipped windows make D's hole 3 x 3, E's 5 x 5); borders: 4 deep (D's hole is the edge pixels alone)
    t += [(0, 0, 6, 6), (W - 6, 0, 6, 6), (0, H - 6, 6, 6), (W - 6, H - 6, 6, 6)]
    t += [(0, H // 2 - 4, 4, 8), (W - 4, H // 2 - 4, 4, 8), (W // 2 - 24, 0, 9, 4), (W // 2 - 4, H - 4, 9, 4)]
    if SEAM < W <= SEAM + 8:
        # the right edge lies in the second strip's first word: the seam patches and masked singles have it (the patch across the
        # seam is clipped there, so its hole reaches the edge like a border patch's)
        t[1] = t[3] = t[5] = (W, 0, 0, 0)
    # the row seams of the 8-row tiles and the 16- and 32-row bands, rows 7|8, 15|16, 31|32: a hole of D across each (rows s - 2 .. s),
    # and a hole of E that starts at row s
    xs = W // 2 - 30
    for k, s in enumerate((8, 16, 32)):
        if s + 1 <= H:
            t.append((xs + 14 * k, s - 5, 9, 9))
        if s + 6 <= H:
            t.append((xs - 14 - 12 * k, s - 1, 8, 7))
    return t


def _clip(W, H, p):
    x, y, w, h = p
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None


def _mask(W, H, rng, dead_fraction):
    """Masked pixels as singles, pairs, one whole column, one block, and a single at each place the erosion kernels split the plane:
    bit 0 and bit 31 of a word, x = 1983 and 1984 (and 1981 and 1986: SEAM_MASKS), rows 15, 16, 31 and 32 (and 8, and two rows
    below each row seam: under flavour 0 such a pixel's 5x5 hole starts at the seam)."""
    mask = np.ones((H, W), np.uint8)
    n = max(int(W * H * dead_fraction), 4)
    k = rng.choice(W * H, n, replace=False)
    mask.reshape(-1)[k] = 0
    for _ in range(max(n // 8, 2)):                                   # pairs, side by side or one above the other
        y, x = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
        mask[y, x] = 0
        mask[(y + 1, x) if rng.integers(2) else (y, x + 1)] = 0
    mask[:, 2 * W // 3 + 1] = 0                                       # one whole column
    for x, y in ((64, H // 2 - 3), (95, H // 2 + 3), (32, H - 9), (63, 9)):   # bit 0 / bit 31 of a word
        if x < W:
            mask[y, x] = 0
    for j, y in enumerate((15, 16, 31, 32, 8, 10, 18, 34)):
        if y < H:
            mask[y, 12 + 9 * j] = 0
            mask[y, W - 14 - 9 * j] = 0
    # one block: under flavour 1 it erodes nothing, so signal-region pixels beside it see few valid pixels outside the region
    bx, by = W // 2 + 14, 3 * H // 5     # (below the busy middle rows: at 330 x 40 every tile has to stay above the list's capacity)
    mask[by:by + 10, bx:bx + 13] = 0
    if W > SEAM:
        # the strip seam, in rows that the seam patches leave alone; nothing else is masked near them.  Flavour 1: a masked pixel is out
        # of E and erodes nothing, so the one at 1984 makes E 1|0 across the seam and the one at 1983 0|1.  Flavour 0: each erodes its
        # 5x5 -- the one at 1984 reaches 1982 and 1983 only through the word that lane 63 carries (rows 0, 1), the one at 1983 reaches
        # 1984 and 1985 through lane 0's (rows 3 .. 6); the one at 1981 erodes up to 1983, so E is 0|1 (rows 7 .. 10), the one at 1986
        # from 1984, so E is 1|0 (rows 11 .. 13; at W = 1985 there is no such column, and no other way: the last column's clipped 5x5 is a
        # subset of its neighbour's).
        mask[0:15, SEAM - 8:min(SEAM + 8, W)] = 1
        for y, x in SEAM_MASKS.values():
            if x < W and y < H:
                mask[y, x] = 0
    return mask


# ---- the generators --------------------------------------------------------------------------------------------------

def dense(dtype, W, H, seed=0):
    """Noise with flat zero patches: D and E dense, their edges placed.  (img, mask, note)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([seed, W, H, dtype.itemsize, 1])
    img = rng.integers(1, NOISE_MAX[dtype.itemsize] + 1, (H, W)).astype(dtype)
    patches = _walk(W, H) + _targets(W, H) + (_seam_patches(W, H) if W > SEAM else [])
    boxes = [b for b in (_clip(W, H, p) for p in patches) if b]
    for x0, y0, x1, y1 in boxes:
        img[y0:y1, x0:x1] = 0
    if dtype.itemsize == 4:
        # a handful at and above 2^24: three in the noise, three inside zero patches (valid, outside E, and no background)
        ys, xs = rng.integers(0, H, 3), rng.integers(0, W, 3)
        img[ys, xs] = (BIG, BIG + 5, 1 << 30)
        for (x0, y0, x1, y1), v in zip(boxes[1:8:3], (BIG, BIG + 1, (1 << 32) - 1)):
            img[(y0 + y1) // 2, (x0 + x1) // 2] = v
    mask = _mask(W, H, rng, 0.003 if dtype.itemsize == 2 else 0.0008)
    return img, mask, "dense %s %dx%d seed %d: %d zero patches" % (dtype.name, W, H, seed, len(boxes))


def islands(dtype, W, H, seed=0):
    """The sparse complement: Poisson(2) background, where D is almost empty, and 9x9 to 15x15 noise patches at the places `dense`
    targets (every third of its walking patches), so E is a few small islands and most words of its plane are zero.  (img, mask, note)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([seed, W, H, dtype.itemsize, 2])
    img = rng.poisson(2.0, (H, W)).astype(dtype)
    mask = _mask(W, H, rng, 0.003 if dtype.itemsize == 2 else 0.0008)
    boxes = []
    walk, targets = _walk(W, H)[::3], _targets(W, H)
    for i, (x, y, w, h) in enumerate(walk + targets):
        corner = len(walk) <= i < len(walk) + 4
        border = len(walk) + 4 <= i < len(walk) + 8
        s = 9 if corner or border else 9 + 2 * (i % 4)                  # 9, 11, 13, 15
        # the same left / top edge where the patch touches one, else the same centre
        nx = x if x == 0 else W - s if x + w >= W else x + w // 2 - s // 2
        ny = y if y == 0 else H - s if y + h >= H else y + h // 2 - s // 2
        b = _clip(W, H, (nx, ny, s, s))
        if b:
            boxes.append(b)
    for j, (x0, y0, x1, y1) in enumerate(boxes):
        img[y0:y1, x0:x1] = rng.integers(1, NOISE_MAX[dtype.itemsize] + 1, (y1 - y0, x1 - x0)).astype(dtype)
        if j % 2 == 0:                                                 # a masked single inside every second island
            mask[(y0 + y1) // 2, (x0 + x1) // 2] = 0
    if W > SEAM:
        # one island (16 x 16) across the strip seam, tall enough to hold the masked singles of SEAM_MASKS; below it, where the frame has
        # the rows and columns, one noise patch on either side.  D reaches three columns beyond a noise patch: the one that ends at
        # 1981 has D's edge at 1984 | 1985, which erodes 1983 through the word lane 63 carries; the one that starts at 1987 has it at
        # 1983 | 1984, which erodes 1984 and 1985 through lane 0's
        for p in ((SEAM - 8, 0, 16, 16), (SEAM - 11, 24, 9, 7), (SEAM + 3, 32, 9, 7)):
            b = _clip(W, H, p)
            if b and b[3] - b[1] >= 7 and b[2] - b[0] >= 7 or p[1] == 0:
                x0, y0, x1, y1 = b
                img[y0:y1, x0:x1] = rng.integers(1, NOISE_MAX[dtype.itemsize] + 1, (y1 - y0, x1 - x0)).astype(dtype)
    if dtype.itemsize == 4:
        for (x0, y0, x1, y1), v in zip(boxes[:6:2], (BIG, BIG + 5, 1 << 30)):
            img[y0 + 1, x0 + 1] = v
    return img, mask, "islands %s %dx%d seed %d: %d noise patches" % (dtype.name, W, H, seed, len(boxes))


def empty(dtype, W, H):
    """All zeros, nothing masked: D, E and the strong plane are empty.  (img, mask, note)"""
    return np.zeros((H, W), np.dtype(dtype)), np.ones((H, W), np.uint8), "empty %s %dx%d" % (np.dtype(dtype).name, W, H)


_CACHE = {}


def fixture(kind, dtype, W, H, seed=0):
    """The generators' frames, made once per process and read-only."""
    key = (kind, np.dtype(dtype).name, W, H, seed)
    if key not in _CACHE:
        img, mask, note = empty(dtype, W, H) if kind == "empty" else {"dense": dense, "islands": islands}[kind](dtype, W, H, seed)
        img.setflags(write=False)
        mask.setflags(write=False)
        _CACHE[key] = (img, mask, note)
    return _CACHE[key]


# ---- the independent restatement (boolean planes; never calls the oracle) ------------------------------------------------

def erode(D, mask, flavour):
    """The signal region E from the first-pass plane D.  A pixel is in E when it is in D and every pixel of its 5x5 neighbourhood
    either lies outside the image or is in D (flavour 0, baseline.cpp:552-571: Chebyshev distance >= 3 to the nearest pixel that is
    not in D; a masked pixel is not in D, so it erodes) or is masked (flavour 1, erosion.cu:101-105: masked neighbours are skipped)."""
    D = np.asarray(D).astype(bool)
    valid = np.asarray(mask) != 0
    return _erode(D, valid, D | ~valid if flavour == 1 else D)


def _erode(D, valid, passes):
    """D, valid, and every pixel of the 5x5 neighbourhood outside the image or in `passes`."""
    H, W = D.shape
    p = np.pad(passes, 2, constant_values=True)
    keep = D & valid
    for dy in range(5):
        for dx in range(5):
            keep = keep & p[dy:dy + H, dx:dx + W]
    return keep


def _box_sum(a, r):
    """Sums of `a` (int64) over the (2r+1)^2 window clipped to the frame, from an integral image."""
    H, W = a.shape
    ii = np.zeros((H + 1, W + 1), np.int64)
    ii[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]


def background_counts(E, mask, img):
    """(m2, x2), int64: count and sum over the clipped 11x11 window of the second pass's background pixels -- valid, outside E and
    (32-bit pixels) below 2^24 (baseline.cpp:755 with compute_sat's rule)."""
    v = np.asarray(img).astype(np.int64)
    bg = (np.asarray(mask) != 0) & ~np.asarray(E).astype(bool) & (v < BIG)
    return _box_sum(bg.astype(np.int64), 5), _box_sum(np.where(bg, v, 0), 5)


def final(img, m2, x2, E, flavour, nsig_s=3.0, threshold=0.0):
    """The strong plane, float64, operation by operation as baseline.cpp:640-645 (E holds valid pixels only, m2 and x2 are never
    negative: the guard of :636 is E itself); flavour 1 also wants a background pixel in the window (thresholding.cu:472)."""
    src = np.asarray(img).astype(np.float64)
    m, x = m2.astype(np.float64), x2.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(m2 >= 2, x / m, 0.0)
    local = src >= (mean + np.float64(nsig_s) * np.sqrt(mean))
    strong = np.asarray(E).astype(bool) & (src > np.float64(threshold)) & local
    if flavour == 1:
        strong &= m2 > 0
    return strong


# ---- the census ------------------------------------------------------------------------------------------------------

def _edges(P):
    """({x mod 32 where P rises along a row}, {... falls}): P[y, x - 1] != P[y, x], counted at x."""
    P = P.astype(bool)
    xs = np.arange(1, P.shape[1])
    rise, fall = ~P[:, :-1] & P[:, 1:], P[:, :-1] & ~P[:, 1:]
    return set((xs[rise.any(0)] % 32).tolist()), set((xs[fall.any(0)] % 32).tolist())


def census(img, mask, first, eroded, flavour):
    """Counts of what the kernels' branches need, from planes that the oracle and the restatement agree on."""
    D, E = np.asarray(first).astype(bool), np.asarray(eroded).astype(bool)
    H, W = E.shape
    c = {}
    pad = (-W) % 4
    groups = np.pad(E, ((0, 0), (0, pad))).reshape(H, -1, 4).any(2)
    tiles = range(0, H, TILE_ROWS)
    c["tile_rows"] = [min(TILE_ROWS, H - y) for y in tiles]
    c["tile_pixels"] = [int(E[y:y + TILE_ROWS].sum()) for y in tiles]
    c["tile_groups"] = [int(groups[y:y + TILE_ROWS].sum()) for y in tiles]
    c["E_rise"], c["E_fall"] = _edges(E)
    c["D_rise"], c["D_fall"] = _edges(D)
    # whole words of E's plane that are zero in a row that holds a non-zero one
    words = np.pad(E, ((0, 0), (0, (-W) % 32))).reshape(H, -1, 32).any(2)
    c["zero_words_in_live_rows"] = int((~words[words.any(1)]).sum())
    if W > SEAM:
        a, b = E[:, SEAM - 1], E[:, SEAM]
        c["seam_E_rise"], c["seam_E_fall"] = int((~a & b).sum()), int((a & ~b).sum())
        a, b = D[:, SEAM - 1], D[:, SEAM]
        c["seam_D_rise"], c["seam_D_fall"] = int((~a & b).sum()), int((a & ~b).sum())
        c["seam_E_pixels"] = int(E[:, SEAM - 5:SEAM + 5].sum())      # columns 1979 .. 1988
        c["E_at_seam_column"] = int(E[:, SEAM].sum())                # their 5x5 reaches x = 1982, 1983
        # pixels next to the seam that ONLY the other strip's columns erode: what the words carried by lanes 63 and 0 are for
        valid = np.asarray(mask) != 0
        passes = D | ~valid if flavour == 1 else D
        left, right = passes.copy(), passes.copy()
        left[:, SEAM:] = True                                        # (as if nothing from column 1984 on could erode)
        right[:, :SEAM] = True
        c["seam_carry_lane63"] = int((_erode(D, valid, left) & ~E)[:, SEAM - 2:SEAM].sum())
        c["seam_carry_lane0"] = int((_erode(D, valid, right) & ~E)[:, SEAM:SEAM + 2].sum())
    c["E_left"] = int(E[:, :8].sum())
    c["E_right"] = int(E[:, max(pitch_px(W) - 12, 0):].sum())
    c["E_top"], c["E_bottom"] = int(E[:5].sum()), int(E[max(H - 5, 0):].sum())
    m2, _ = background_counts(E, mask, img)
    for k in (0, 1, 2):
        c["m2_%d" % k] = int((E & (m2 == k)).sum())
    c["m2_3plus"] = int((E & (m2 >= 3)).sum())
    c["flavours_differ"] = int((E != erode(D, mask, 1 - flavour)).sum())
    c["rows_E_changes"] = set((1 + np.flatnonzero((E[1:] != E[:-1]).any(1))).tolist())
    return c
