"""Voxel sets built to break the 3D connected components, and the independent graph formulation they are judged by.

A plain helper module (no fixtures, no pytest settings).  Every generator returns (W, H, slices, note): `slices` is a
list of (k uint64 ascending, intensity uint32) in z order, k = y W + x -- what ffs_stack3d_add_slice and O.cc3d take.

Intensities are at least 1 everywhere.  A strong pixel of intensity 0 cannot come out of the dispersion threshold
(it would have to exceed its window's mean), and on such a pixel the oracle and the kernel legitimately disagree
about the peak: the reference's peak search starts from numeric_limits<double>::min(), which 0 never reaches, while
the kernel's packed maximum starts from 0.  Nothing here builds one.

Limits the generators keep: at most 65 536 voxels per fixture, and no straight chain of voxels (a column, a z pillar)
longer than 4096 -- uf_find has no path compression, so long chains cost quadratic time, and these fixtures are about
correctness (DESIGN.md section 3.5 has that cost as a measurement).
"""
import numpy as np

W0, H0 = 64, 48            # the small frame most fixtures live on
ROOT_CHUNK = 512           # kRootChunk (kernels_uf.hpp): list entries per chunk of k_finalize_roots3d


def _helix_components(vol):
    """Independent formulation of the reference's graph INCLUDING its row-wrap edge: strong pixels of each slice
    as a 1D sequence (linear index k = y W + x), edges k -- k+1 (no row-end check, connected_components.cc:62-70),
    k -- k+W, and the same k in the next slice (:352-370); components by scipy's sparse-graph labelling; numbered
    in order of their smallest (z, k) vertex (Boost's DFS discovery order over ascending vertex ids)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    Z, H, W = vol.shape
    flat = vol.reshape(Z, H * W) != 0
    ids = -np.ones((Z, H * W), np.int64)
    n = 0
    for z in range(Z):
        on = np.flatnonzero(flat[z])
        ids[z, on] = np.arange(n, n + len(on))
        n += len(on)
    src, dst = [], []
    for z in range(Z):
        a = ids[z]
        for step in (1, W):                        # k+1 joins (W-1, y) with (0, y+1) too
            both = (a[:-step] >= 0) & (a[step:] >= 0)
            src.append(a[:-step][both]); dst.append(a[step:][both])
        if z + 1 < Z:
            both = (a >= 0) & (ids[z + 1] >= 0)
            src.append(a[both]); dst.append(ids[z + 1][both])
    src, dst = np.concatenate(src), np.concatenate(dst)
    g = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    order = np.argsort(first)                      # label order = order of the smallest vertex
    rank = np.empty_like(order); rank[order] = np.arange(len(order))
    return ids, rank[lab] if n else lab


# ---- between volumes and slice lists ---------------------------------------------------------------------------------

def slices_of(vol):
    """(Z, H, W) array of intensities, 0 = no voxel -> the slice lists."""
    out = []
    for plane in vol:
        flat = plane.reshape(-1)
        k = np.flatnonzero(flat)
        out.append((k.astype(np.uint64), flat[k].astype(np.uint32)))
    return out


def volume_of(W, H, slices):
    """The slice lists as a (Z, H, W) occupancy volume (for _helix_components)."""
    vol = np.zeros((max(len(slices), 1), H * W), np.uint8)
    for z, (k, _) in enumerate(slices):
        vol[z, np.asarray(k, np.int64)] = 1
    return vol.reshape(-1, H, W)


def vertex_arrays(W, slices):
    """x, y, z, intensity of every voxel in vertex order (slice by slice, ascending k)."""
    if not slices or not sum(len(k) for k, _ in slices):
        e = np.zeros(0, np.int64)
        return e, e, e, e
    k = np.concatenate([np.asarray(k, np.int64) for k, _ in slices])
    z = np.concatenate([np.full(len(k), z, np.int64) for z, (k, _) in enumerate(slices)])
    i = np.concatenate([np.asarray(i, np.int64) for _, i in slices])
    return k % W, k // W, z, i


def _ramp(vol):
    """Distinct-ish intensities >= 1 on the voxels of an occupancy volume: peaks and centroids differ per component."""
    Z, H, W = vol.shape
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(H), np.arange(W), indexing="ij")
    return np.where(vol != 0, 1 + (7 * xx + 13 * yy + 29 * zz) % 251, 0).astype(np.uint32)


# ---- topology --------------------------------------------------------------------------------------------------------

def late_join(last_row=False, NZ=12):
    """Two arms from slice 0 through every slice meet only through a bridge in the last slice; a third component has
    its smallest (z, k) vertex between the arms' first voxels.  One joined component labelled 0, the third labelled 1."""
    W, H = W0, H0
    vol = np.zeros((NZ, H, W), np.uint8)
    if last_row:
        ya = yb = 40
        xa, xb = 10, 50
        vol[:, ya, xa] = 1
        vol[:, yb, xb] = 1
        vol[0:2, 40, 30:32] = 1                    # the third: first vertex (z 0, y 40, x 30) lies between the arms'
        vol[NZ - 1, ya:H, xa] = 1                  # down to the last row ...
        vol[NZ - 1, H - 1, xa:xb + 1] = 1          # ... along it ...
        vol[NZ - 1, yb:H, xb] = 1                  # ... and up again
    else:
        ya, xa, yb, xb = 5, 10, 20, 40
        vol[:, ya, xa] = 1
        vol[:, yb, xb] = 1
        vol[0:3, 10, 5:7] = 1                      # the third
        vol[NZ - 1, ya:yb + 1, xa] = 1
        vol[NZ - 1, yb, xa:xb + 1] = 1
    return W, H, slices_of(_ramp(vol)), "late_join" + ("_last_row" if last_row else "")


def z_staircase(NZ=12):
    """Slice z holds x = z and x = z + 1 of one row: consecutive slices share exactly one pixel.  One component, held
    together by z edges and in-row edges alternately."""
    W, H = W0, H0
    vol = np.zeros((NZ, H, W), np.uint8)
    for z in range(NZ):
        vol[z, 7, z:z + 2] = 1
    return W, H, slices_of(_ramp(vol)), "z_staircase"


def z_diagonal(NZ=12):
    """Slice z holds only x = z: NZ components (no diagonal connectivity in z).  Entry i + 1 of the stack holds k + 1
    of entry i every time -- in the NEXT slice, where the k + 1 edge must not reach."""
    W, H = W0, H0
    vol = np.zeros((NZ, H, W), np.uint8)
    for z in range(NZ):
        vol[z, 7, z] = 1
    return W, H, slices_of(_ramp(vol)), "z_diagonal"


def serpentine(NZ=5):
    """A boustrophedon path in plane (full even rows, odd rows one pixel at alternating ends) in the even slices; each
    odd slice holds the single pixel that links its two neighbours (the path's last pixel, then its first, ...)."""
    W, H = 24, 11
    plane = np.zeros((H, W), np.uint8)
    plane[0::2, :] = 1
    for j, y in enumerate(range(1, H, 2)):
        plane[y, W - 1 if j % 2 == 0 else 0] = 1
    vol = np.zeros((NZ, H, W), np.uint8)
    vol[0::2] = plane
    ends = [(H - 1, W - 1 if ((H - 1) // 2) % 2 == 0 else 0), (0, 0)]
    for j, z in enumerate(range(1, NZ, 2)):
        y, x = ends[j % 2]
        vol[z, y, x] = 1
    return W, H, slices_of(_ramp(vol)), "serpentine"


def row_wrap_3d():
    """The k + 1 edge with no row-end check, and where it must stop.
    slice 0: (W-1, 3) -- (0, 4) one component; the same pairs moved to x = W-2 / x = 1 are no edges (three variants).
    slices 1, 2: (W-1, 20) in slice 1 and (0, 21) in slice 2 -- two components; likewise the x = W-2 / x = 1 pairs.
    slices 3, 4: (W-1, H-1) is the last entry of slice 3 and (0, 0) the first entry of slice 4 -- two components.
    slices 4, 5: the last entry of slice 4 is k, the first entry of slice 5 is k + 1 -- two components."""
    W, H = W0, H0
    vol = np.zeros((6, H, W), np.uint8)
    vol[0, 3, W - 1] = vol[0, 4, 0] = 1            # the wrap edge
    vol[0, 10, W - 2] = vol[0, 11, 1] = 1          # k + 3
    vol[0, 14, W - 2] = vol[0, 15, 0] = 1          # k + 2
    vol[0, 18, W - 1] = vol[0, 19, 1] = 1          # k + 2
    vol[1, 20, W - 1] = vol[2, 21, 0] = 1          # k + 1, but in the next slice
    vol[1, 30, W - 2] = vol[2, 31, 1] = 1
    vol[1, 34, W - 2] = vol[2, 35, 0] = 1
    vol[1, 38, W - 1] = vol[2, 39, 1] = 1
    vol[3, 2, 2] = 1
    vol[3, H - 1, W - 1] = 1                       # last entry of slice 3
    vol[4, 0, 0] = 1                               # first entry of slice 4
    vol[4, 30, 20] = 1                             # last entry of slice 4: k
    vol[5, 30, 21] = 1                             # first entry of slice 5: k + 1
    vol[5, 40, 40] = 1
    return W, H, slices_of(_ramp(vol)), "row_wrap_3d"


def _blob_slice():
    vol = np.zeros((1, H0, W0), np.uint8)
    vol[0, 10:13, 20:24] = 1
    vol[0, 30, 5:8] = 1
    return slices_of(_ramp(vol))[0]


_EMPTY = (np.zeros(0, np.uint64), np.zeros(0, np.uint32))


def empty_between():
    """Two identical slices with an empty one between them: nothing joins them (4 components, not 2)."""
    s = _blob_slice()
    return W0, H0, [s, _EMPTY, s], "empty_between"


def empty_first_last():
    """Empty first and last slices: z ranks of the voxels start at 1."""
    s = _blob_slice()
    return W0, H0, [_EMPTY, s, s, _EMPTY], "empty_first_last"


def twin_slices():
    """Two identical slices, to be added under frame ids with a gap (7 and 19): z is a rank, so they are joined."""
    s = _blob_slice()
    return W0, H0, [s, s], "twin_slices"


def only_empty():
    return W0, H0, [_EMPTY, _EMPTY, _EMPTY], "only_empty"


def no_slices():
    return W0, H0, [], "no_slices"


def checker_3d():
    """3D parity checkerboard of 32 x 32 x 4 in the corner of the 64-wide frame (no pixel in the last column, so no
    row-wrap edge): all 2048 voxels are components of their own."""
    W, H = W0, H0
    zz, yy, xx = np.meshgrid(np.arange(4), np.arange(H), np.arange(W), indexing="ij")
    vol = (((xx + yy + zz) % 2 == 0) & (xx < 32) & (yy < 32)).astype(np.uint8)
    return W, H, slices_of(_ramp(vol)), "checker_3d"


def solid():
    """A 48 x 40 x 6 block: one component, every accumulator atomic lands on one root."""
    W, H = W0, H0
    vol = np.zeros((6, H, W), np.uint8)
    vol[:, 4:44, 8:56] = 1
    return W, H, slices_of(_ramp(vol)), "solid"


# k_finalize_roots3d: thread t of chunk c handles the entries i0 = c * 512 + 2 t and i0 + 1.  Around every chunk
# boundary b the fixtures put one of these root (R) / non-root (N) patterns on the entries b-2, b-1 | b, b+1; a
# non-root directly behind a root or non-root is the next pixel of the same horizontal run, so "? N" across the
# bar is a component that spans the boundary.
CHUNK_TOTALS = (511, 512, 513, 1023, 1024, 1025, 1537)
_CHUNK_PATTERNS = {
    511: {},
    512: {},
    513: {512: "RNR"},
    1023: {512: "NNRN"},
    1024: {512: "NNNR"},
    1025: {512: "RNNN", 1024: "NRN"},
    1537: {512: "NRRR", 1024: "RRNN", 1536: "RRR"},
}
_CHUNK_TAILS = {511: "RN", 512: "NR", 513: "R", 1023: "RR", 1024: "NN", 1025: "N", 1537: "R"}


def chunk_edges(total):
    """Isolated voxels, horizontal pairs and short runs whose entry count is exactly `total`, with chosen root /
    non-root patterns on the entries either side of every multiple of kRootChunk and at the end of the list."""
    W, H = W0, H0
    s = list(("RRN" * (total // 3 + 1))[:total])
    for b, pat in _CHUNK_PATTERNS[total].items():
        for j, ch in enumerate(pat):
            if b - 2 + j < total:
                s[b - 2 + j] = ch
    tail = _CHUNK_TAILS[total]
    s[total - len(tail):] = list(tail)
    s[0] = "R"
    runs = []                                      # lengths of the horizontal runs, in list order
    for ch in s:
        if ch == "R":
            runs.append(1)
        else:
            runs[-1] += 1
    # runs in raster order with a gap behind each, on every other row (even rows in even slices, odd rows in odd
    # slices: nothing is adjacent vertically or in z), never in the last column
    planes, plane, y, x, z = [], np.zeros((H, W), np.uint8), 0, 0, 0
    for L in runs:
        if x + L > W - 1:
            x, y = 0, y + 2
        if y >= H:
            planes.append(plane)
            plane, z = np.zeros((H, W), np.uint8), z + 1
            y, x = z % 2, 0
        plane[y, x:x + L] = 1
        x += L + 1
    planes.append(plane)
    vol = np.stack(planes)
    assert int(vol.sum()) == total
    return W, H, slices_of(_ramp(vol)), f"chunk_edges_{total}"


def root_flags(W, H, slices):
    """True where a vertex is the first of its component (what the kernels call a root), by the graph formulation."""
    _, lab = _helix_components(volume_of(W, H, slices))
    if len(lab) == 0:
        return np.zeros(0, bool), lab
    first = np.full(int(lab.max()) + 1, len(lab), np.int64)
    np.minimum.at(first, lab, np.arange(len(lab)))
    flags = np.zeros(len(lab), bool)
    flags[first] = True
    return flags, lab


TOPOLOGY = {
    "late_join": late_join,
    "late_join_last_row": lambda: late_join(last_row=True),
    "z_staircase": z_staircase,
    "z_diagonal": z_diagonal,
    "serpentine": serpentine,
    "row_wrap_3d": row_wrap_3d,
    "empty_between": empty_between,
    "empty_first_last": empty_first_last,
    "twin_slices": twin_slices,
    "only_empty": only_empty,
    "no_slices": no_slices,
    "checker_3d": checker_3d,
    "solid": solid,
    **{f"chunk_edges_{t}": (lambda t=t: chunk_edges(t)) for t in CHUNK_TOTALS},
}


# ---- numerics: each with a hand-known answer (tests/test_cc_shapes.py holds the oracle to it) ------------------------

def _from_voxels(W, H, NZ, voxels):
    vol = np.zeros((NZ, H, W), np.uint32)
    for (z, y, x, v) in voxels:
        assert v >= 1 and vol[z, y, x] == 0
        vol[z, y, x] = v
    return slices_of(vol)


def peak_ties():
    """Equal maxima: the smallest (z, y, x) wins.  Components in label order, with their peaks:
      0: row y = 3 of slice 0, x = 5..8 with 5, 9, 9, 2                               -> peak (x 6, y 3, z 0), 9
      1: pixel (20, 10) in slices 0, 1, 2 with 4, 7, 7                                -> peak (20, 10, z 1), 7
      2: a 2 x 2 x 2 block at x 40, y 30, slices 0 and 1, all 6                       -> peak (40, 30, z 0), 6
      3: (30, 21) = 8 in slice 1; (30, 21) = 1 and (30, 20) = 8 in slice 2: the later slice has the smaller y, but z
         decides first                                                                -> peak (30, 21, z 1), 8"""
    vox = [(0, 3, 5, 5), (0, 3, 6, 9), (0, 3, 7, 9), (0, 3, 8, 2),
           (0, 10, 20, 4), (1, 10, 20, 7), (2, 10, 20, 7),
           (1, 21, 30, 8), (2, 21, 30, 1), (2, 20, 30, 8)]
    vox += [(z, y, x, 6) for z in (0, 1) for y in (30, 31) for x in (40, 41)]
    return W0, H0, _from_voxels(W0, H0, 3, vox), "peak_ties"


PEAK_TIES_EXPECTED = [   # (peak_x, peak_y, peak_z, peak_intensity, num_pixels) in label order
    (6, 3, 0, 9, 4), (20, 10, 1, 7, 3), (40, 30, 0, 6, 8), (30, 21, 1, 8, 3)]


def line5(axis):
    """Five voxels in a line along `axis` ("x", "y" or "z": the same pixel in five slices) with intensities 3, 1, 1, 1, 3.
    The peak is the first voxel (tie rule), the centroid is the middle of the third: exactly 2.0 apart."""
    inten = (3, 1, 1, 1, 3)
    y0, x0 = 9, 17
    if axis == "x":
        vox = [(0, y0, x0 + j, v) for j, v in enumerate(inten)]
    elif axis == "y":
        vox = [(0, y0 + j, x0, v) for j, v in enumerate(inten)]
    else:
        vox = [(j, y0, x0, v) for j, v in enumerate(inten)]
    return W0, H0, _from_voxels(W0, H0, 5 if axis == "z" else 1, vox), f"line5_{axis}"


def small_and_spread():
    """Seven voxels along x with 1000, 1, 1, 1, 1, 1, 1000: the peak is the first, the centroid 3.0 away.  With
    min_spot_size_3d 8 it is too small AND too spread: it counts under size only (size is tested first)."""
    inten = (1000, 1, 1, 1, 1, 1, 1000)
    vox = [(0, 12, 30 + j, v) for j, v in enumerate(inten)]
    return W0, H0, _from_voxels(W0, H0, 1, vox), "small_and_spread"


WIDE_W, WIDE_H, WIDE_ROW = 10240, 16, 5
WIDE_X0, WIDE_N, WIDE_I = 10176, 64, 2 ** 32 - 1


def wide_sums():
    """64 voxels at x = 10176..10239 of one row of a 10240-wide frame, all 2^32 - 1: sum (2x+1) I has 53 bits, so the
    reference's double accumulation is still exact.  com_x = 10208.0, sum_intensity = 64 (2^32 - 1)."""
    k = (WIDE_ROW * WIDE_W + WIDE_X0 + np.arange(WIDE_N)).astype(np.uint64)
    return WIDE_W, WIDE_H, [(k, np.full(WIDE_N, WIDE_I, np.uint32))], "wide_sums"


# ---- delivery: a fixture as frames the dispersion threshold turns back into the same voxel set -----------------------

def render(W, H, slices, bright=1000, quiet=1):
    """One uint16 frame per slice: the voxels at `bright` on a background of `quiet` (one-pixel lines of a bright value
    on a quiet background are strong, and nothing else is)."""
    frames = np.full((len(slices), H * W), quiet, np.uint16)
    for z, (k, _) in enumerate(slices):
        frames[z, np.asarray(k, np.int64)] = bright
    return frames.reshape(len(slices), H, W)
