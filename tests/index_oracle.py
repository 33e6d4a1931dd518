"""The rule of the indexer's basis-vector search (csrc/index_model.hpp) in NumPy float64 and Python floats: every
operation an IEEE float64 + - * / sqrt rounded on its own in the header's order (NumPy fuses nothing), libm through `math` (the C
library's cos, sin, exp, log, acos).  The FFT is vectorised stage by stage in the header's schedule for any power of two; components and
the host steps work for any n."""
import math

import numpy as np

PEAK_DT = np.dtype([("root", "<u4"), ("n_voxels", "<u4"), ("sum", "<i8", (3,)), ("frac", "<f8", (3,))])     # ffs_index_peak
VECTOR_DT = np.dtype([("v", "<f8", (3,)), ("length", "<f8"), ("volume", "<u4"), ("reserved", "<u4")])       # ffs_index_vector
STATS_DT = np.dtype([("sum", "<f8"), ("mean", "<f8"), ("rmsd", "<f8"), ("cutoff", "<f8"), ("n_selected", "<u4"), ("n_peaks", "<u4")])
NOT_USED = 0xFFFFFFFF
RMSD_CUTOFF, PEAK_VOLUME_CUTOFF, MIN_CELL = 15.0, 0.15, 3.0
DEG = math.pi / 180.0


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def norm(v):
    return math.sqrt(dot(v, v))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def normalized(v):
    n = norm(v)
    return [v[0] / n, v[1] / n, v[2] / n]


def c_round(x):
    """C's round(): halves away from zero"""
    return math.floor(x + 0.5) if x >= 0.0 else -math.floor(-x + 0.5)


def c_round_exact(x):
    r = c_round(x)
    # floor(x + 0.5) rounds x + 0.5 first: 0.49999999999999994 + 0.5 == 1.0.  C's round does not.
    if abs(r - x) > 0.5:
        r -= math.copysign(1.0, x)
    return r


def rlp(g, xyz):
    """(rlp, s1, xyz_mm), each (n, 3)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = [np.zeros((len(xyz), 3)) for _ in range(3)]
    D = [float(v) for v in g["d_matrix"]]
    px = [float(v) for v in g["pixel_size_mm"]]
    wl, s0 = float(g["wavelength"]), [float(v) for v in g["s0"]]
    u = normalized([float(v) for v in g["rot_axis"]])
    for i, (xp, yp, z) in enumerate(xyz.tolist()):
        x, y = xp * px[0], yp * px[1]
        L = normalized([(D[3 * k] * x + D[3 * k + 1] * y) + D[3 * k + 2] for k in range(3)])
        s1 = [L[k] / wl for k in range(3)]
        angle = (float(g["osc_start_deg"]) + z * float(g["osc_width_deg"])) * DEG
        S = [s1[k] - s0[k] for k in range(3)]
        c, s, d = math.cos(-1.0 * angle), math.sin(-1.0 * angle), dot(u, S)
        X = cross(u, S)
        out[0][i] = [(S[k] * c + (u[k] * d) * (1.0 - c)) + s * X[k] for k in range(3)]
        out[1][i] = s1
        out[2][i] = [x, y, angle]
    return tuple(out)


def defaults(r, max_cell, n_points, dmin=None):
    r = np.asarray(r, np.float64).reshape(-1, 3)
    if dmin is None or dmin == 0.0:
        dmin = 5.0 * max_cell / float(n_points)
        if len(r):
            d_data = min(1.0 / norm(v) if norm(v) != 0.0 else math.inf for v in r.tolist())
            if d_data > dmin:
                dmin = d_data
    return dmin, (-4.0 * (dmin * dmin)) * math.log(0.05)


def twiddles(n):
    out = np.zeros((n // 2, 2))
    for k in range(n // 2):
        a = math.pi * (float(2 * k) / float(n))
        out[k] = [math.cos(a), -math.sin(a)]
    return out


def map_spots(r, dmin, b_iso, n):
    """per spot (cell, weight); cell NOT_USED where the spot is not mapped"""
    r = np.asarray(r, np.float64).reshape(-1, 3)
    cell, weight = np.full(len(r), NOT_USED, np.uint32), np.zeros(len(r))
    q = 1.0 / (2.0 / (dmin * float(n)))
    for i, v in enumerate(r.tolist()):
        ln = norm(v)
        if ln != 0.0 and 1.0 / ln < dmin:
            continue
        c = [int(c_round_exact(v[j] * q)) + n // 2 for j in range(3)]
        if min(c) < 0 or max(c) >= n:
            continue
        weight[i] = math.exp(((-b_iso * ln) * ln) / 4.0) if b_iso != 0.0 else 1.0
        cell[i] = c[2] + n * c[1] + n * n * c[0]
    return cell, weight


def dedup(cell, weight):
    """cell -> weight of the highest spot number"""
    out = {}
    for i in range(len(cell)):
        if cell[i] != NOT_USED:
            out[int(cell[i])] = float(weight[i])
    return out


def bitrev(n):
    m = n.bit_length() - 1
    return np.array([int(format(p, f"0{m}b")[::-1], 2) for p in range(n)])


def fft_axis(re, im, axis, tw):
    """one pass of the schedule along `axis` of the (N, N, N) arrays; returns new arrays"""
    n = re.shape[axis]
    m = n.bit_length() - 1
    re, im = np.moveaxis(re, axis, 0)[bitrev(n)].copy(), np.moveaxis(im, axis, 0)[bitrev(n)].copy()
    b = np.arange(n // 2)
    for s in range(m):
        half = 1 << s
        j = b & (half - 1)
        i0 = ((b >> s) << (s + 1)) + j
        i1 = i0 + half
        w = j << (m - 1 - s)
        wre, wim = tw[w, 0][:, None, None], tw[w, 1][:, None, None]
        x1re, x1im = re[i1], im[i1]
        tre = wre * x1re - wim * x1im
        tim = wre * x1im + wim * x1re
        are, aim = re[i0], im[i0]
        re[i0], im[i0] = are + tre, aim + tim
        re[i1], im[i1] = are - tre, aim - tim
    return np.ascontiguousarray(np.moveaxis(re, 0, axis)), np.ascontiguousarray(np.moveaxis(im, 0, axis))


def fft3d(cells, n, tw=None):
    """the real part of the transform of the mapped grid, (N, N, N); cells: {cell: weight}"""
    tw = twiddles(n) if tw is None else tw
    re, im = np.zeros(n ** 3), np.zeros((n, n, n))
    for c, w in cells.items():
        re[c] = w
    re = re.reshape(n, n, n)
    for axis in range(3):
        re, im = fft_axis(re, im, axis, tw)
    return re


def power_grid(cells, n, tw=None):
    re = fft3d(cells, n, tw)
    return (re * re).reshape(-1)


def tree(v):
    """the tree sum over the last axis"""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:2 * h]
    return v[..., 0]


def grid_stats(power, n, rmsd_cutoff):
    p = np.asarray(power, np.float64).reshape(n, n, n)
    total = float(tree(tree(tree(p))))
    mean = total / float(n ** 3)
    d = p - mean
    ssq = float(tree(tree(tree(d * d))))
    rmsd = math.sqrt(ssq / float(n ** 3))
    st = np.zeros((), STATS_DT)
    st["sum"], st["mean"], st["rmsd"], st["cutoff"] = total, mean, rmsd, rmsd_cutoff * rmsd
    return st


def components(selected, n):
    """selected: ascending flat indices -> for each its root's flat index (union-find over the +1 neighbours with wrap, root = minimum)"""
    selected = np.asarray(selected, np.int64)
    pos = {int(f): i for i, f in enumerate(selected)}
    parent = list(range(len(selected)))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    c = [selected // (n * n), (selected // n) % n, selected % n]
    step = [n * n, n, 1]
    for j in range(3):
        nb = selected + np.where(c[j] + 1 == n, -(n - 1) * step[j], step[j])
        for i, f in enumerate(nb.tolist()):
            k = pos.get(f)
            if k is not None:
                a, b = find(i), find(k)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return selected[[find(i) for i in range(len(selected))]] if len(selected) else selected


def peaks_of_selection(sel, n):
    """records (ascending root) of the selected flat indices (ascending) on a periodic grid of any n"""
    sel = np.asarray(sel, np.int64)
    root = components(sel, n)
    roots = np.unique(root)
    out = np.zeros(len(roots), PEAK_DT)
    which = np.searchsorted(roots, root)
    out["root"] = roots
    out["n_voxels"] = np.bincount(which, minlength=len(roots))
    for j, (cv, cr) in enumerate(zip((sel // (n * n), (sel // n) % n, sel % n), (root // (n * n), (root // n) % n, root % n))):
        u = cr + ((cv - cr + n // 2) % n) - n // 2
        s = np.zeros(len(roots), np.int64)
        np.add.at(s, which, u)
        out["sum"][:, j] = s
        out["frac"][:, j] = s.astype(np.float64) / (out["n_voxels"].astype(np.float64) * float(n))
    return out


def peaks(power, n, rmsd_cutoff=RMSD_CUTOFF):
    """(records in ascending order of root, statistics)"""
    st = grid_stats(power, n, rmsd_cutoff)
    sel = np.flatnonzero(np.asarray(power, np.float64).reshape(-1) >= float(st["cutoff"]))
    out = peaks_of_selection(sel, n)
    st["n_selected"], st["n_peaks"] = len(sel), len(out)
    return out, st


def filter_peaks(volumes, peak_volume_cutoff=PEAK_VOLUME_CUTOFF):
    """the indices of the peaks that stay (flood_fill_filter)"""
    vol = [int(v) for v in volumes]
    if not vol:
        return []
    s = sorted(vol)
    q3, q1 = s[len(s) * 3 // 4], s[len(s) // 4]
    cut = (q3 - q1) * 5 + q3
    while s[-1] > cut:
        s.pop()
    peak_cutoff = int(peak_volume_cutoff * s[-1])
    return [i for i, v in enumerate(vol) if not v <= peak_cutoff]


def angle_deg(a, b):
    nd = dot(a, b) / (norm(a) * norm(b))
    if abs(nd - 1.0) < 1e-6:
        return 0.0
    if abs(nd + 1.0) < 1e-6:
        return 180.0
    return math.acos(nd) * 180.0 / math.pi


def integer_multiple(v1, v2):
    angle = angle_deg(v1, v2)
    if angle < 5.0 or abs(180.0 - angle) < 5.0:
        l1, l2 = norm(v1), norm(v2)
        if l1 > l2:
            l1, l2 = l2, l1
        k = l2 / l1
        if abs(c_round_exact(k) - k) < 0.2:
            return True
    return False


def basis_vectors(pk, n_points, dmin, max_cell, peak_volume_cutoff=PEAK_VOLUME_CUTOFF, min_cell=MIN_CELL):
    """flood_fill_filter and peaks_to_rlvs on records of PEAK_DT -> records of VECTOR_DT"""
    pk = np.asarray(pk, PEAK_DT)
    keep = filter_peaks(pk["n_voxels"], peak_volume_cutoff)
    fft_cell_length = float(n_points) * dmin / 2.0
    sites = []   # (v, length, volume)
    for i in keep:
        v = []
        for val in pk["frac"][i].tolist():
            if val > 0.5:
                val -= 1.0
            v.append(val * fft_cell_length)
        ln = norm(v)
        if ln > min_cell and ln < 2.0 * max_cell:
            sites.append((v, ln, int(pk["n_voxels"][i])))

    def mean(members):
        o = [0.0, 0.0, 0.0]
        for v, _ in members:
            o = [o[j] + v[j] for j in range(3)]
        return [o[j] / float(len(members)) for j in range(3)]

    groups = []
    for v, ln, vol in sites:
        for members in groups:
            mv = mean(members)
            ml = norm(mv)
            if abs(ml - ln) / max(ml, ln) < 0.1:
                angle = angle_deg(mv, v)
                if angle < 5.0:
                    members.append((v, vol))
                    break
                if abs(180.0 - angle) < 5.0:
                    members.append(([-1.0 * x for x in v], vol))
                    break
        else:
            groups.append([(v, vol)])
    grouped = []
    for members in groups:
        mv = mean(members)
        grouped.append((mv, norm(mv), max(vol for _, vol in members)))
    grouped.sort(key=lambda s: -s[2])   # Python's sort is stable
    grouped.sort(key=lambda s: s[1])
    unique = []
    for s in grouped:
        if not any(u[2] > s[2] and integer_multiple(u[0], s[0]) for u in unique):
            unique.append(s)
    unique.sort(key=lambda s: -s[2])
    out = np.zeros(len(unique), VECTOR_DT)
    for i, (v, ln, vol) in enumerate(unique):
        out[i]["v"], out[i]["length"], out[i]["volume"] = v, ln, vol
    return out


def chain(g, xyz, max_cell, n_points, dmin=None):
    """the whole chain with the reference's constants: a dict of every intermediate"""
    r, s1, mm = rlp(g, xyz)
    dmin, b_iso = defaults(r, max_cell, n_points, dmin)
    cell, weight = map_spots(r, dmin, b_iso, n_points)
    power = power_grid(dedup(cell, weight), n_points)
    pk, st = peaks(power, n_points, RMSD_CUTOFF)
    return dict(rlp=r, s1=s1, xyz_mm=mm, dmin=dmin, b_iso=b_iso, cell=cell, weight=weight, used=cell != NOT_USED, power=power, peaks=pk, stats=st,
                vectors=basis_vectors(pk, n_points, dmin, max_cell))
