"""Inputs of the indexing tests: a flat-panel geometry, synthetic lattices whose spots are generated through the INVERSE of that geometry
(which rotation angle puts a lattice point on the Ewald sphere, and where its ray meets the panel), and the list of cases the CPU and GPU
tests share.  Nothing here decides what is right (tests/index_oracle.py does)."""
import numpy as np

F = np.float64
PANEL = (2463, 2527)   # pixels


def geometry(pixel_mm=0.172, distance_mm=150.0, beam_px=(1231.4, 1263.7), wavelength=1.0, osc_start=0.0, osc_width=0.25, axis=(1.0, 0.0, 0.0)):
    """A panel perpendicular to the beam: lab = D (x_mm, y_mm, 1), fast axis +x, slow axis -y, the beam along -z."""
    D = np.array([[1, 0, -beam_px[0] * pixel_mm], [0, -1, beam_px[1] * pixel_mm], [0, 0, -distance_mm]], F)
    return dict(d_matrix=D.reshape(9), pixel_size_mm=np.array([pixel_mm, pixel_mm], F), wavelength=F(wavelength),
                s0=np.array([0.0, 0.0, -1.0 / wavelength], F), rot_axis=np.array(axis, F), osc_start_deg=F(osc_start), osc_width_deg=F(osc_width))


def orientation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def real_axes(cell, seed):
    """The rows are the real-space axes a, b, c (Angstrom) of the cell (a, b, c, alpha, beta, gamma) in the orientation of the seed."""
    a, b, c, al, be, ga = cell
    al, be, ga = np.radians([al, be, ga])
    cx = np.cos(be)
    cy = (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    rows = np.array([[a, 0, 0], [b * np.cos(ga), b * np.sin(ga), 0], [c * cx, c * cy, c * np.sqrt(1 - cx * cx - cy * cy)]], F)
    return rows @ orientation(seed).T


def lattice_spots(g, axes, n_images, dmin, panel=PANEL):
    """(x_px, y_px, z) of every lattice point within 1/dmin that crosses the Ewald sphere inside the scan and meets the panel"""
    A = np.linalg.inv(axes)   # r = A h
    hmax = [int(np.linalg.norm(axes[i]) / dmin) + 1 for i in range(3)]
    h = np.stack(np.meshgrid(*[np.arange(-m, m + 1) for m in hmax], indexing="ij"), -1).reshape(-1, 3)
    h = h[np.any(h != 0, axis=1)]
    r0 = h @ A.T
    r0 = r0[np.einsum("ij,ij->i", r0, r0) <= 1.0 / dmin ** 2]
    u = np.asarray(g["rot_axis"], F) / np.linalg.norm(g["rot_axis"])
    s0 = np.asarray(g["s0"], F)
    ur, su = r0 @ u, s0 @ u
    a = r0 @ s0 - su * ur
    b = np.cross(u, r0) @ s0
    c = -0.5 * np.einsum("ij,ij->i", r0, r0) - su * ur
    rad = np.hypot(a, b)
    ok = np.abs(c) <= rad
    out = []
    Dinv = np.linalg.inv(np.asarray(g["d_matrix"], F).reshape(3, 3))
    for sign in (1.0, -1.0):
        phi = np.degrees(np.arctan2(b[ok], a[ok]) + sign * np.arccos(c[ok] / rad[ok]))
        z = np.mod(phi - float(g["osc_start_deg"]), 360.0) / float(g["osc_width_deg"])
        p = np.radians(float(g["osc_start_deg"]) + z * float(g["osc_width_deg"]))
        r = r0[ok]
        rot = r * np.cos(p)[:, None] + np.outer((r @ u) * (1 - np.cos(p)), u) + np.cross(u, r) * np.sin(p)[:, None]
        v = (rot + s0) @ Dinv.T
        x, y = v[:, 0] / v[:, 2] / float(g["pixel_size_mm"][0]), v[:, 1] / v[:, 2] / float(g["pixel_size_mm"][1])
        keep = (v[:, 2] > 0) & (z < n_images) & (x >= 0) & (x < panel[0]) & (y >= 0) & (y < panel[1])
        out.append(np.stack([x, y, z], 1)[keep])
    return np.concatenate(out)


def disturbed(xyz, n_images, seed, missing=0.2, extra=0.05, noise_px=0.3, noise_z=0.1, panel=PANEL):
    """20 % of the spots missing, 5 % random extra spots, centroid noise"""
    rng = np.random.default_rng(seed)
    xyz = xyz[rng.random(len(xyz)) >= missing]
    xyz = xyz + rng.normal(size=xyz.shape) * [noise_px, noise_px, noise_z]
    more = rng.random((int(extra * len(xyz)), 3)) * [panel[0], panel[1], n_images]
    return np.ascontiguousarray(np.concatenate([xyz, more]))


def random_spots(n, n_images, seed, panel=PANEL, spread=None):
    """n spots anywhere on the panel, or within `spread` pixels of its middle (low resolution)"""
    r = np.random.default_rng(seed).random((n, 3))
    if spread is None:
        return r * [panel[0], panel[1], n_images]
    return np.stack([panel[0] / 2 + (2 * r[:, 0] - 1) * spread, panel[1] / 2 + (2 * r[:, 1] - 1) * spread, r[:, 2] * n_images], 1)


def spot_for(g, v):
    """(x_px, y_px, 0) of the spot whose reciprocal-lattice point is v at rotation angle 0 (v must lie on the Ewald sphere; osc_start 0)"""
    s1 = np.asarray(v, F) + np.asarray(g["s0"], F)
    w = np.linalg.inv(np.asarray(g["d_matrix"], F).reshape(3, 3)) @ s1
    return [w[0] / w[2] / float(g["pixel_size_mm"][0]), w[1] / w[2] / float(g["pixel_size_mm"][1]), 0.0]


def on_sphere(g, t):
    """the point of length t on the Ewald sphere in the x-z plane: t (sqrt(1 - ez^2), 0, ez), ez = t wavelength / 2"""
    ez = t * float(g["wavelength"]) / 2.0
    return np.array([t * np.sqrt(1 - ez * ez), 0.0, t * ez])


TRICLINIC = (23.0, 31.0, 37.0, 82.0, 97.0, 105.0)
ORTHOGONAL = (25.0, 33.0, 41.0, 90.0, 90.0, 90.0)
SMALL = (7.5, 9.0, 11.0, 85.0, 100.0, 95.0)   # with max_cell 12 the default dmin keeps spots on the grid at n_points 16 and 32 too
N_IMAGES = 360   # 90 degrees of 0.25


def case(name, xyz, max_cell=45.0, dmin=None, g=None, axes=None):
    return dict(name=name, g=g if g is not None else geometry(), xyz=np.ascontiguousarray(np.asarray(xyz, F).reshape(-1, 3)), max_cell=max_cell, dmin=dmin, axes=axes)


_CACHE = {}


def cases():
    """The cases the check program, the host tool and the GPU are held to the oracle on (built once)."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    g = geometry()
    out = []
    for name, cell, seed in (("triclinic", TRICLINIC, 5), ("orthogonal", ORTHOGONAL, 8)):
        axes = real_axes(cell, seed)
        xyz = lattice_spots(g, axes, N_IMAGES, 2.2)
        out.append(case(name, xyz, axes=axes))
        out.append(case(name + "-disturbed", disturbed(xyz, N_IMAGES, seed + 100), axes=axes))
    axes = real_axes(SMALL, 12)
    out.append(case("small-disturbed", disturbed(lattice_spots(g, axes, N_IMAGES, 1.2), N_IMAGES, 112), max_cell=12.0, axes=axes))
    out.append(case("random", random_spots(300, N_IMAGES, 3)))
    # spots that meet in one cell: the same centre four times with a little noise (their weights differ: the highest spot number's stays), among others
    base = random_spots(40, N_IMAGES, 4, spread=300)
    meet = np.concatenate([base, base[:10] + 0.01, base[:10] - 0.02, base[5:10] + 0.015])
    out.append(case("meet", meet, dmin=2.5))
    # an explicit dmin of 4: spots beyond it are not used; and one spot whose first coordinate maps to n_points (at 16 .. 64)
    far = random_spots(60, N_IMAGES, 6, spread=600)
    edge = spot_for(g, on_sphere(g, 0.999 / 4.0))
    out.append(case("beyond-dmin-and-edge", np.concatenate([far, [edge]]), dmin=4.0))
    out.append(case("no-spots", np.zeros((0, 3))))
    out.append(case("one-spot", [[700.2, 1500.9, 17.3]]))
    _CACHE["cases"] = out
    return out


# ---- power grids built to break the peak search (ffs_ctx_index_load_grid): 1.0 where a voxel is to be selected -----------------------------
def empty(n):
    return np.zeros((n, n, n))


def faces(n):
    g = empty(n)
    for j in range(3):
        for k, run in enumerate(((n - 3, n - 2, n - 1, 0), (n - 1, 0, 1, 2))):   # the bulk on the high side, then on the low side
            at = [3 + 4 * j + 2 * k, 5 + 2 * j + k, 7 + j + 5 * k]
            for c in run:
                at[j] = c
                g[tuple(at)] = 1.0
    return g


def corners(n):
    g = empty(n)
    for c0 in (n - 1, 0):
        for c1 in (n - 1, 0):
            for c2 in (n - 1, 0):
                g[c0, c1, c2] = 1.0
    g[n // 2, n // 2, n // 2] = 1.0
    return g


def through_the_wrap(n):
    g = empty(n)
    g[4, 4, 0:3] = 1.0
    g[4, 4, n - 2:n] = 1.0      # meets the piece above only across the x seam
    g[0:2, 9, 9] = 1.0
    g[n - 3:n, 9, 9] = 1.0      # ... and these two across the slowest axis
    g[7, 0, 2] = g[7, n - 1, 2] = 1.0
    g[7, 5, 2] = 1.0            # one that stays alone
    return g


def snake(n):
    """rows c1 = 0, 2, .. of the planes c0 = 0, 2, .., joined at alternating ends; the planes joined by one voxel"""
    g = empty(n)
    for c0 in range(0, n, 2):
        for c1 in range(0, n - 1, 2):
            g[c0, c1, 1:n - 1] = 1.0
            if c1 + 2 < n - 1:
                g[c0, c1 + 1, n - 2 if (c1 // 2) % 2 == 0 else 1] = 1.0
        if c0 + 2 < n:
            g[c0 + 1, 0, 1] = 1.0
    return g


def seams(n):
    g = empty(n)
    g[:, 3, 5] = 1.0                       # through every plane: every workgroup of the selection
    g[2:2 + n // 2, 6:6 + n // 2, 7] = 1.0   # a slab across planes ...
    g[4, 6:6 + n // 2, 2:2 + n // 2 + 3] = 1.0   # ... and one inside a plane that crosses it: more than 256 list entries at 32
    g[1, 3, 5:8] = 1.0                     # from the bar ...
    g[1:3, 3, 7] = 1.0
    g[2, 3:7, 7] = 1.0                     # ... to the slab
    return g


def diagonals(n):
    g = empty(n)
    for i in range(n):
        g[i, i, i] = 1.0
        g[i, (i + 1) % n, (i + 2) % n] = 1.0
    return g


def reach(n):
    """from the root (2, n/2 + 1, 3): n/2 - 1 up along each axis in turn, and n/2 down along axis 1 and 2 (the root is the smallest flat index, so
    nothing lies below it along axis 0)"""
    g = empty(n)
    h = n // 2
    g[2:2 + h, h + 1, 3] = 1.0              # axis 0: + (n/2 - 1)
    g[3, h + 1:h + 1 + h, 3] = 1.0          # axis 1: + (n/2 - 1), with wrap
    g[3, 1:h + 2, 3] = 1.0                  # axis 1: - n/2
    g[3, h + 1, 3:3 + h] = 1.0              # axis 2: + (n/2 - 1)
    g[4, h + 1, 3 - 3:4] = 1.0
    g[4, h + 1, n - (h - 3):n] = 1.0        # axis 2: - n/2 through the wrap
    return g


SHAPES = dict(faces=faces, corners=corners, through_the_wrap=through_the_wrap, snake=snake, seams=seams, diagonals=diagonals, reach=reach)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)
