"""Inputs of the shoebox tests: random geometries, frames of 96 x 80 pixels with the values the counting rule turns on, a mask, and tables
of random and of hand-placed boxes.  Everything follows from a seed; nothing here decides what is right (tests/shoebox_oracle.py does)."""
import numpy as np

import shoebox_oracle as O

W, H = 96, 80
F = np.float64


def random_geometry(rng):
    """A flat panel some 150-300 mm away, tilted by up to a degree, with a beam centre near the image's and an oscillation of 0.1-0.5 deg."""
    px = F(rng.uniform(0.075, 0.172))
    dist, bx, by = F(rng.uniform(150.0, 300.0)), F(W / 2 + rng.uniform(-20, 20)), F(H / 2 + rng.uniform(-20, 20))
    lam = F(rng.uniform(0.7, 1.5))
    D = np.array([[1, 0, -bx * px], [0, -1, by * px], [0, 0, -dist]], F)
    a, b = np.deg2rad(rng.uniform(-1.0, 1.0, 2))
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    axis = np.array([1.0, rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)])
    return O.geometry((Rx @ Ry @ D).reshape(9), [px, px], lam, [0.0, 0.0, -1.0 / lam], axis / np.linalg.norm(axis), rng.uniform(-30.0, 30.0),
                      rng.uniform(0.1, 0.5))


def s1_at(g, x, y):
    """The beam vector through the fractional pixel position (x, y) -- the driver's rule on a general D."""
    D = g["d_matrix"]
    xm, ym = F(x) * g["pixel_size_mm"][0], F(y) * g["pixel_size_mm"][1]
    L = np.array([D[3 * i] * xm + D[3 * i + 1] * ym + D[3 * i + 2] for i in range(3)])
    return L / np.sqrt((L * L).sum()) / g["wavelength"]


def phi_at(g, z):
    return (g["osc_start_deg"] + F(z) * g["osc_width_deg"]) * O.DEG


def pixel_angle(g):
    """Roughly the angle a pixel subtends at the crystal: the unit of delta_b."""
    return float(g["pixel_size_mm"][0] / abs(g["d_matrix"][8]))


def box(g, x, y, z, x_min, x_max, y_min, y_max, z_min, z_max):
    b = np.zeros((), O.BOX_DT)
    b["s1"], b["phi"] = s1_at(g, x, y), phi_at(g, z)
    b["x_min"], b["x_max"], b["y_min"], b["y_max"], b["z_min"], b["z_max"] = x_min, x_max, y_min, y_max, z_min, z_max
    return b


def random_boxes(rng, g, n, n_images):
    """n boxes around random centres in and a little outside the image and the scan, half-widths of 1-6 pixels and 1-2 images; one in
    twenty has its predicted centre 40 pixels away from the box, which leaves it without foreground."""
    out = np.zeros(n, O.BOX_DT)
    for i in range(n):
        x, y, z = rng.uniform(-3, W + 3), rng.uniform(-3, H + 3), rng.uniform(-1, n_images + 1)
        hx, hy, hz = rng.integers(1, 7), rng.integers(1, 7), rng.integers(1, 3)
        ix, iy, iz = int(np.floor(x)), int(np.floor(y)), int(np.floor(z))
        away = 40.0 if rng.random() < 0.05 else 0.0
        out[i] = box(g, x + away, y, z, ix - hx, ix + hx + 1, iy - hy, iy + hy + 1, iz - hz, iz + hz + 1)
    return out


def frames(rng, dtype, n_images):
    """Poisson(3) frames with bright pixels, and scattered over them the values the counting rule and the histogram turn on: 255, 256, 65535
    and, for 32-bit pixels, 2^24 - 1 and 2^24."""
    f = rng.poisson(3.0, (n_images, H, W)).astype(dtype)
    bright = rng.random(f.shape) < 0.02
    f[bright] = rng.integers(100, 4000, int(bright.sum())).astype(dtype)
    special = [255, 256, 65535] + ([(1 << 24) - 1, 1 << 24] if np.dtype(dtype).itemsize == 4 else [])
    for v in special:
        f[rng.random(f.shape) < 0.004] = v
    return f


def mask(rng):
    """Valid-pixel mask: a dead column band, a dead row band and scattered dead pixels."""
    m = np.ones((H, W), np.uint8)
    m[:, 40:43] = 0
    m[55:57, :] = 0
    m[rng.random(m.shape) < 0.01] = 0
    return m
