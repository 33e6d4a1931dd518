"""Inputs of the index-assignment tests: lattices from tests/index_cases.py under settings from their own basis vectors, duplicate groups placed
by hand, the corners of the arithmetic and the shapes.  Nothing here decides what is right (tests/assign_oracle.py does); `expected` runs
the oracle once per case and keeps the result, which nobody changes."""
import math

import numpy as np

import assign_oracle as AO
import index_cases as K
import index_oracle as IO

F = np.float64
_CACHE = {}


def case(name, rlp, phi, A, tolerance=0.3, selected=None, **more):
    rlp = np.ascontiguousarray(np.asarray(rlp, F).reshape(-1, 3))
    return dict(name=name, rlp=rlp, phi=np.ascontiguousarray(np.asarray(phi, F).reshape(-1)), A=np.ascontiguousarray(np.asarray(A, F).reshape(-1, 9)),
                tolerance=tolerance, selected=None if selected is None else np.asarray(selected, bool), **more)


def lattice(name, n_settings=None):
    """A case of index_cases: its rlp and phi, the settings from its own vectors at 64 points (all, or the first n_settings), then the true
    setting, the cell doubled and the cell halved"""
    key = ("lattice", name, n_settings)
    if key not in _CACHE:
        c = K.by_name(name)
        o = IO.chain(c["g"], c["xyz"], c["max_cell"], 64, c["dmin"])
        s = AO.settings(o["vectors"]["v"])
        if n_settings is not None:
            s = s[:n_settings]
        true_A, ok = AO.inverse(c["axes"].reshape(9))
        assert ok
        A = np.concatenate([s["A"].reshape(-1, 9), [true_A, true_A * F(0.5), true_A * F(2.0)]])
        _CACHE[key] = case(name, o["rlp"], o["xyz_mm"][:, 2], A, vectors=o["vectors"], settings=s, axes=c["axes"], n_own=len(s))
    return _CACHE[key]


SCALE = 0.01   # A = SCALE * identity: hf = 100 r, one unit of h is 0.01 in r


def _spots(rng, h, m, spread=0.1):
    """m spots near index h: (h + d) * SCALE with |d_j| < spread"""
    return (np.asarray(h, F) + (rng.random((m, 3)) * 2 - 1) * spread) * SCALE


def built_groups():
    if "groups" in _CACHE:
        return _CACHE["groups"]
    rng = np.random.default_rng(31)
    rlp, phi = [], []

    def add(r, p):
        rlp.extend(np.asarray(r, F).reshape(-1, 3))
        phi.extend(np.asarray(p, F).reshape(-1))

    # groups of 1, 2, 3, 64, 65 and 200 on one index each; phi over 2 rad, so some pairs are in the window and some are not
    for h, m in (((1, 2, 3), 1), ((2, 2, 3), 2), ((3, 2, 3), 3), ((4, -2, 3), 64), ((-5, 2, 3), 65), ((6, 2, -3), 200)):
        add(_spots(rng, h, m), rng.random(m) * 2.0)
    # ... and the same sizes with every member inside the window (a chain of kills through the whole group)
    for h, m in (((1, 7, 3), 2), ((2, 7, 3), 3), ((3, 7, 3), 64), ((4, 7, 3), 65), ((5, 7, 3), 200)):
        add(_spots(rng, h, m), rng.random(m) * 0.5)
    # exact lsq ties: identical rlp, the later spot dies; three of a kind
    tie = _spots(rng, (9, 1, 1), 1)
    add(np.repeat(tie, 2, 0), [0.1, 0.2])
    tie = _spots(rng, (9, 2, 1), 1)
    add(np.repeat(tie, 3, 0), [0.3, 0.1, 0.2])
    # phi chains 0, 0.5, 1.0, 1.5: neighbours are in the window, next-neighbours are not; lsq ascending, descending and mixed
    chain_phi = [0.0, 0.5, 1.0, 1.5]
    for h, d in (((10, 1, 1), (0.01, 0.02, 0.03, 0.04)), ((10, 2, 1), (0.04, 0.03, 0.02, 0.01)), ((10, 3, 1), (0.02, 0.01, 0.04, 0.03)), ((10, 4, 1), (0.03, 0.04, 0.01, 0.02)),
                 ((10, 5, 1), (0.02, 0.02, 0.02, 0.02))):
        add([(np.asarray(h, F) + [x, 0, 0]) * SCALE for x in d], chain_phi)
    # the first member is killed midway: it kills the second, is killed by the third, the fourth then meets the third
    add([(np.asarray((11, 1, 1), F) + [x, 0, 0]) * SCALE for x in (0.05, 0.08, 0.02, 0.03, 0.01)], [0.0, 0.1, 0.2, 0.3, 0.4])
    # keys that differ only in the last component, and keys with negative components
    for h in ((12, 4, 5), (12, 4, 6), (-12, -4, -5), (-12, 4, -5), (-12, -4, -6)):
        add(_spots(rng, h, 3), rng.random(3) * 0.5)
    # singles, and spots beyond the tolerance
    add(_spots(rng, (0, 0, 0), 40, spread=20.0), rng.random(40) * 2.0)
    rlp, phi = np.array(rlp, F), np.array(phi, F)
    mix = rng.permutation(len(rlp))   # the members of a group lie anywhere among the spots
    keep = np.zeros(len(rlp), bool)
    first_hand = 1 + 2 + 3 + 64 + 65 + 200 + 2 + 3 + 64 + 65 + 200
    keep[first_hand:first_hand + 2 + 3 + 20 + 5] = True
    # a permutation that moves the random groups' members anywhere and leaves the hand-ordered spots in their relative order
    pos = np.argsort(mix)
    hand = np.flatnonzero(keep)
    pos[hand] = np.sort(pos[hand])
    perm = np.argsort(pos)
    A = np.array([SCALE, 0, 0, 0, SCALE, 0, 0, 0, SCALE], F)
    sel = np.ones(len(rlp), bool)
    sel[::7] = False   # leaves out members of groups too
    out = [case("built-groups", rlp[perm], phi[perm], A), case("built-groups-selected", rlp[perm], phi[perm], A, selected=sel)]
    _CACHE["groups"] = out
    return out


def _lsq_at(target):
    """(x, y1, y2) with (x x + y1 y1) + y2 y2 == target exactly, x near sqrt(target), y1 and y2 powers of two (or 0)"""
    x = F(math.sqrt(float(target)))
    for _ in range(400):
        for y1 in (0.0, 2.0 ** -28, 2.0 ** -27, 2.0 ** -26):
            for y2 in (0.0, 2.0 ** -28, 2.0 ** -27, 2.0 ** -26):
                if (x * x + F(y1) * F(y1)) + F(y2) * F(y2) == target:
                    return float(x), y1, y2
        x = np.nextafter(x, F(0.0))
    raise AssertionError("no decomposition")


def corners():
    if "corners" in _CACHE:
        return _CACHE["corners"]
    I = np.eye(3).reshape(9)
    out = []
    # hf at the rounding's corners (A = identity: hf = r exactly), each with a second component that makes h != 0
    halves = [0.5, -0.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 1.5, -1.5, 0.0, 3.0]
    rlp = [[x, 1.0, 0.0] for x in halves] + [[1.0, x, -2.0] for x in halves] + [[0.0, 1.0, x] for x in halves]
    out.append(case("halves", rlp, np.linspace(0.0, 6.0, len(rlp)), I, tolerance=0.5))
    out.append(case("halves-strict", rlp, np.linspace(0.0, 6.0, len(rlp)), I, tolerance=0.3))
    # lsq one ulp either side of tolerance^2, and on it
    for tol in (0.3, 0.2):
        t2 = F(tol) * F(tol)
        rl = []
        for target in (np.nextafter(t2, F(0.0)), t2, np.nextafter(t2, F(1.0))):
            x, y1, y2 = _lsq_at(target)
            rl.append([x, 1.0 + y1, y2])
            rl.append([-x, -1.0 - y1, -y2])
        out.append(case(f"tolerance-edge-{tol}", rl, np.arange(len(rl)) * 1.0, I, tolerance=tol, targets=[np.nextafter(t2, F(0.0)), t2, np.nextafter(t2, F(1.0))]))
    # an accepted (0, 0, 0), the origin itself, and the range's edge
    edge = [[0.1, 0.1, 0.1], [0.0, 0.0, 0.0], [524287.5, 1.0, 0.0], [-524287.5, 1.0, 0.0], [524288.0, 1.0, 0.0], [1.0, -524288.0, 0.0], [1.0, 0.0, 524287.0], [1.0, 2.0, -524287.25],
            [1.0, 0.0, 1e300], [524287.75, 0.25, 0.0]]
    out.append(case("range-edge", edge, np.zeros(len(edge)), I, tolerance=0.5))
    # a singular setting, one of rank two, a nearly singular one and one with an overflowing inverse among good ones
    lat = lattice("small-disturbed")
    good = lat["A"][lat["n_own"]]
    near = good.copy()
    near[6:9] = near[0:3] * 2.0 + near[3:6] * F(1e-13)
    tiny = good * F(1e-200)
    A = np.stack([good, np.zeros(9), np.array([1, 2, 3, 2, 4, 6, 0, 1, 0], F), near, tiny, good * F(0.5), np.full(9, 1e-320)])
    out.append(case("singular-among-good", lat["rlp"], lat["phi"], A))
    _CACHE["corners"] = out
    return out


def shaped(n):
    """n spots of a lattice (beyond its 4093: the same spots again with a little noise, which are duplicates under the true setting)"""
    lat = lattice("triclinic-disturbed", 200)
    rlp, phi = lat["rlp"], lat["phi"]
    if n > len(rlp):
        extra = n - len(rlp)
        rng = np.random.default_rng(n)
        rlp = np.concatenate([rlp, rlp[:extra] + rng.normal(size=(extra, 3)) * 1e-4])
        phi = np.concatenate([phi, phi[:extra] + 0.01])
    return rlp[:n], phi[:n], lat["A"]


def check_cases():
    """The cases the check program, the host tool and the GPU are held to the oracle on (the large lattice with a few settings only)"""
    if "check" not in _CACHE:
        tri = lattice("triclinic-disturbed", 200)
        few = np.concatenate([tri["A"][:6], tri["A"][-3:]])
        _CACHE["check"] = [lattice("small-disturbed"), dict(tri, name="triclinic-few", A=few)] + built_groups() + corners()
    return _CACHE["check"]


_EXPECTED = {}


def expected(c):
    """(records, hkl, lsq) of the oracle for a case, computed once"""
    key = (c["name"], len(c["rlp"]), len(c["A"]))
    if key not in _EXPECTED:
        _EXPECTED[key] = AO.assign_many(c["rlp"], c["phi"], c["A"], c["tolerance"], c["selected"])
    return _EXPECTED[key]
