"""CPU: the tie frames of tests/tie_windows.py -- every family present on each side of its boundary, the cells' exact
decisions against the oracle restatement (standard and extended algorithm, every parameter set the GPU tests use), the
integer-predicate model against the same cells, and the restatement against the compiled reference on the frames themselves
(live where oracle/_ref is built, and always against tests/golden/dispersion_ties.npz)."""
import os

import numpy as np
import pytest

import tie_windows as T
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispersion_ties.npz")

# minimum number of cells per (family, side) at the default parameters: fixed here, so that the generator cannot quietly stop
# producing ties
MIN_COMMON = {
    ("a", "below"): 20, ("a", "at"): 25, ("a", "above"): 20,
    ("b", "below"): 25, ("b", "at"): 25, ("b", "above"): 25,
    ("c", "below"): 10, ("c", "at"): 20, ("c", "above"): 10,
    ("d16", "below"): 8, ("d16", "above"): 8,
    ("d20", "out_below"): 8, ("d20", "in_below"): 8, ("d20", "in_above"): 8, ("d20", "out_above"): 8,
    ("e", "above"): 3,
    ("f", "below"): 3, ("f", "at"): 3, ("f", "above"): 3,
    ("j", "below"): 20, ("j", "at"): 20,
}
MIN_U16 = {("h", "below"): 2, ("h", "at"): 2, ("h", "above"): 2, ("h", "y_over_2^32"): 10}
MIN_U32 = {("i", f"{kind}_{v}"): n for kind, n in (("pixel", 3), ("centre", 2)) for v in (T.BIG - 1, T.BIG, T.BIG + 1)}
MIN_U32.update({("i", f"{lab}_{half}_{side}"): 1 for lab in ("y_2^46", "my_2^53") for half in ("lo", "hi")
                for side in ("below", "at", "above")})
# what the other parameter sets add
MIN_PARAMS = {
    "mincount3_maxvalid": {("g", "below"): 3, ("g", "at"): 3, ("g", "above"): 3},
    "threshold_40.5": {("e", "below"): 3, ("e", "above"): 3},
    "threshold_41": {("e", "below"): 3, ("e", "at"): 3, ("e", "above"): 3},
}


@pytest.mark.parametrize("dt", ["uint16", "uint32"])
def test_every_family_on_each_side(dt):
    fam = T.families(T.frame(dt))
    want = {**MIN_COMMON, **(MIN_U16 if dt == "uint16" else MIN_U32)}
    short = {k: (fam.get(k, 0), n) for k, n in want.items() if fam.get(k, 0) < n}
    assert not short, f"families below their minimum (have, want): {short}"


@pytest.mark.parametrize("name", sorted(MIN_PARAMS))
def test_parameter_families(name):
    fam = T.families(T.frame("uint16", T.PARAM_SETS[name]))
    short = {k: (fam.get(k, 0), n) for k, n in MIN_PARAMS[name].items() if fam.get(k, 0) < n}
    assert not short, short


def test_ties_are_ties():
    """The cells labelled "at" sit exactly on their boundary: b == d (family a), a == c (family b), both (family c)."""
    from fractions import Fraction
    tf = T.frame("uint16")
    ns, nb = Fraction(3), Fraction(6)
    n = 0
    for c in tf.cells:
        if c.side != "at" or c.family not in "abc":
            continue
        a, b = c.m * c.y - c.x * c.x - c.x * (c.m - 1), c.m * c.p - c.x
        if c.family in "ac":
            assert b * b == ns * ns * c.x * c.m and b > 0
        if c.family in "bc":
            assert a * a == nb * nb * c.x * c.x * 2 * (c.m - 1) and a > 0
        assert not c.exact and not c.f64
        n += 1
    assert n >= 70


def test_fill():
    """Whatever fill returns has the asked sums; it reaches most reachable targets (it is a greedy search, not a complete one)."""
    rng = np.random.default_rng(1)
    n_found = 0
    for _ in range(300):
        k = int(rng.integers(1, 49))
        v = rng.integers(0, int(rng.choice([3, 300, 65535])), k, endpoint=True)
        X, Y = int(v.sum()), int((v.astype(np.int64) ** 2).sum())
        got = T.fill(k, X, Y, 65535)
        if got is not None:
            n_found += 1
            assert len(got) == k and sum(got) == X and sum(t * t for t in got) == Y and 0 <= min(got) and max(got) <= 65535
    assert n_found >= 270
    assert T.fill(3, 10, 35, 65535) is None          # parity: the sum of squares of integers has the parity of their sum


@pytest.mark.parametrize("name", list(T.PARAM_SETS))
@pytest.mark.parametrize("dt", ["uint16", "uint32"])
def test_oracle_agrees_with_cells(name, dt):
    """O.dispersion and O.dispersion_extended decide every cell centre as exact arithmetic does, and as the oracle's float64
    operation sequence does; and each cell's window is the one it was built for."""
    prm = T.PARAM_SETS[name]
    tf = T.frame(dt, prm)
    img = tf.image.astype(np.int64)
    strong = O.dispersion(tf.image, tf.mask, prm.disp())
    _, first, _ = O.dispersion_extended(tf.image, tf.mask, prm.disp(), max_valid=float(prm.max_valid), debug=True)
    for c in tf.cells:
        win = img[c.row - 3:c.row + 4, c.col - 3:c.col + 4].ravel().tolist()
        ok = tf.mask[c.row - 3:c.row + 4, c.col - 3:c.col + 4].ravel().astype(bool).tolist()
        assert T.window_stats(win, ok) == (c.m, c.x, c.y) and win[24] == c.p
        what = (c.family, c.side, c.m, c.x, c.y, c.p)
        assert c.exact == c.f64 == bool(strong[c.row, c.col]), what
        assert c.first_exact == c.first_f64 == bool(first[c.row, c.col]), what
    for flavour in (0, 1):
        final = O.dispersion_extended(tf.image, tf.mask, prm.disp(), flavour=flavour, max_valid=float(prm.max_valid))
        for r, col, fam, side, want in tf.ext_cells:
            assert bool(final[r, col]) == want, (fam, side, flavour)


def test_int_predicate_model_on_cells():
    """The Python model of the device's int_predicate (tests/test_int_predicate_model.py) on every cell it covers (x < 65536):
    where it says "certain" it must agree with the exact decision; at the ties it must not be certain."""
    from test_int_predicate_model import int_predicate
    n_uncertain = 0
    for dt in ("uint16", "uint32"):
        for c in T.frame(dt).cells:
            if c.x >= 65536 or c.m < 2 or c.p > 65535:
                continue
            strong, certain = int_predicate(c.m, c.x, c.y, c.p, 6, 3)
            if certain:
                assert strong == c.exact, (c.family, c.side)
            else:
                n_uncertain += 1
            if c.side == "at" and c.family in "abc":
                assert not certain, (c.family, c.m, c.x, c.y, c.p)
    assert n_uncertain >= 100


@pytest.mark.parametrize("dt", ["uint16", "uint32"])
def test_port_equals_compiled_reference_on_ties(dt):
    tf = T.frame(dt)
    z = np.load(GOLD)
    assert str(z[f"{dt}/digest"]) == tf.digest(), "tests/tie_windows.py drifted from tests/golden/dispersion_ties.npz"
    assert tuple(z[f"{dt}/shape"]) == tf.image.shape
    want = np.unpackbits(z[f"{dt}/strong"])[: tf.image.size].reshape(tf.image.shape)
    if O.have_ref():
        H, W = tf.image.shape
        np.testing.assert_array_equal(O.RefSpotfinder(W, H)(tf.image, tf.mask), want)
    np.testing.assert_array_equal(O.dispersion(tf.image, tf.mask), want)
    np.testing.assert_array_equal(O.dispersion(tf.image.astype(np.float64), tf.mask), want)
