"""GPU: scan prediction (ffs_ctx_predict, ffs_predict_scan_settings) through the C ABI, bit for bit against tests/predict_oracle.py fed the
library's own scan-point settings: every field of every record and their order, on the cases of tests/predict_cases.py (the main case of
40 x 45 x 50 A at dmin 2 over 16 images of 0.5 deg on 300 x 200 pixels, and the sizes at which a launch can go wrong); cap below n; two
calls; a call while a batch is in flight; the hand-off to ffs_ctx_shoebox_begin; every refusal."""
import numpy as np
import pytest

import predict_cases as K
import predict_oracle as O

pytestmark = pytest.mark.gpu

W, H = K.W, K.H
CASES = {c["name"]: c for c in K.cases()}
_oracle = {}


def args(c):
    return (c["g"], c["A"], c["n_images"], c["dmin"], c["delta_b"], c["delta_m"], c["centring"])


def expected(ffs, c):
    """The oracle's records for the library's scan-point settings, and its census; computed once per case."""
    if c["name"] not in _oracle:
        settings = ffs.predict_scan_settings(c["g"], c["A"], c["n_images"])
        census = {}
        rec = O.predict(c["g"], c["A"], c["n_images"], c["dmin"], c["delta_b"], c["delta_m"], W, H, c["centring"], settings, census)
        _oracle[c["name"]] = (rec, census)
    return _oracle[c["name"]]


@pytest.fixture(scope="module")
def ctx(ffs):
    return ffs.Context(W, H, np.uint16, max_batch=4)


def assert_same(got, want, what):
    assert got.dtype.itemsize == 96 and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        for name in O.PREDICTION_DT.names:
            bad = np.nonzero(np.any(np.atleast_2d((got[name] != want[name]).T), axis=0))[0]
            assert len(bad) == 0, (what, name, bad[:5], got[bad[:3]], want[bad[:3]])
        raise AssertionError(what + ": the bytes differ where no field does")


@pytest.mark.parametrize("name", list(CASES))
def test_the_records_equal_the_oracles_bit_for_bit(ffs, ctx, name):
    c = CASES[name]
    want, census = expected(ffs, c)
    got = ctx.predict(*args(c))
    assert_same(got, want, name)
    if name == "nothing":
        assert len(got) == 0
    if name == "every-seam":
        assert list(np.unique(census["q"] // 256)) == list(range((census["candidates"] + 255) // 256)), "some candidate of every workgroup predicts"
    if name == "full-turn":
        assert np.max(np.unique(census["q"], return_counts=True)[1]) >= 2, "a lane whose count exceeds one"
    if name == "main":
        assert census["negative_d"] == 0 and census["rootless"] == 0 and census["candidates"] % 64 != 0 and census["crossings"] > len(want) > 1500


def test_the_flags_the_cases_are_built_for(ffs, ctx):
    for name, flag in (("zeta-small", O.ZETA_SMALL), ("corner-lost", O.CORNER_LOST), ("box-refused", O.BOX_REFUSED)):
        got = ctx.predict(*args(CASES[name]))
        assert np.any(got["flags"] & flag), name
    wide = ctx.predict(*args(CASES["wide-boxes"]))
    assert np.any(wide["x_min"] < 0) and np.any(wide["y_min"] < 0) and np.any(wide["x_max"] > W) and np.any(wide["y_max"] > H)
    assert np.any((wide["z_min"] == 0) & (wide["z_max"] == 16))


def test_a_cap_below_n_gives_the_first_records_and_the_full_count(ffs, ctx):
    c = K.MAIN
    want, _ = expected(ffs, c)
    for cap in (1, 255, 257, len(want) - 1):
        with pytest.raises(ffs.FfsError) as e:
            ctx.predict(*args(c), cap=cap)
        assert e.value.code == -4 and e.value.n == len(want)
        assert e.value.records.tobytes() == want[:cap].tobytes(), cap
    assert_same(ctx.predict(*args(c), cap=len(want)), want, "cap == n")
    assert_same(ctx.predict(*args(c), cap=len(want) + 1000), want, "cap > n")


def test_two_calls_give_identical_bytes(ffs, ctx):
    a, ms = ctx.predict(*args(K.MAIN), want_ms=True)
    b = ctx.predict(*args(K.MAIN))
    assert a.tobytes() == b.tobytes() and ms > 0.0
    other = ffs.Context(W, H, np.uint32, max_batch=1)
    assert other.predict(*args(K.MAIN)).tobytes() == a.tobytes()


def test_a_call_while_a_batch_is_in_flight(ffs):
    from ffs_amd import synth
    frames = synth.frames(synth.params(W, H, np.uint16, seed=5, background=2.0, n_spots=30), range(4))
    c = ffs.Context(W, H, np.uint16, max_batch=4)
    c.set_params(want_reflections=1)
    quiet = c.predict(*args(K.MAIN))
    st, st2 = c.stream(), c.stream()
    before = st2.process(frames)
    st.submit(frames)
    busy = c.predict(*args(K.MAIN))
    after = st.wait()
    assert busy.tobytes() == quiet.tobytes()
    assert sum(r.num_strong_pixels for r in after) > 0
    for a, b in zip(before, after):
        assert a.num_strong_pixels == b.num_strong_pixels and a.boxes.tobytes() == b.boxes.tobytes() and a.reflections.tobytes() == b.reflections.tobytes()


def test_the_predictions_are_a_table_shoebox_begin_takes(ffs):
    import shoebox_oracle as S
    c = K.case("hand-off", dmin=4.0, delta_b=0.012, delta_m=0.01)
    ctx = ffs.Context(W, H, np.uint16, max_batch=4)
    pred = ctx.predict(*args(c))
    table = ffs.shoeboxes_of(pred)
    assert len(table) == len(pred) > 100 and table.dtype.itemsize == 56
    with_refused = ctx.predict(*args(CASES["box-refused"]))
    assert 0 < len(ffs.shoeboxes_of(with_refused)) + np.count_nonzero(with_refused["flags"] & O.BOX_REFUSED) == len(with_refused)
    assert len(ffs.shoeboxes_of(with_refused, skip_refused=False)) == len(with_refused)
    rng = np.random.default_rng(31)
    frames = rng.poisson(3.0, (4, H, W)).astype(np.uint16)
    frames[rng.random(frames.shape) < 0.01] = 900
    ctx.shoebox_begin(c["g"], table, "ellipsoid", delta_b=c["delta_b"], delta_m=c["delta_m"])
    st = ctx.stream()
    st.process(frames, first_frame_id=0)
    st.shoebox_fold(0)
    boxes = np.zeros(len(table), S.BOX_DT)
    for name in S.BOX_DT.names:
        boxes[name] = table[name]
    acc = S.fold(c["g"], boxes, S.ELLIPSOID, c["delta_b"], c["delta_m"], frames, 0, None, -1, S.new_accumulators(len(boxes)), None)
    S.assert_records_equal(ctx.shoebox_sums("tukey"), S.sums(acc, "tukey"), "the fold over the predicted table")
    assert np.count_nonzero(acc["fg_count"]) > 10
    ctx.shoebox_end()


def refused(ffs, call, *needles):
    with pytest.raises(ffs.FfsError) as e:
        call()
    assert e.value.code == -1 and all(n in str(e.value) for n in needles), str(e.value)


def test_every_refusal_through_the_live_context(ffs, ctx):
    c = K.MAIN
    g, A = c["g"], c["A"]
    want, _ = expected(ffs, c)
    p = lambda g=g, A=A, n=16, dmin=2.0, db=0.01, dm=0.004, centring=0: ctx.predict(g, A, n, dmin, db, dm, centring)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(ffs, lambda: p(dmin=bad), "dmin")
        refused(ffs, lambda: p(db=bad), "delta_b")
        refused(ffs, lambda: p(dm=bad), "delta_m")
    refused(ffs, lambda: p(g=dict(g, wavelength=0.0)), "positive")
    refused(ffs, lambda: p(g=dict(g, pixel_size_mm=[0.5, -0.5])), "positive")
    refused(ffs, lambda: p(g=dict(g, osc_width_deg=0.0)), "osc_width_deg")
    refused(ffs, lambda: p(g=dict(g, s0=[0.0, np.nan, -1.0])), "not finite")
    refused(ffs, lambda: p(A=np.where(np.arange(9) == 4, np.inf, A)), "a_matrix", "not finite")
    refused(ffs, lambda: p(A=np.zeros(9)), "a_matrix is singular")
    refused(ffs, lambda: p(A=np.array([1, 2, 3, 2, 4, 6, 0, 0, 1.0]) / 64.0), "a_matrix is singular")
    refused(ffs, lambda: p(g=dict(g, d_matrix=np.array([1, 0, 0, 0, 1, 0, 1, 1, 0.0]))), "d_matrix is singular")
    refused(ffs, lambda: p(n=0), "n_images")
    refused(ffs, lambda: p(n=65536), "n_images")
    refused(ffs, lambda: p(centring=7), "centring")
    refused(ffs, lambda: p(centring=-1), "centring")
    refused(ffs, lambda: p(dmin=0.01), "2^31 - 1")
    refused(ffs, lambda: p(A=np.asarray(A) * 1e-9), "2^31 - 1")
    with pytest.raises(ffs.FfsError) as e:
        ffs.predict_scan_settings(g, A, 0)
    assert e.value.code == -1 and "n_images" in str(e.value)
    import ctypes as C
    lib = ffs.load_library()
    n = C.c_uint32(77)
    assert lib.ffs_ctx_predict(ctx._h, None, None, 16, 2.0, 0.01, 0.004, None, 0, C.byref(n), None) == -1 and n.value == 77
    assert b"NULL" in lib.ffs_last_error(ctx._h)
    assert_same(p(), want, "after the refusals")
