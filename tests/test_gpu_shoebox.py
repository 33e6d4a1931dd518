"""GPU: summation integration of shoeboxes in Kabsch space (ffs_ctx_shoebox_begin, ffs_stream_shoebox_fold, ffs_ctx_get_shoebox_sums,
ffs_ctx_get_shoebox_histogram) through the C ABI, bit for bit against tests/shoebox_oracle.py: every integer, every histogram bin, the
flags, and bg_mean, intensity and variance as float64 bit patterns under both background models.  Frames of 96 x 80 pixels, 16 and 32
bits, both algorithms, max_valid set and unset, submitted in batches of 1, 3 and 8 and folded over the three batches; hand-placed boxes at
every edge the kernel has (the image's four sides and a corner, one pixel wide and high, wider and higher than a wave's 64 lanes, corner
grids of exactly 64 and 65 columns, z-ranges before, after, across and outside the folded images, phi on an image's edge) and a hundred
random ones.  Then: order independence, no side effects on the batch, every refusal with the state unchanged, begin-end-begin, n = 0."""
import numpy as np
import pytest

import shoebox_cases as K
import shoebox_oracle as O

pytestmark = pytest.mark.gpu

W, H = K.W, K.H
N_IMAGES = 12
BATCHES = [(0, 1), (1, 4), (4, 12)]   # batches of 1, 3 and 8 frames
MAX_VALID = 60000


def table(g, rng):
    at = lambda x0, x1, y0, y1, z0, z1, **kw: K.box(g, kw.get("x", (x0 + x1) / 2), kw.get("y", (y0 + y1) / 2), kw.get("z", (z0 + z1) / 2), x0, x1, y0, y1, z0, z1)
    hand = [
        at(30, 41, 20, 31, 2, 6),                 # inside the image; its z-range straddles the seam between the batches [1, 4) and [4, 12)
        at(-4, 5, 30, 39, 1, 4),                  # over the left edge
        at(W - 5, W + 4, 30, 39, 1, 4),           # over the right edge
        at(50, 59, -3, 6, 1, 4),                  # over the top edge
        at(50, 59, H - 4, H + 5, 1, 4),           # over the bottom edge
        at(-5, 4, -5, 4, 0, 3),                   # over a corner, negative minima
        at(50, 51, 30, 40, 2, 5),                 # one pixel wide
        at(50, 60, 33, 34, 2, 5),                 # one pixel high
        at(10, 80, 40, 43, 3, 6),                 # 70 x 3: wider than a wave's 64 lanes
        at(60, 65, 5, 75, 3, 6),                  # 5 x 70: higher than 64
        at(5, 68, 60, 64, 4, 7),                  # a corner grid of exactly 64 columns
        at(5, 69, 64, 68, 4, 7),                  # ... and of 65
        at(28, 38, 22, 33, 3, 8), at(33, 45, 18, 28, 1, 5), at(30, 41, 20, 31, 2, 6, x=36.2, y=26.7),   # overlapping the first in x, y and z
        at(20, 29, 60, 69, -2, 2),                # starts before the first folded image
        at(20, 29, 60, 69, 10, 15),               # ends after the last
        at(70, 79, 60, 69, 3, 6),                 # straddles a batch seam
        at(70, 79, 10, 19, 20, 25), at(70, 79, 10, 19, -9, -4),   # miss every image
        at(15, 24, 10, 19, 3, 8, z=5.0),          # phi exactly on image 5's phi_low
        at(36, 47, 25, 36, 2, 6),                 # the dead columns 40-42 in its foreground
        at(20, 31, 50, 61, 2, 6, y=52.5),         # the dead rows 55-56 in its background
    ]
    return np.concatenate([np.array(hand, O.BOX_DT), K.random_boxes(rng, g, 100, N_IMAGES)])


_cases = {}


def case(dtype, algorithm, max_valid):
    """Geometry, frames, mask, table and the oracle's accumulators over the twelve images, computed once per combination."""
    key = (np.dtype(dtype).name, algorithm, max_valid)
    if key not in _cases:
        rng = np.random.default_rng(977 + 2 * np.dtype(dtype).itemsize + algorithm)
        g = K.random_geometry(rng)
        c = dict(g=g, dtype=dtype, algorithm=algorithm, max_valid=max_valid, frames=K.frames(rng, dtype, N_IMAGES), mask=K.mask(rng), boxes=table(g, rng),
                 delta_b=2.0 * K.pixel_angle(g), delta_m=float(g["osc_width_deg"] * O.DEG), census={})
        f = c["frames"]
        f[3, 25, 35], f[4, 26, 36], f[3, 22, 31], f[4, 29, 39] = 65535, 255, 256, 255   # in the first box: at its centre and in its background
        if f.dtype.itemsize == 4:
            f[5, 25, 35], f[5, 26, 35], f[5, 21, 31], f[5, 21, 32] = 1 << 24, (1 << 24) - 1, 1 << 24, (1 << 24) - 1
        c["acc"] = oracle_fold(c, range(N_IMAGES), c["census"])
        _cases[key] = c
    return _cases[key]


def oracle_fold(c, images, census=None):
    images = list(images)
    return O.fold(c["g"], c["boxes"], c["algorithm"], c["delta_b"], c["delta_m"], c["frames"][images[0]:images[-1] + 1], images[0], c["mask"], c["max_valid"],
                  O.new_accumulators(len(c["boxes"])), census)


def open_job(ffs, c, max_batch=8, **params):
    ctx = ffs.Context(W, H, c["dtype"], max_batch=max_batch)
    ctx.set_mask(c["mask"])
    ctx.set_params(max_valid=c["max_valid"], **params)
    ctx.shoebox_begin(c["g"], c["boxes"], c["algorithm"], delta_b=c["delta_b"], delta_m=c["delta_m"])
    return ctx


def fold_batches(st, c, batches):
    for a, b in batches:
        st.process(c["frames"][a:b], first_frame_id=a)
        st.shoebox_fold(a)


def assert_matches(ctx, acc, what):
    for background in ("tukey", "glm"):
        got = ctx.shoebox_sums(background)
        assert got.dtype == O.SUM_DT and not got["reserved"].any()
        O.assert_records_equal(got, O.sums(acc, background), f"{what}, {background}")
    hist = np.stack([ctx.shoebox_histogram(i) for i in range(len(acc["fg_sum"]))])
    assert np.array_equal(hist, acc["hist"].astype(np.uint32)), (what, np.argwhere(hist != acc["hist"])[:8])


COMBOS = [(d, a, m) for d in (np.uint16, np.uint32) for a in (O.ELLIPSOID, O.DIALS) for m in (-1, MAX_VALID)]
IDS = [f"{np.dtype(d).name}-{'dials' if a else 'ellipsoid'}-{'max_valid' if m >= 0 else 'no_max_valid'}" for d, a, m in COMBOS]


@pytest.mark.parametrize("dtype,algorithm,max_valid", COMBOS, ids=IDS)
def test_three_batches_match_the_oracle_bit_for_bit(ffs, dtype, algorithm, max_valid):
    c = case(dtype, algorithm, max_valid)
    ctx = open_job(ffs, c)
    fold_batches(ctx.stream(), c, BATCHES)
    assert_matches(ctx, c["acc"], "batches of 1, 3 and 8")
    ctx.shoebox_end()


def test_the_cases_contain_what_they_are_built_for():
    """On the oracle alone: foreground, background, overflow pixels, FG_INVALID from every cause, boxes that no image met."""
    c16, c32 = case(np.uint16, O.ELLIPSOID, MAX_VALID), case(np.uint32, O.ELLIPSOID, -1)
    for c in (c16, c32):
        s = c["census"]
        assert s["foreground"] > 500 and s["background"] > 5000 and s["overflow"] > 5
        assert 0 in s["edge"] or {1, 2, 3, 4, 5} <= s["edge"], s["edge"]
        assert 21 in s["mask"]
        acc = c["acc"]
        for i in (18, 19):
            assert acc["fg_count"][i] == 0 and acc["hist"][i].sum() == 0 and acc["flags"][i] == 0   # no image met them
        assert all(acc["fg_count"][i] > 0 for i in range(18)), [acc["fg_count"][i] for i in range(18)]
        assert acc["hist"][0, 255] > 0 and acc["n_overflow"][0] > 0                               # the 255 and the 256 in the first box's background
    assert 0 in c16["census"]["max_valid"] and 0 in c32["census"]["ge_2_24"]
    assert "max_valid" not in case(np.uint16, O.ELLIPSOID, -1)["census"]                         # (65535 counts without a max_valid)


@pytest.mark.parametrize("dtype,algorithm", [(np.uint16, O.ELLIPSOID), (np.uint32, O.DIALS)], ids=["u16-ellipsoid", "u32-dials"])
def test_order_batching_and_streams_do_not_matter(ffs, dtype, algorithm):
    c = case(dtype, algorithm, MAX_VALID)
    want = oracle_fold(c, range(8))
    parts = [(0, 1), (1, 4), (4, 8)]
    records = []
    for order in (parts, parts[::-1], [(0, 8)]):
        ctx = open_job(ffs, c)
        fold_batches(ctx.stream(), c, order)
        assert_matches(ctx, want, f"order {order}")
        records.append((ctx.shoebox_sums("tukey").tobytes(), ctx.shoebox_sums("glm").tobytes()))
    # alternately on two streams, each fold after the other stream's batch has been waited for too
    ctx = open_job(ffs, c)
    s1, s2 = ctx.stream(), ctx.stream()
    s1.process(c["frames"][0:1])
    s2.process(c["frames"][1:4])
    s2.shoebox_fold(1)
    s1.shoebox_fold(0)
    s1.process(c["frames"][4:8])
    s1.shoebox_fold(4)
    records.append((ctx.shoebox_sums("tukey").tobytes(), ctx.shoebox_sums("glm").tobytes()))
    assert all(r == records[0] for r in records)


def test_a_fold_leaves_the_batch_as_it_was(ffs):
    c = case(np.uint16, O.ELLIPSOID, MAX_VALID)
    ctx = open_job(ffs, c, want_reflections=1)
    st = ctx.stream()
    res = st.process(c["frames"][4:12], first_frame_id=4)
    before = (st.spot_backgrounds(3).tobytes(), st.spot_backgrounds_glm(3).tobytes(), st.last_path())
    assert sum(len(r.reflections) for r in res) > 0
    st.shoebox_fold(4)
    assert (st.spot_backgrounds(3).tobytes(), st.spot_backgrounds_glm(3).tobytes(), st.last_path()) == before
    # ... and a context that had a job gives a run's results as one that never had
    ctx.shoebox_end()
    plain = ffs.Context(W, H, c["dtype"], max_batch=8)
    plain.set_mask(c["mask"])
    plain.set_params(max_valid=c["max_valid"], want_reflections=1)
    st1, st2 = ctx.stream(), plain.stream()   # (two new streams: a stream's re-runs depend on the batches it has seen)
    for a, b in zip(st1.process(c["frames"][4:12], first_frame_id=4), st2.process(c["frames"][4:12], first_frame_id=4)):
        assert a.num_strong_pixels == b.num_strong_pixels and a.boxes.tobytes() == b.boxes.tobytes() and a.reflections.tobytes() == b.reflections.tobytes()
    assert st1.last_path() == st2.last_path()


def refused(ffs, call, *needles):
    with pytest.raises(ffs.FfsError) as e:
        call()
    assert e.value.code == -1 and all(n in str(e.value) for n in needles), str(e.value)


def test_every_refusal_leaves_the_state_unchanged(ffs):
    c = case(np.uint16, O.ELLIPSOID, MAX_VALID)
    g, boxes, db, dm = c["g"], c["boxes"], c["delta_b"], c["delta_m"]
    ctx = ffs.Context(W, H, np.uint16, max_batch=8)
    ctx.set_mask(c["mask"])
    ctx.set_params(max_valid=MAX_VALID)
    st = ctx.stream()
    no_job = lambda: refused(ffs, lambda: ctx.shoebox_sums(), "no job")
    # without a job: the getters and the fold
    no_job()
    refused(ffs, lambda: ctx.shoebox_histogram(0), "no job")
    refused(ffs, lambda: st.shoebox_fold(0), "no batch has been waited")
    st.process(c["frames"][0:1])
    refused(ffs, lambda: st.shoebox_fold(0), "no job")
    # begin: the deltas, the algorithm, the geometry, every kind of table entry -- none opens a job
    for bad in (0.0, -1e-3, np.inf, np.nan):
        refused(ffs, lambda: ctx.shoebox_begin(g, boxes, delta_b=bad, delta_m=dm), "delta_b")
        refused(ffs, lambda: ctx.shoebox_begin(g, boxes, delta_b=db, delta_m=bad), "delta_m")
    refused(ffs, lambda: ctx.shoebox_begin(g, boxes, 7, delta_b=db, delta_m=dm), "algorithm")
    refused(ffs, lambda: ctx.shoebox_begin(dict(g, wavelength=0.0), boxes, delta_b=db, delta_m=dm), "positive")
    refused(ffs, lambda: ctx.shoebox_begin(dict(g, osc_width_deg=np.nan), boxes, delta_b=db, delta_m=dm), "not finite")
    for field, value, needle in (("x_max", -100, "empty or reversed"), ("y_max", -100, "empty or reversed"), ("z_max", -100, "empty or reversed"), ("x_max", 2000, "wider"),
                                 ("y_max", 2000, "higher"), ("phi", np.inf, "phi"), ("s1", [np.nan, 0, -1], "s1"), ("s1", [0, 0, -1.0], "parallel")):
        t = boxes.copy()
        t[field][2] = value
        refused(ffs, lambda: ctx.shoebox_begin(g, t, delta_b=db, delta_m=dm), "shoebox 2 ", needle)
    t = boxes.copy()
    t["x_min"][5], t["x_max"][5] = W + 1024, W + 1030
    refused(ffs, lambda: ctx.shoebox_begin(g, t, delta_b=db, delta_m=dm), "shoebox 5 ", "outside the image")
    no_job()
    # begin while a batch of the context is in flight
    st.submit(c["frames"][0:1])
    refused(ffs, lambda: ctx.shoebox_begin(g, boxes, delta_b=db, delta_m=dm), "in flight")
    st.wait()
    no_job()

    # with a job open and one batch folded: nothing below changes a record
    ctx.shoebox_begin(g, boxes, delta_b=db, delta_m=dm)
    st.process(c["frames"][0:1])
    st.shoebox_fold(0)
    state = ctx.shoebox_sums("glm").tobytes()
    refused(ffs, lambda: ctx.shoebox_begin(g, boxes, delta_b=db, delta_m=dm), "a job is open")
    refused(ffs, lambda: st.shoebox_fold(-1), "first_image")
    refused(ffs, lambda: st.shoebox_fold(2**31 - 1), "first_image")
    refused(ffs, lambda: ctx.stream().shoebox_fold(0), "no batch has been waited")
    refused(ffs, lambda: ctx.shoebox_sums(2), "background_model")
    refused(ffs, lambda: ctx.shoebox_histogram(len(boxes)), "outside the table")
    st.submit(c["frames"][1:4])
    refused(ffs, lambda: st.shoebox_fold(1), "in flight")
    st.wait()
    assert ctx.shoebox_sums("glm").tobytes() == state
    O.assert_records_equal(ctx.shoebox_sums("tukey"), O.sums(oracle_fold(c, range(1)), "tukey"), "after the refusals")


def test_begin_end_begin_starts_from_zero(ffs):
    c = case(np.uint32, O.ELLIPSOID, -1)
    ctx = open_job(ffs, c)
    st = ctx.stream()
    fold_batches(st, c, [(0, 1), (1, 4)])
    assert ctx.shoebox_sums()["fg_count"].any()
    ctx.shoebox_end()
    ctx.shoebox_end()   # (idempotent)
    ctx.shoebox_begin(c["g"], c["boxes"], c["algorithm"], delta_b=c["delta_b"], delta_m=c["delta_m"])
    zero = ctx.shoebox_sums()
    assert not zero["fg_count"].any() and not zero["fg_sum"].any() and not zero["n_background"].any() and not zero["flags"].any()
    assert (zero["variance"] == -1.0).all() and not ctx.shoebox_histogram(0).any()
    fold_batches(st, c, [(4, 12)])
    assert_matches(ctx, oracle_fold(c, range(4, 12)), "the second job")
    # folding an image twice counts it twice
    st.shoebox_fold(4)
    twice = ctx.shoebox_sums()
    once = O.sums(oracle_fold(c, range(4, 12)))
    assert np.array_equal(twice["fg_sum"], 2 * once["fg_sum"]) and np.array_equal(twice["fg_count"], 2 * once["fg_count"])


def test_an_empty_table(ffs):
    c = case(np.uint16, O.DIALS, -1)
    ctx = ffs.Context(W, H, np.uint16, max_batch=8)
    ctx.shoebox_begin(c["g"], np.zeros(0, O.BOX_DT), "dials", delta_b=c["delta_b"], delta_m=c["delta_m"])
    st = ctx.stream()
    st.process(c["frames"][0:3])
    assert st.shoebox_fold(0, want_ms=True) == 0.0
    assert len(ctx.shoebox_sums("tukey")) == 0 and len(ctx.shoebox_sums("glm")) == 0
    with pytest.raises(ffs.FfsError):
        ctx.shoebox_histogram(0)
    ctx.shoebox_end()
