"""CPU: the inputs of tests/test_gpu_transitions.py are what that file needs them to be -- decided by the oracle alone -- and the
walker issues the calls it promises.  A walk over frames that are all empty, or over kinds whose parameters change nothing, would
pass on the GPU without having tested a thing."""
from collections import Counter

import numpy as np
import pytest

import batch_walk as BW


@pytest.fixture(scope="module")
def want():
    return BW.OracleCache()


def test_kind_list_is_the_issues():
    names = [k.name for k in BW.KINDS]
    assert len(names) == len(set(names)) >= 19
    assert set(names) >= {"default", "lists", "bytemask", "dense", "empty", "short", "overflow", "ext0", "ext1", "ext_plain", "win52",
                          "win_as_7x7", "path1", "path2", "plane", "grid", "device_in", "compressed", "odd_params"}
    K = BW.BY_NAME
    assert K["default"].params == {} and K["default"].tuning == {} and K["default"].mask == 0 and K["default"].form == "host"
    assert K["lists"].params == dict(want_strong_list=1, want_reflections=1)
    assert K["bytemask"].params == dict(want_strong_mask=1)
    i = names.index("bytemask")
    assert not BW.KINDS[i - 1].all_params["want_strong_mask"] and not BW.KINDS[i - 2].all_params["want_strong_mask"]
    assert len(K["short"].frames) == 1 and all(len(k.frames) == 3 for k in BW.KINDS if k.name != "short")
    assert K["ext0"].all_params["algorithm"] == 1 and K["ext0"].all_params["extended_flavour"] == 0
    assert K["ext1"].params == dict(algorithm=1, extended_flavour=1, want_strong_mask=1) and K["ext1"].mask == 1
    assert K["ext1"].tuning == dict(ext_e_sparse=1)
    assert K["ext_plain"].extended and K["ext_plain"].tuning == dict(ext_first_pass=0)
    assert K["win52"].params == dict(kernel_half_x=5, kernel_half_y=2) and K["win52"].mask == 1
    assert K["win_as_7x7"].tuning == dict(window_kernel=1) and K["win_as_7x7"].params == {}
    assert K["path1"].tuning == dict(threshold_path=1) and K["path2"].tuning == dict(threshold_path=2)
    assert K["plane"].tuning == dict(strong_log=0) and K["grid"].tuning == dict(sparse_stage=1)
    assert K["device_in"].form == "device" and K["compressed"].form == "compressed"
    for k in ("device_in", "compressed"):
        assert K[k].params == {} and K[k].tuning == {} and K[k].mask == 0
    assert K["odd_params"].params == dict(min_count=3, nsig_b=4.0, nsig_s=2.5, threshold=4.0, max_valid=1000, min_spot_size=1,
                                          max_peak_centroid_separation=0.5)
    # only the keys that may change between batches of a context
    for k in BW.KINDS:
        assert set(k.tuning) <= set(BW.DEFAULT_TUNING) and not set(k.tuning) & {"sched", "direct_records", "sparse_priority"}
        assert set(k.params) <= set(BW.DEFAULT_PARAMS)
    assert {k.name for k in BW.KINDS if k.window} == {"win52", "win_as_7x7"}
    assert {k.name for k in BW.KINDS if k.extended} == {"ext0", "ext1", "ext_plain"}


def test_default_parameters_are_the_librarys(ffs):
    from ffs_amd import api
    p = api.default_params()
    for key, value in BW.DEFAULT_PARAMS.items():
        if key == "want_reflections":
            continue                                   # (on in every kind, as bench.py and the driver set it)
        got = getattr(p, key)
        if key in ("kernel_half_x", "kernel_half_y"):
            got = got or 3                             # 0 means 3
        assert got == value, key


@pytest.mark.parametrize("n", [1, 2, 3, 7, len(BW.KINDS), len(BW.in_flight_kinds())])
def test_de_bruijn_holds_every_ordered_pair_once(n):
    seq = BW.de_bruijn(n)
    assert len(seq) == n * n and seq == BW.de_bruijn(n)          # (no randomness)
    pairs = Counter((seq[i - 1], seq[i]) for i in range(len(seq)))   # i = 0: the wrap-around pair
    assert len(pairs) == n * n and set(pairs.values()) == {1}
    assert set(pairs) == {(a, b) for a in range(n) for b in range(n)}


@pytest.mark.parametrize("offset", [0, 1, 90, 200])
def test_walk_runs_every_pair_on_the_stream(offset):
    w = BW.walk(BW.KINDS, offset)
    n = len(BW.KINDS)
    assert len(w) == n * n + 1 and w[0][0] is None
    pairs = Counter((p.name, k.name) for p, k in w[1:])
    assert len(pairs) == n * n and set(pairs.values()) == {1}
    for i in range(1, len(w)):
        assert w[i][0] is w[i - 1][1]                            # the previous kind is the batch before
    assert BW.walk()[0][1].name == "default"                     # the fresh stream's first batch


def test_in_flight_kinds_change_no_tuning_and_no_mask():
    kinds = BW.in_flight_kinds()
    assert all(not k.tuning and k.mask == 0 for k in kinds)
    names = {k.name for k in kinds}
    assert len(names) == len(kinds)
    assert names >= {"default", "lists", "bytemask", "dense", "empty", "short", "overflow", "ext0", "ext1_m0", "win52_m0", "device_in",
                     "compressed", "odd_params"}
    assert any(k.extended for k in kinds) and any(k.window for k in kinds)
    n = len(kinds)
    for i in range(4):                                           # the offsets the four streams start from
        assert len({(p.name, k.name) for p, k in BW.walk(kinds, i * (n * n // 4))[1:]}) == n * n


def test_dense_frames_are_beyond_the_lds_forest_and_within_the_run_plan(want):
    k = BW.BY_NAME["dense"]
    for f in range(3):
        w = want(k, f)
        assert BW.CHAIN_LDS_ENTRIES < w.cc.num_strong_pixels <= BW.MAX_STRONG, (f, w.cc.num_strong_pixels)
        runs, word_runs = BW.run_counts(w.strong)
        assert runs <= word_runs <= BW.CHAIN_MAX_RUNS, (f, runs, word_runs)   # (the plan counts runs cut at the plane's 32-pixel words)


def test_overflow_frame_is_beyond_the_lists(want):
    k = BW.BY_NAME["overflow"]
    assert k.frames[1] == "big" and want(k, 1).cc.num_strong_pixels > BW.MAX_STRONG
    for f in (0, 2):                                             # ... between two sparse ones
        assert 50 <= want(k, f).cc.num_strong_pixels <= 5000 and len(want(k, f).refl.reflections) >= 5


def test_empty_frames_hold_no_strong_pixel(want):
    k = BW.BY_NAME["empty"]
    assert not BW.frame(k.frames[0]).any() and BW.frame(k.frames[1]).all()     # all zero; no zero at all
    for f in range(3):
        assert want(k, f).cc.num_strong_pixels == 0 and want(k, f).strong.sum() == 0


@pytest.mark.parametrize("kind", [k for k in BW.KINDS if k.name not in BW.NOT_SPARSE]
                         + [k for k in BW.in_flight_kinds() if k.name.endswith("_m0")], ids=lambda k: k.name)
def test_sparse_kinds_have_something_to_find(want, kind):
    for f in range(len(kind.frames)):
        w = want(kind, f)
        assert 50 <= w.cc.num_strong_pixels <= 5000, (f, w.cc.num_strong_pixels)
        assert w.cc.num_strong_pixels == int(w.strong.sum())
        assert len(w.cc.boxes) >= 5 and len(w.refl.reflections) >= 5, (f, len(w.cc.boxes), len(w.refl.reflections))


@pytest.mark.parametrize("name", ["ext0", "ext1", "win52", "odd_params", "ext1_m0", "win52_m0"])
def test_parameters_change_the_strong_mask(want, name):
    """A path that silently kept the previous batch's parameters gives another mask: at least 10 pixels apart from the default's."""
    kind = {k.name: k for k in BW.KINDS + BW.in_flight_kinds()}[name]
    for f in range(3):
        with_defaults = BW.strong_mask(BW.BY_NAME["default"], BW.frame(kind.frames[f]), BW.masks()[kind.mask])
        assert int((want(kind, f).strong != with_defaults).sum()) >= 10, f


def test_extended_kinds_have_planes_to_compare(want):
    for name in ("ext0", "ext1", "ext_plain"):
        for f in range(3):
            w = want(BW.BY_NAME[name], f)
            assert w.first.sum() > 0 and w.eroded.sum() > 0 and not np.array_equal(w.first, w.eroded)


def test_the_two_masks_differ():
    m = BW.masks()
    assert m[0].all() and (m[0] != m[1]).mean() >= 0.01


def test_frames_differ():
    for k in BW.KINDS:
        fr = [BW.frame(n) for n in k.frames]
        for i in range(len(fr)):
            for j in range(i):
                assert not np.array_equal(fr[i], fr[j]), (k.name, i, j)
    short = BW.frame(BW.BY_NAME["short"].frames[0])
    for k in BW.KINDS:
        if len(k.frames) == 3:
            assert not np.array_equal(short, BW.frame(k.frames[0])), k.name
    # kinds share no frame: what one batch leaves behind is never the right answer for the next
    names = [n for k in BW.KINDS for n in k.frames]
    assert len(names) == len(set(names))
    digests = {BW.frame(n).tobytes() for n in names}
    assert len(digests) == len(names)


class _FakeContext:
    def __init__(self, log):
        self.log = log

    def set_tuning(self, **kw):
        self.log.append(("set_tuning", kw))

    def set_params(self, **kw):
        self.log.append(("set_params", kw))

    def set_mask(self, mask):
        self.log.append(("set_mask", mask))


class _FakeStream:
    def __init__(self, log):
        self.log = log

    def submit(self, frames, first_frame_id=0):
        self.log.append(("submit", frames, first_frame_id))

    def submit_device(self, ptr, pitch, fstride, n, first_frame_id=0):
        self.log.append(("submit_device", ptr, pitch, fstride, n, first_frame_id))

    def submit_compressed(self, chunks, first_frame_id=0):
        self.log.append(("submit_compressed", chunks, first_frame_id))

    def wait(self):
        self.log.append(("wait",))
        return "results"


class _FakeMemory:
    def data_ptr(self):
        return 4096


def test_walker_issues_the_calls_it_promises():
    log = []
    walker = BW.Walker(_FakeContext(log), resident=lambda ctx, frames: (_FakeMemory(), 1280, 1280 * BW.H),
                       compress=lambda img: ("chunk", img.shape))
    st = _FakeStream(log)
    K = BW.BY_NAME
    order = ["odd_params", "default", "ext1", "win52", "path2", "device_in", "compressed", "short"]
    mask_calls = []
    for step, name in enumerate(order):
        del log[:]
        assert walker.run(st, K[name], 3 * step) == "results"
        calls = [c[0] for c in log]
        with_mask = "set_mask" in calls
        mask_calls.append(with_mask)
        assert calls[:2] == ["set_tuning", "set_params"] and calls[-1] == "wait" and len(calls) == 4 + with_mask
        # every tuning key and every parameter, at its default unless the kind says otherwise: nothing survives from the batch before
        assert log[0][1] == {**BW.DEFAULT_TUNING, **K[name].tuning} and set(log[0][1]) == set(BW.DEFAULT_TUNING)
        assert log[1][1] == {**BW.DEFAULT_PARAMS, **K[name].params} and set(log[1][1]) == set(BW.DEFAULT_PARAMS)
        if with_mask:
            assert calls[2] == "set_mask" and log[2][1] is BW.masks()[K[name].mask]
        sub = log[-2]
        if K[name].form == "device":
            assert sub == ("submit_device", 4096, 1280, 1280 * BW.H, 3, 3 * step)
        elif K[name].form == "compressed":
            assert sub == ("submit_compressed", [("chunk", (BW.H, BW.W))] * 3, 3 * step)
        else:
            assert sub[0] == "submit" and sub[2] == 3 * step and sub[1].shape == (len(K[name].frames), BW.H, BW.W)
            for f, n in enumerate(K[name].frames):
                assert np.array_equal(sub[1][f], BW.frame(n))
    # set_mask: on the first batch and whenever the mask id changes (0, 0, 1, 1, 0, 0, 0, 0), never otherwise
    assert mask_calls == [True, False, True, False, True, False, False, False]
    # with batches in flight: parameters alone
    del log[:]
    walker.prepare(K["lists"], tuning=False, mask=False)
    assert [c[0] for c in log] == ["set_params"]
