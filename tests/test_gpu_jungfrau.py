"""GPU: raw Jungfrau words converted on the device (FFS_CODEC_JUNGFRAU_RAW, csrc/kernels_jungfrau.hpp) against the NumPy float32 truth
(tests/jungfrau_oracle.py), bit for bit: decode alone over widths on both sides of every path of the kernel, batch sizes and chunk
placements; the pipeline from raw words against the pipeline from the converted frames, with the radial profile and the pixel statistics;
one stream through a sequence of input kinds with the calibration replaced in between; every refusal of the ABI."""
import numpy as np
import pytest

import jungfrau_oracle as J
from ffs_amd import bslz4, synth
from ffs_amd.api import CODEC_BSLZ4, CODEC_JUNGFRAU_RAW

pytestmark = pytest.mark.gpu

MAX_BATCH = 4
TOP = (1 << 24) - 1
# 1x1, widths unrelated to the group of eight (a group straddles rows), a width of whole groups; then one group short of, equal to and one
# pixel beyond the 2048 pixels a workgroup covers in a row
SHAPES = [(1, 1), (7, 3), (67, 9), (200, 100), (2040, 3), (2048, 3), (2049, 3)]


def assert_same(got, want, what=""):
    d = np.argwhere(got != want)
    assert d.size == 0, f"{what}: {len(d)} pixels differ, first at {d[:4].tolist()}: got {got[tuple(d[0])]} want {want[tuple(d[0])]}"


@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_decode_only_equals_the_oracle(ffs, W, H):
    ped, fac = J.calibration(W, H, seed=W + H)
    fac[np.random.default_rng(W).random(fac.shape) < 0.02] = 4096.0      # (results beyond the clamp)
    raw = J.stage_mix_frames(MAX_BATCH, H, W, ped, fac, seed=W * 7 + H, all_g0=(2,))
    want = J.convert(raw, ped, fac)
    if W * H >= 8:
        assert (raw[2] >> 14 == 0).all() and {0, 1, 2, 3} <= set(np.unique(raw[0].reshape(-1)[:8] >> 14).tolist())
        assert (want == J.INVALID).any() and ((want > 0) & (want < TOP)).any()
    ctx = ffs.Context(W, H, np.uint32, max_batch=MAX_BATCH)
    ctx.set_jungfrau_calibration(ped, fac)
    st = ctx.stream()
    for n in (1, 2, MAX_BATCH):
        # outside the host buffer: uint16 arrays, and bytes
        _, got = st.decode_only(list(raw[:n]), codec=CODEC_JUNGFRAU_RAW)
        assert got.dtype == np.uint32
        assert_same(got, want[:n], f"{n} frames, arrays")
        _, got = st.decode_only([f.tobytes() for f in raw[MAX_BATCH - n:]], codec=CODEC_JUNGFRAU_RAW)
        assert_same(got, want[MAX_BATCH - n:], f"{n} frames, bytes")
        # inside it, at 16-aligned offsets with gaps, not in order
        hb = st.host_bytes()
        size = W * H * 2
        slot = (size + 15) // 16 * 16
        order = list(range(n))[::-1]
        views = [None] * n
        at = 48
        for j, i in enumerate(order):
            assert at % 16 == 0 and at + size <= hb.size
            hb[at:at + size] = np.frombuffer(raw[i].tobytes(), np.uint8)
            views[i] = hb[at:at + size]
            at += slot + 16 * (1 + j % 3)
        _, got = st.decode_only(views, codec=CODEC_JUNGFRAU_RAW)
        assert_same(got, want[:n], f"{n} frames, in place")


def _photon_frames(n, seed=7):
    p = synth.params(300, 200, np.uint32, seed=seed, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=TOP)
    return synth.frames(p, range(n), threads=2)


def _raw_case(n=MAX_BATCH, seed=7):
    """Raw frames of spots on a background, their calibration and what they convert to; an invalid word inside a spot's window and another
    on a spot's peak, in every frame."""
    W, H = 300, 200
    photons = _photon_frames(n, seed)
    ped, fac = J.calibration(W, H, seed=seed)
    raw = J.encode(photons, ped, fac, seed=seed)
    for f in range(n):
        inner = photons[f, 6:H - 6, 6:W - 6]
        y0, x0 = np.unravel_index(np.argmax(inner), inner.shape)
        raw[f, y0 + 6, x0 + 6] = 0xC000      # the peak of the frame's brightest spot
        far = np.argwhere((inner > 300) & (np.hypot(*np.mgrid[0:inner.shape[0], 0:inner.shape[1]]
                                                     - np.array([y0, x0])[:, None, None]) > 20))
        assert len(far) >= 1
        y1, x1 = far[0]
        raw[f, y1 + 6 + 2, x1 + 6 + 1] = 0xFFFF   # inside the window of another spot's bright pixel
    want = J.convert(raw, ped, fac)
    assert (want == J.INVALID).sum() >= 2 * n
    return raw, ped, fac, want


def assert_results_equal(a, b, what=""):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for f in ("frame_id", "num_strong_pixels", "num_strong_pixels_filtered", "n_components", "n_filtered_size", "n_filtered_sep"):
            assert getattr(ra, f) == getattr(rb, f), (what, f)
        assert ra.boxes.tobytes() == rb.boxes.tobytes(), what
        assert ra.reflections.tobytes() == rb.reflections.tobytes(), what
        if ra.strong_k is not None:
            np.testing.assert_array_equal(ra.strong_k, rb.strong_k, err_msg=what)
            np.testing.assert_array_equal(ra.strong_intensity, rb.strong_intensity, err_msg=what)


def _context(ffs, ped, fac, **params):
    ctx = ffs.Context(300, 200, np.uint32, max_batch=MAX_BATCH)
    ctx.set_params(max_valid=TOP, want_strong_list=1, **params)
    ctx.set_jungfrau_calibration(ped, fac)
    return ctx


def test_pipeline_from_raw_words_equals_pipeline_from_converted_frames(ffs):
    raw, ped, fac, want = _raw_case()
    ctx = _context(ffs, ped, fac)
    st = ctx.stream()
    res = st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW, first_frame_id=5)
    ref = st.process(want, first_frame_id=5)
    assert sum(len(r.boxes) for r in ref) > 40 and [r.frame_id for r in res] == [5, 6, 7, 8]
    assert_results_equal(res, ref)
    # no invalid pixel is strong, and the calibration outlives set_params
    for r in res:
        assert (r.strong_intensity <= TOP).all()
    ctx.set_params(threshold=1.0)
    assert_results_equal(st.process_encoded(list(raw[:2]), CODEC_JUNGFRAU_RAW), st.process(want[:2]), "after set_params")


def test_pipeline_with_a_radial_bin_map(ffs):
    raw, ped, fac, want = _raw_case(seed=11)
    ctx = _context(ffs, ped, fac)
    yy, xx = np.mgrid[0:200, 0:300]
    bins = np.minimum(np.hypot(xx - 140.0, yy - 90.0) / 12, 15).astype(np.uint16)
    ctx.set_radial_bins(bins, 16)
    st = ctx.stream()
    res = st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW)
    prof = [st.radial_profile(i) for i in range(len(raw))]
    ref = st.process(want)
    assert_results_equal(res, ref)
    for i in range(len(raw)):
        for a, b in zip(prof[i], st.radial_profile(i)):
            np.testing.assert_array_equal(a, b)
        # ... and the invalid pixels are in no bin's count
        valid = want[i] <= TOP
        np.testing.assert_array_equal(prof[i][0], np.bincount(bins[valid], minlength=16))


def test_pipeline_with_pixel_statistics(ffs):
    raw, ped, fac, want = _raw_case(seed=13)
    ctx = _context(ffs, ped, fac)
    st = ctx.stream()
    ctx.set_pixel_stats("start")
    res = st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW)
    got = ctx.pixel_stats()
    ctx.set_pixel_stats("start")
    ref = st.process(want)
    exp = ctx.pixel_stats()
    assert_results_equal(res, ref)
    assert got[0] == exp[0] == len(raw)
    for a, b in zip(got[1:], exp[1:]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got[1], (want <= TOP).sum(axis=0))


def test_one_stream_through_a_sequence_of_inputs(ffs):
    raw, ped, fac, want = _raw_case(seed=17)
    ctx = _context(ffs, ped, fac)
    st = ctx.stream()
    fresh = _context(ffs, ped, fac).stream()
    ref = fresh.process(want)
    plain = _photon_frames(MAX_BATCH, seed=23)
    ref_plain = fresh.process(plain)
    # pedestals drift: a second calibration, and what the same words are under it
    ped2 = (ped + np.float32(400.25)).astype(np.float32)
    fac2 = fac.copy()
    fac2[0, 50:60, 50:60] = 0.0
    want2 = J.convert(raw, ped2, fac2)
    assert (want2 != want).mean() > 0.05
    ref2 = fresh.process(want2)
    assert_results_equal(st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW), ref, "raw words")
    assert_results_equal(st.process_encoded([bslz4.compress(f) for f in plain], CODEC_BSLZ4), ref_plain, "bitshuffle-LZ4")
    assert_results_equal(st.process(plain), ref_plain, "plain submit")
    ctx.set_jungfrau_calibration(ped2, fac2)
    assert_results_equal(st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW), ref2, "raw words, second calibration")
    _, got = st.decode_only(list(raw), codec=CODEC_JUNGFRAU_RAW)
    assert_same(got, want2, "decode alone, second calibration")
    ctx.set_jungfrau_calibration(ped, fac)
    assert_results_equal(st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW), ref, "raw words, first calibration again")


def test_refusals_leave_the_state_unchanged(ffs):
    W, H = 300, 200
    raw, ped, fac, want = _raw_case(n=2, seed=19)
    ctx = _context(ffs, ped, fac)
    st = ctx.stream()
    ref = st.process(want)

    def still_works():
        _, got = st.decode_only(list(raw), codec=CODEC_JUNGFRAU_RAW)
        assert_same(got, want, "after a refusal")
        assert_results_equal(st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW), ref, "after a refusal")

    still_works()
    # any other chunk size
    for bad in (raw[0].tobytes()[:-2], raw[0].tobytes() + b"\0\0", b"", want[0].tobytes()):
        for call in (lambda: st.submit_encoded([raw[1], bad], CODEC_JUNGFRAU_RAW), lambda: st.decode_only([bad], codec=CODEC_JUNGFRAU_RAW)):
            with pytest.raises(ffs.FfsError, match="raw Jungfrau chunk of"):
                call()
    still_works()
    # in the host buffer at an offset that is no multiple of 16
    hb = st.host_bytes()
    size = W * H * 2
    views = []
    for i, at in enumerate((32, 32 + size + 8)):
        hb[at:at + size] = np.frombuffer(raw[i].tobytes(), np.uint8)
        views.append(hb[at:at + size])
    assert (32 + size + 8) % 16 == 8
    for call in (lambda: st.submit_encoded(views, CODEC_JUNGFRAU_RAW), lambda: st.decode_only(views, codec=CODEC_JUNGFRAU_RAW)):
        with pytest.raises(ffs.FfsError, match="multiple of 16"):
            call()
    still_works()
    # codec 7 stays unknown
    with pytest.raises(ffs.FfsError, match="codec"):
        st.submit_encoded(list(raw), 7)
    # the calibration cannot change under a batch
    st.submit_encoded(list(raw), CODEC_JUNGFRAU_RAW)
    with pytest.raises(ffs.FfsError, match="in flight"):
        ctx.set_jungfrau_calibration(ped + np.float32(100), fac)
    with pytest.raises(ffs.FfsError, match="in flight"):
        ctx.set_jungfrau_calibration(None)
    assert_results_equal(st.wait(), ref, "the batch in flight")
    still_works()
    # entries outside the ranges: the text names the plane and the index
    for plane, s, value, name in ((ped, 1, 65537.0, r"pedestal\[1\]"), (ped, 0, np.nan, r"pedestal\[0\]"), (fac, 2, 1e-10, r"factor\[2\]"),
                                  (fac, 0, 70000.0, r"factor\[0\]"), (fac, 1, -np.inf, r"factor\[1\]")):
        bad = plane.copy()
        bad[s, 7, 13] = value
        with pytest.raises(ffs.FfsError, match=name + r" entry 2113 \(x = 13, y = 7\)"):
            ctx.set_jungfrau_calibration(bad if plane is ped else ped, bad if plane is fac else fac)
        still_works()
    with pytest.raises(ValueError):
        ctx.set_jungfrau_calibration(ped[:2], fac[:2])
    # no calibration on the context
    ctx.set_jungfrau_calibration(None)
    for call in (lambda: st.submit_encoded(list(raw), CODEC_JUNGFRAU_RAW), lambda: st.decode_only(list(raw), codec=CODEC_JUNGFRAU_RAW)):
        with pytest.raises(ffs.FfsError, match="calibration"):
            call()
    assert_results_equal(st.process(want), ref, "plain submit without a calibration")
    ctx.set_jungfrau_calibration(ped, fac)
    still_works()
    # a 2-byte context takes neither the calibration nor the codec
    ctx16 = ffs.Context(W, H, np.uint16, max_batch=2)
    with pytest.raises(ffs.FfsError, match="pixel_bytes 4"):
        ctx16.set_jungfrau_calibration(ped, fac)
    st16 = ctx16.stream()
    for call in (lambda: st16.submit_encoded(list(raw), CODEC_JUNGFRAU_RAW), lambda: st16.decode_only(list(raw), codec=CODEC_JUNGFRAU_RAW)):
        with pytest.raises(ffs.FfsError, match="pixel_bytes 4"):
            call()
    photons16 = np.minimum(_photon_frames(2, seed=19), 65535).astype(np.uint16)
    assert len(st16.process(photons16)) == 2
