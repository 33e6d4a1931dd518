"""GPU: dark frames of raw Jungfrau words folded into per-pixel, per-stage accumulators on the device (ffs_stream_jungfrau_pedestal_fold,
csrc/kernels_jfped.hpp) against the NumPy / integer truth (tests/jungfrau_pedestal_oracle.py), everything compared with !=, no tolerance:
shapes on both sides of every path of the kernel, batch sizes and chunk placements, which stages a lane sees, sums beyond 32 bits inside a
launch, more frames than a launch carries, two streams on two threads, lifetime and refusals, independence from the batches around a fold,
and the loop closed: measured pedestals into a calibration into a conversion.

Not reachable here: the refusal at 2^32 - 1 frames (its arithmetic is held by tests/test_jungfrau_pedestal_oracle.py::test_frame_limit), and
begin / get / end while a FOLD is in flight -- a fold is synchronous, so only another thread could be inside one, and whether it is at the
moment of the call is not the test's to decide; the refusal reads the same in-flight count a submitted batch raises, which is tested."""
import ctypes as C
import threading

import numpy as np
import pytest

import jungfrau_oracle as J
import jungfrau_pedestal_oracle as P
from ffs_amd import synth
from ffs_amd.api import CODEC_JUNGFRAU_RAW

pytestmark = pytest.mark.gpu

MAX_BATCH = 4
TOP = (1 << 24) - 1
# W * H below one group of eight, groups that straddle rows, a frame that is no multiple of 8, both sides of a workgroup's 2048 pixels
SHAPES = [(1, 1), (7, 3), (67, 9), (300, 200), (2040, 3), (2048, 3), (2049, 3)]


def assert_acc(ctx, acc, what=""):
    n, count, total, total_sq = ctx.jungfrau_pedestal()
    assert n == acc[0], (what, n, acc[0])
    for name, got, want in (("count", count, acc[1]), ("sum", total, acc[2]), ("sum_sq", total_sq, acc[3])):
        assert got.dtype == want.dtype and got.shape == want.shape
        d = np.argwhere(got != want)
        assert d.size == 0, f"{what}: {name}: {len(d)} entries differ, first at {d[:4].tolist()}: got {got[tuple(d[0])]} want {want[tuple(d[0])]}"


def in_place(st, frames, order=None):
    """The frames copied into the stream's host buffer at 16-aligned offsets with gaps, not in order; views in the frames' order."""
    hb = st.host_bytes()
    size = frames[0].size * 2
    slot = (size + 15) // 16 * 16
    order = list(range(len(frames)))[::-1] if order is None else order
    views = [None] * len(frames)
    at = 48
    for j, i in enumerate(order):
        assert at % 16 == 0 and at + size <= hb.size
        hb[at:at + size] = np.frombuffer(frames[i].tobytes(), np.uint8)
        views[i] = hb[at:at + size]
        at += slot + 16 * (1 + j % 3)
    return views


@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_folds_equal_the_oracle_over_shapes_batches_and_placements(ffs, W, H):
    raw = np.concatenate([P.stage_mix_frames(MAX_BATCH, H, W, seed=W * 7 + H), P.uniform_frames(MAX_BATCH, H, W, 1, seed=W + H)])
    ctx = ffs.Context(W, H, np.uint32, max_batch=MAX_BATCH)
    st = ctx.stream()
    ctx.jungfrau_pedestal_begin()
    acc = P.zeros(H, W)
    assert_acc(ctx, acc, "after begin")
    for n in (1, 2, MAX_BATCH):
        st.jungfrau_pedestal_fold(list(raw[:n]))
        assert_acc(ctx, P.fold(acc, raw[:n]), f"{n} frames, arrays")
        st.jungfrau_pedestal_fold([f.tobytes() for f in raw[len(raw) - n:]])
        assert_acc(ctx, P.fold(acc, raw[len(raw) - n:]), f"{n} frames, bytes")
        st.jungfrau_pedestal_fold(in_place(st, raw[1:1 + n]))
        assert_acc(ctx, P.fold(acc, raw[1:1 + n]), f"{n} frames, in place")
    if W * H >= 8:
        assert (acc[1] > 0).any(axis=(1, 2)).all() and (acc[1].sum(axis=0) < acc[0]).any()
    ms = st.jungfrau_pedestal_fold(list(raw[:2]), want_ms=True)
    assert ms > 0
    assert_acc(ctx, P.fold(acc, raw[:2]), "with want_ms")


@pytest.mark.parametrize("W,H", [(67, 9), (300, 200)], ids=lambda v: str(v))
def test_stage_presence(ffs, W, H):
    ctx = ffs.Context(W, H, np.uint32, max_batch=MAX_BATCH)
    st = ctx.stream()
    ctx.jungfrau_pedestal_begin()
    acc = P.zeros(H, W)
    # batches wholly in one stage: the other two are neither loaded nor stored
    for code in (0, 1, 3, 1, 0):
        fr = P.uniform_frames(3, H, W, code, seed=code + W)
        st.jungfrau_pedestal_fold(list(fr))
        assert_acc(ctx, P.fold(acc, fr), f"all of gain code {code}")
    # all four gain codes within one lane's eight pixels
    fr = P.stage_mix_frames(MAX_BATCH, H, W, seed=3)
    assert {0, 1, 2, 3} <= set((fr[0].reshape(-1)[:8] >> 14).tolist())
    st.jungfrau_pedestal_fold(list(fr))
    assert_acc(ctx, P.fold(acc, fr), "all gain codes in a lane")
    # lanes with no word of a stage beside lanes with some; a lane whose only words of the batch are invalid
    fr = P.uniform_frames(MAX_BATCH, H, W, 0, seed=5).reshape(MAX_BATCH, -1)
    fr[:, 8 * 3:8 * 4] |= 0x4000                     # lane 3: G1 in every pixel
    fr[1, 8 * 10 + 2] = 0xC000 | 77                  # lane 10: one G2 word in one frame
    fr[:, 8 * 5:8 * 6] = [0xFFFF, 0xC000, 0x8000, 0xBFFF, 0xFFFF, 0x8123, 0xC000, 0xFFFF]   # lane 5: nothing counts
    fr[:, 8 * 6] = 0xFFFF                            # lane 6: one pixel never counts
    fr = fr.reshape(MAX_BATCH, H, W)
    before = [a.copy() if isinstance(a, np.ndarray) else a for a in acc]
    st.jungfrau_pedestal_fold(list(fr))
    assert_acc(ctx, P.fold(acc, fr), "lanes that differ in their stages")
    flat = [(a - b).reshape(3, -1) for a, b in zip(acc[1:], before[1:])]
    assert not flat[0][:, 40:48].any() and flat[0][1, 24:32].all() and not flat[0][0, 24:32].any() and flat[0][2].sum() == 1


def test_sums_beyond_32_bits_inside_a_launch(ffs):
    W, H = 67, 9
    ctx = ffs.Context(W, H, np.uint32, max_batch=64)
    st = ctx.stream()
    ctx.jungfrau_pedestal_begin()
    acc = P.zeros(H, W)
    for n in (17, 64):
        fr = np.full((n, H, W), 0x3FFF, np.uint16)
        st.jungfrau_pedestal_fold(list(fr))
        assert_acc(ctx, P.fold(acc, fr), f"{n} frames of 0x3FFF")
    assert int(acc[3][0, 0, 0]) == 81 * 16383 ** 2 and 64 * 16383 ** 2 > 1 << 32
    fr = np.full((64, H, W), 0x7FFF, np.uint16)      # ... and in G1, beside the G0 sums that stay
    st.jungfrau_pedestal_fold(list(fr))
    assert_acc(ctx, P.fold(acc, fr), "64 frames of 0x7FFF")


def test_more_frames_than_one_launch_carries(ffs):
    W, H = 67, 9
    ctx = ffs.Context(W, H, np.uint32, max_batch=70)
    st = ctx.stream()
    ctx.jungfrau_pedestal_begin()
    fr = P.stage_mix_frames(70, H, W, seed=70)
    st.jungfrau_pedestal_fold(list(fr))
    acc = P.fold(P.zeros(H, W), fr)
    assert_acc(ctx, acc, "70 frames")
    st.jungfrau_pedestal_fold(in_place(st, fr[:65]))
    assert_acc(ctx, P.fold(acc, fr[:65]), "65 frames in place")


def test_two_streams_on_two_threads(ffs):
    W, H = 300, 200
    ctx = ffs.Context(W, H, np.uint32, max_batch=MAX_BATCH)
    streams = [ctx.stream(), ctx.stream()]
    ctx.jungfrau_pedestal_begin()
    frames = [np.concatenate([P.stage_mix_frames(6, H, W, seed=20 + t), P.uniform_frames(6, H, W, (0, 3)[t], seed=30 + t)]) for t in range(2)]
    errors = []
    barrier = threading.Barrier(2)

    def work(t):
        try:
            barrier.wait()
            for i in range(3):
                streams[t].jungfrau_pedestal_fold(list(frames[t][4 * i:4 * i + 4]))
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    acc = P.fold(P.fold(P.zeros(H, W), frames[0]), frames[1])
    assert_acc(ctx, acc, "three folds on each of two threads")


def _photon_case(n=2, seed=7):
    W, H = 300, 200
    p = synth.params(W, H, np.uint32, seed=seed, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=TOP)
    photons = synth.frames(p, range(n), threads=2)
    ped, fac = J.calibration(W, H, seed=seed)
    raw = J.encode(photons, ped, fac, seed=seed)
    return raw, ped, fac, J.convert(raw, ped, fac)


def test_lifetime_and_refusals(ffs):
    W, H = 300, 200
    fr = P.stage_mix_frames(MAX_BATCH, H, W, seed=1)
    ctx = ffs.Context(W, H, np.uint32, max_batch=MAX_BATCH)
    st = ctx.stream()
    lib = ffs.load_library()

    def refused(call, match):
        with pytest.raises(ffs.FfsError, match=match):
            call()

    # before begin
    refused(lambda: st.jungfrau_pedestal_fold(list(fr)), "no accumulators")
    refused(ctx.jungfrau_pedestal, "no accumulators")
    ctx.jungfrau_pedestal_end()                       # idempotent
    ctx.jungfrau_pedestal_begin()
    st.jungfrau_pedestal_fold(list(fr))
    acc = P.fold(P.zeros(H, W), fr)
    assert_acc(ctx, acc)
    n, count, total, total_sq = ctx.jungfrau_pedestal(planes=("sum",))
    assert n == MAX_BATCH and count is None and total_sq is None and np.array_equal(total, acc[2])

    def unchanged():
        assert_acc(ctx, acc, "after a refusal")

    # n_frames outside 1..max_batch
    refused(lambda: st.jungfrau_pedestal_fold([]), "1..max_batch")
    refused(lambda: st.jungfrau_pedestal_fold(list(fr) + [fr[0]]), "1..max_batch")
    # a chunk of any other size
    for bad in (fr[0].tobytes()[:-2], fr[0].tobytes() + b"\0\0", b"", fr[0].astype(np.uint32)):
        refused(lambda: st.jungfrau_pedestal_fold([fr[1], bad]), "is not a dark frame of 60000 16-bit words")
    # a misaligned chunk in the host buffer; chunks half in it
    hb = st.host_bytes()
    size = W * H * 2
    views = []
    for i, at in enumerate((32, 32 + size + 8)):
        hb[at:at + size] = np.frombuffer(fr[i].tobytes(), np.uint8)
        views.append(hb[at:at + size])
    refused(lambda: st.jungfrau_pedestal_fold(views), "ffs_stream_jungfrau_pedestal_fold: raw Jungfrau chunk 1 .* multiple of 16")
    refused(lambda: st.jungfrau_pedestal_fold([views[0], fr[1]]), "either all chunks")
    # NULL where it is not allowed
    ptrs, sizes = (C.c_void_p * 1)(fr[0].ctypes.data), (C.c_size_t * 1)(size)
    assert lib.ffs_stream_jungfrau_pedestal_fold(st._h, None, sizes, 1, None) != 0 and "NULL" in lib.ffs_last_error(ctx._h).decode()
    assert lib.ffs_stream_jungfrau_pedestal_fold(st._h, ptrs, None, 1, None) != 0
    assert lib.ffs_stream_jungfrau_pedestal_fold(None, ptrs, sizes, 1, None) != 0
    null_chunk = (C.c_void_p * 1)(None)
    assert lib.ffs_stream_jungfrau_pedestal_fold(st._h, null_chunk, sizes, 1, None) != 0 and "(NULL)" in lib.ffs_last_error(ctx._h).decode()
    assert lib.ffs_ctx_get_jungfrau_pedestal(ctx._h, None) != 0 and "out is NULL" in lib.ffs_last_error(ctx._h).decode()
    assert lib.ffs_ctx_jungfrau_pedestal_begin(None) != 0 and lib.ffs_ctx_jungfrau_pedestal_end(None) != 0
    unchanged()
    # while a batch of the context is in flight: fold on its stream, begin, get, end (on any stream's batch)
    raw, ped, fac, want = _photon_case()
    ctx.set_params(max_valid=TOP)
    other = ctx.stream()
    for busy in (st, other):
        busy.submit(want)
        if busy is st:
            refused(lambda: st.jungfrau_pedestal_fold(list(fr)), "batch in flight")
        refused(ctx.jungfrau_pedestal_begin, "in flight")
        refused(ctx.jungfrau_pedestal, "in flight")
        refused(ctx.jungfrau_pedestal_end, "in flight")
        assert len(busy.wait()) == 2
        unchanged()
    # the host function's arguments
    for bad, match in ((dict(min_frames=0), "min_frames"), (dict(max_rms=-0.5), "max_rms"), (dict(max_rms=float("inf")), "max_rms"), (dict(max_rms=float("nan")), "max_rms")):
        refused(lambda: ffs.jungfrau_pedestal_planes(acc, **bad), match)
    # begin zeroes; end, then get and fold are refused; begin again works
    ctx.jungfrau_pedestal_begin()
    assert_acc(ctx, P.zeros(H, W), "begin zeroes")
    st.jungfrau_pedestal_fold(list(fr[:1]))
    ctx.jungfrau_pedestal_end()
    refused(ctx.jungfrau_pedestal, "no accumulators")
    refused(lambda: st.jungfrau_pedestal_fold(list(fr)), "no accumulators")
    ctx.jungfrau_pedestal_end()
    ctx.jungfrau_pedestal_begin()
    st.jungfrau_pedestal_fold(list(fr[2:]))
    assert_acc(ctx, P.fold(P.zeros(H, W), fr[2:]), "begin again")
    # a 2-byte context
    ctx16 = ffs.Context(W, H, np.uint16, max_batch=2)
    refused(ctx16.jungfrau_pedestal_begin, "pixel_bytes 4")
    refused(lambda: ctx16.stream().jungfrau_pedestal_fold(list(fr[:1])), "no accumulators")


def _results_key(res):
    return [(r.frame_id, r.num_strong_pixels, r.n_components, r.boxes.tobytes(), r.reflections.tobytes()) for r in res]


def test_a_fold_is_independent_of_the_batches_around_it(ffs):
    W, H = 300, 200
    raw, ped, fac, want = _photon_case(seed=11)
    yy, xx = np.mgrid[0:H, 0:W]
    bins = np.minimum(np.hypot(xx - 140.0, yy - 90.0) / 12, 15).astype(np.uint16)
    dark = synth.dark_frames(W, H, 11, 6)

    def context():
        ctx = ffs.Context(W, H, np.uint32, max_batch=MAX_BATCH)
        ctx.set_params(max_valid=TOP, want_reflections=1)
        ctx.set_radial_bins(bins, 16)
        return ctx

    def data_batch(ctx, st):
        ctx.set_pixel_stats("start")
        res = st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW, first_frame_id=3)
        return (_results_key(res), [tuple(a.tobytes() for a in st.radial_profile(i)) for i in range(len(raw))],
                tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in ctx.pixel_stats()), st.last_path(), st.spot_backgrounds().tobytes())

    # what the batch gives without any fold
    ref_ctx = context()
    ref_ctx.set_jungfrau_calibration(ped, fac)
    ref = data_batch(ref_ctx, ref_ctx.stream())
    assert sum(len(k[3]) for k in ref[0]) > 0 and "pixel_stats" in ref[3][0] and "radial" in ref[3][0]
    # a fold works on a context with no calibration
    ctx = context()
    st = ctx.stream()
    ctx.jungfrau_pedestal_begin()
    st.jungfrau_pedestal_fold(list(dark[:3]))
    acc = P.fold(P.zeros(H, W), dark[:3])
    assert_acc(ctx, acc, "no calibration")
    with pytest.raises(ffs.FfsError, match="calibration"):
        st.submit_encoded(list(raw), CODEC_JUNGFRAU_RAW)
    # the batch between two folds on the same stream
    ctx.set_jungfrau_calibration(ped, fac)
    got = data_batch(ctx, st)
    for a, b, what in zip(got, ref, ("results", "radial profile", "pixel statistics", "last path", "spot backgrounds")):
        assert a == b, what
    st.jungfrau_pedestal_fold(in_place(st, dark[3:]))
    assert_acc(ctx, P.fold(acc, dark[3:]), "the second fold")
    # ... which left the stream's last batch as it was: the header says ffs_stream_spot_backgrounds remains available after a fold
    assert st.last_path() == ref[3]
    assert st.spot_backgrounds().tobytes() == ref[4]
    assert tuple(a.tobytes() for a in st.radial_profile(1)) == ref[1][1]
    assert tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in ctx.pixel_stats()) == ref[2]
    assert _results_key(st.process_encoded(list(raw), CODEC_JUNGFRAU_RAW, first_frame_id=3)) == ref[0]


def test_closing_the_loop(ffs):
    W, H, seed, n = 300, 200, 7, 24
    old_ped, fac = synth.jungfrau_calibration(W, H, seed)
    true_ped = (old_ped + np.float32(37.5)).astype(np.float32)           # the pedestals have drifted since the old calibration
    dark = np.stack([synth.jungfrau_dark(W, H, true_ped, seed, i, n) for i in range(n)])
    ctx = ffs.Context(W, H, np.uint32, max_batch=8)
    st = ctx.stream()
    ctx.jungfrau_pedestal_begin()
    for i in range(0, n, 8):
        st.jungfrau_pedestal_fold(list(dark[i:i + 8]))
    stats = ctx.jungfrau_pedestal()
    ctx.jungfrau_pedestal_end()
    acc = P.fold(P.zeros(H, W), dark)
    ped, rms, ok = ffs.jungfrau_pedestal_planes(stats, min_frames=4, max_rms=2.5)
    want_ped, want_rms, want_ok = P.planes(*acc[1:], min_frames=4, max_rms=2.5)
    assert np.array_equal(ped.view(np.uint32), want_ped.view(np.uint32)) and np.array_equal(rms.view(np.uint32), want_rms.view(np.uint32))
    assert np.array_equal(ok, want_ok) and 0.99 < ok.mean() < 1
    new_ped, new_fac = P.repedestal(old_ped, fac, want_ped, want_ok)
    ctx.set_jungfrau_calibration(P.repedestal(old_ped, fac, ped, ok)[0], P.repedestal(old_ped, fac, ped, ok)[1])
    raw = synth.raw_frames(synth.tiny_params(seed, np.uint32), range(2))
    _, got = st.decode_only(list(raw), codec=CODEC_JUNGFRAU_RAW)
    want = J.convert(raw, new_ped, new_fac)
    d = np.argwhere(got != want)
    assert d.size == 0, f"{len(d)} pixels differ, first at {d[:4].tolist()}"
    # the stuck pixels have no G1 / G2 pedestal: a word of theirs in those stages is invalid now
    assert ((new_fac == 0) & (fac != 0)).any() and (want == J.INVALID).any()
