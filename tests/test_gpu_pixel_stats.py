"""GPU: the per-pixel statistics over a run (ffs_ctx_set_pixel_stats / ffs_ctx_get_pixel_stats), held bit for bit to tests/pixel_stats_oracle.py.

Everything is an integer and independent of order, so every comparison is array_equal on each plane plus n_frames.  The shapes are where
the kernel can go wrong, not where the detector is: (37, 29) is a row of five lanes (32-bit pixels: ten) with a tail, (517, 41) crosses
one 512-pixel wave row with a tail, (1030, 3) several of them with fewer rows than a workgroup has waves, (8, 1) is one lane's load (32-bit:
two), (2, 2) less than one.  Lanes are numbered row by row, so in all but the last two a wave's sixty-four lanes span several rows."""
import os
import re
import subprocess

import numpy as np
import pytest

import pixel_stats_oracle as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
SHAPES = [(37, 29), (517, 41), (1030, 3), (8, 1), (2, 2)]
DTYPES = pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])


def _frames(dtype, B, H, W, seed):
    """B distinct frames: a low background, a sprinkle of bright pixels, some at the type's maximum; 32-bit: some at and above 2^24
    (as tests/test_gpu_radial.py builds them)."""
    rng = np.random.default_rng(seed)
    f = rng.poisson(3.0, (B, H, W)).astype(np.uint64)
    bright = rng.random((B, H, W)) < 0.05
    f[bright] = rng.integers(100, 60000, int(bright.sum()))
    top = rng.random((B, H, W)) < 0.02
    if np.dtype(dtype) == np.dtype(np.uint16):
        f[top] = 65535
    else:
        f[top] = rng.choice(np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 7, 0xFFFFFFFF, 1 << 20], np.uint64), int(top.sum()))
    return f.astype(dtype)


def _gappy_mask(W, H, seed):
    rng = np.random.default_rng(seed)
    m = np.ones((H, W), np.uint8)
    m[:, W // 3:W // 3 + 5] = 0
    m[H // 2:H // 2 + 3, :] = 0
    m[rng.random((H, W)) < 0.03] = 0
    return m


def _resident_padded(ctx, frames):
    """The frames in the context's pitched device layout, the row padding and the tail of every frame filled with the type's maximum."""
    import torch
    pitch, fstride = ctx.device_layout()
    B, H, W = frames.shape
    item = frames.dtype.itemsize
    host = np.full((B, fstride // item), np.iinfo(frames.dtype).max, frames.dtype)
    rows = host[:, :H * (pitch // item)].reshape(B, H, pitch // item)
    rows[:, :, :W] = frames
    assert pitch // item > W
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).to("cuda:0"), pitch, fstride


# ---- 1. shapes x pixel types, batches of 1, 3 and 5 frames over several batches
@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_batches(ffs, shape, dtype):
    W, H = shape
    frames = _frames(dtype, 18, H, W, seed=W * 31 + H)
    assert not np.array_equal(frames[0], frames[1]) or W * H < 8
    ctx = ffs.Context(W, H, dtype, max_batch=5)
    st = ctx.stream()
    ctx.set_pixel_stats("start")
    want = P.empty(H, W)
    at = 0
    for B in (1, 3, 5, 5, 3, 1):
        batch = frames[at:at + B]
        at += B
        st.process(batch)
        assert "pixel_stats" in st.last_path()[0]
        want = P.fold(want, batch)
        P.assert_equal(ctx.pixel_stats(), want, "after %d frames" % at)
    assert at == 18 and want[0] == 18
    if np.dtype(dtype) == np.dtype(np.uint32) and W * H > 100:
        assert (want[1] < 18).any()               # (values at and above 2^24 were there, and did not count)


# ---- 2. the inclusion rule: max_valid under both scopes, the mask plays no part, max is 0 where count is 0
@DTYPES
def test_inclusion_rule(ffs, dtype):
    W, H = 517, 41
    frames = _frames(dtype, 4, H, W, seed=11)
    frames[:, 7, 100:140] = 60000                # pixels that never count under max_valid = 1000
    assert (frames == 1000).sum() == 0
    frames[0, 3, 5] = frames[2, 20, 511] = frames[3, 40, 516] = 1000     # the value itself is present: p <= max_valid counts
    if np.dtype(dtype) == np.dtype(np.uint32):
        assert (frames == 1 << 24).any() and (frames == (1 << 24) - 1).any() and (frames > 1 << 24).any()
    ctx = ffs.Context(W, H, dtype, max_batch=2)
    st = ctx.stream()

    def run(max_valid):
        ctx.set_pixel_stats("start")
        for i in (0, 2):
            st.process(frames[i:i + 2])
        got = ctx.pixel_stats()
        P.assert_equal(got, P.pixel_stats(frames, max_valid), "max_valid %d" % max_valid)
        assert not got[4][got[1] == 0].any()
        return got

    unset = run(-1)
    ctx.set_mask(_gappy_mask(W, H, 3))           # a mask with holes changes nothing
    P.assert_equal(run(-1), unset, "masked")
    for scope in ("centre", "window"):
        ctx.set_max_valid_scope(scope)
        ctx.set_params(max_valid=1000)
        got = run(1000)
        assert got[1][3, 5] == 4 - int((frames[:, 3, 5] > 1000).sum()) and got[4][3, 5] == 1000
        assert not got[1][7, 100:140].any() and not got[4][7, 100:140].any() and not got[2][7, 100:140].any()
        assert not np.array_equal(got[1], unset[1])
    ctx.set_max_valid_scope("centre")
    ctx.set_params(max_valid=-1)
    P.assert_equal(run(-1), unset, "unset again")


# ---- 3. carries
def test_sum_sq_leaves_32_bits_from_the_second_frame(ffs):
    W, H = 37, 29
    ctx = ffs.Context(W, H, np.uint16, max_batch=2)
    st = ctx.stream()
    ctx.set_pixel_stats("start")
    frames = np.full((2, H, W), 65535, np.uint16)
    st.process(frames)
    n, count, s, q, mx = ctx.pixel_stats()
    assert n == 2 and (count == 2).all() and (s == 2 * 65535).all() and (q == 2 * 65535 ** 2).all() and (mx == 65535).all()
    assert 2 * 65535 ** 2 > 1 << 32
    P.assert_equal((n, count, s, q, mx), P.pixel_stats(frames))


def test_u32_sum_crosses_2_32(ffs):
    W, H = 16, 8
    top = (1 << 24) - 1
    ctx = ffs.Context(W, H, np.uint32, max_batch=32)
    st = ctx.stream()
    ctx.set_pixel_stats("start")
    frames = np.full((32, H, W), top, np.uint32)
    for _ in range(9):
        st.process(frames)
    n, count, s, q, mx = ctx.pixel_stats()
    assert 288 * top > 1 << 32
    assert n == 288 and (count == 288).all() and (s == 288 * top).all() and (q == 288 * top * top).all() and (mx == top).all()


def test_u16_sum_crosses_2_32_over_many_batches(ffs):
    """1025 batches of 64 resident frames at 65535: the 16-bit kernel's sums in memory are 64 bits (two minutes of real Eiger data)."""
    W, H = 8, 2
    ctx = ffs.Context(W, H, np.uint16, max_batch=64)
    st = ctx.stream()
    mem, pitch, fstride = _resident_padded(ctx, np.full((64, H, W), 65535, np.uint16))
    ctx.set_pixel_stats("start")
    for _ in range(1025):
        st.submit_device(mem.data_ptr(), pitch, fstride, 64)
        st.wait()
    n, count, s, q, mx = ctx.pixel_stats()
    N = 1025 * 64
    assert N * 65535 > 1 << 32
    assert n == N and (count == N).all() and (s == N * 65535).all() and (q == N * 65535 ** 2).all() and (mx == 65535).all()


# ---- 4. streams in flight together: the accumulators are the context's, the launches must not overlap
@DTYPES
@pytest.mark.parametrize("tuning", [{"sched": 3, "stats_stream": 0}, {"sched": 3, "stats_stream": 1}, {"sched": 0, "stats_stream": 0}, {"sched": 0, "stats_stream": 1},
                                    {"sched": 3, "stats_stream": 1, "dense_overlap": 1}],
                         ids=lambda t: "+".join("%s_%d" % kv for kv in t.items()))
def test_streams_in_flight_together(ffs, dtype, tuning):
    W, H = 517, 41
    ROUNDS, STREAMS, B = 4, 3, 3
    frames = _frames(dtype, ROUNDS * STREAMS * B, H, W, seed=5).reshape(ROUNDS, STREAMS, B, H, W)
    ctx = ffs.Context(W, H, dtype, max_batch=B)
    ctx.set_tuning(**tuning)
    streams = [ctx.stream() for _ in range(STREAMS)]
    ctx.set_pixel_stats("start")
    for r in range(ROUNDS):
        for k, st in enumerate(streams):
            st.submit(frames[r, k])              # all three in flight before any wait
        for st in streams:
            st.wait()
            assert "pixel_stats" in st.last_path()[0]
    P.assert_equal(ctx.pixel_stats(), P.pixel_stats(frames.reshape(-1, H, W)), str(tuning))


def test_with_the_radial_profile_on_too(ffs):
    import radial_oracle as R
    W, H = 517, 41
    frames = _frames(np.uint16, 12, H, W, seed=8).reshape(2, 3, 2, H, W)
    bins, n_bins = R.shell_bins(W, H, 9), 9
    for radial_stream in (0, 1):
        ctx = ffs.Context(W, H, np.uint16, max_batch=2)
        ctx.set_tuning(radial_stream=radial_stream)
        ctx.set_radial_bins(bins, n_bins)
        streams = [ctx.stream() for _ in range(3)]
        ctx.set_pixel_stats("start")
        for r in range(2):
            for k, st in enumerate(streams):
                st.submit(frames[r, k])
            for k, st in enumerate(streams):
                st.wait()
                path = st.last_path()[0]
                assert "pixel_stats" in path and "radial" in path
                for f in range(2):
                    for a, b in zip(st.radial_profile(f), R.radial_profile(frames[r, k, f], bins, n_bins)):
                        assert np.array_equal(a, b)
        P.assert_equal(ctx.pixel_stats(), P.pixel_stats(frames.reshape(-1, H, W)))


# ---- 5. every way in; the threshold stage does not notice
@DTYPES
def test_every_way_in(ffs, dtype):
    from ffs_amd import bslz4, byteoffset
    W, H = 517, 41
    frames = _frames(dtype, 3, H, W, seed=21)
    if np.dtype(dtype) == np.dtype(np.uint32):
        frames = np.minimum(frames, 0x7FFFFFFF).astype(dtype)   # (what a byte-offset section holds: int32)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    ctx.set_mask(_gappy_mask(W, H, 8))
    st = ctx.stream()
    ctx.set_pixel_stats("start")
    want = P.empty(H, W)
    st.submit(frames)
    st.wait()
    want = P.fold(want, frames)
    P.assert_equal(ctx.pixel_stats(), want, "ffs_submit")
    mem, pitch, fstride = _resident_padded(ctx, frames)
    st.submit_device(mem.data_ptr(), pitch, fstride, 3)
    st.wait()
    want = P.fold(want, frames)
    P.assert_equal(ctx.pixel_stats(), want, "ffs_submit_device")
    st.process_compressed([bslz4.compress(f) for f in frames[::-1]])
    want = P.fold(want, frames)
    P.assert_equal(ctx.pixel_stats(), want, "ffs_submit_compressed")
    st.process_encoded([byteoffset.compress(f) for f in frames[1:]], ffs.CODEC_BYTE_OFFSET)
    want = P.fold(want, frames[1:])
    P.assert_equal(ctx.pixel_stats(), want, "ffs_submit_encoded")
    assert "pixel_stats" in st.last_path()[0] and want[0] == 11


def test_independence_of_the_threshold_stage(ffs):
    from util import make_frame
    W, H = 530, 97
    img, mask = make_frame(W, H, np.uint16, seed=4)
    frames = np.stack([img, np.ascontiguousarray(img[::-1])])
    want = P.pixel_stats(frames)

    def run(stats, tuning=None, gain=0.0, **params):
        ctx = ffs.Context(W, H, np.uint16, max_batch=2)
        ctx.set_mask(mask)
        if tuning:
            ctx.set_tuning(**tuning)
        ctx.set_params(want_strong_list=1, **params)
        ctx.set_gain(gain)
        if stats:
            ctx.set_pixel_stats("start")
        st = ctx.stream()
        return ctx, st, st.process(frames)

    variants = {"default": {}, "kernel_half_x_5": {"kernel_half_x": 5}, "extended": {"algorithm": ffs.ALGO_DISPERSION_EXTENDED}, "gain": {"gain": 2.5},
                "grid_kernels": {"tuning": {"sparse_stage": 1}}, "in_the_dense_stream": {"tuning": {"stats_stream": 1}}}
    for name, kw in variants.items():
        ctx, st, res = run(True, **kw)
        path = st.last_path()[0]
        assert "pixel_stats" in path, name
        if name in ("kernel_half_x_5", "gain"):
            assert "window" in path, (name, path)
        if name == "extended":
            assert "extended" in path
        P.assert_equal(ctx.pixel_stats(), want, name)
        ctx0, st0, res0 = run(False, **kw)
        assert "pixel_stats" not in st0.last_path()[0]
        for a, b in zip(res, res0):
            assert a.num_strong_pixels == b.num_strong_pixels and np.array_equal(a.strong_k, b.strong_k) and np.array_equal(a.boxes, b.boxes), name
        assert sum(r.num_strong_pixels for r in res) > 0, name


# ---- 6. a batch that ffs_wait runs again counts once (the whole batch, and a frame on the one-frame stream)
def test_reruns_count_once(ffs):
    rng = np.random.default_rng(9)
    W, H = 1000, 300
    base = rng.poisson(2.0, (H, W)).astype(np.uint16)
    fat = base.copy()
    fat[100:130, 200:240] = 3000          # a block whose rim is strong: a band beyond the band plan, a frame beyond the 100 pixels the lists hold
    frames = np.stack([base, fat])
    ctx = ffs.Context(W, H, np.uint16, max_batch=2, max_strong_per_frame=100)
    ctx.set_params(min_spot_size=1)
    ctx.set_pixel_stats("start")
    st = ctx.stream()
    res = st.process(frames)
    path, reruns = st.last_path()
    assert reruns >= 1 and "pixel_stats" in path, (path, reruns)
    assert res[1].num_strong_pixels > 100      # (that frame was run again on its own as well)
    P.assert_equal(ctx.pixel_stats(), P.pixel_stats(frames))


# ---- 7. the state machine, its refusals, NULL planes, two contexts
def test_state_machine_and_refusals(ffs):
    W, H = 37, 29
    f = _frames(np.uint16, 6, H, W, seed=4)
    ctx = ffs.Context(W, H, np.uint16, max_batch=2)
    other = ffs.Context(W, H, np.uint16, max_batch=2)
    st, st_other = ctx.stream(), other.stream()
    with pytest.raises(ffs.FfsError, match="no statistics yet"):
        ctx.pixel_stats()                                    # before any start
    st.process(f[0:2])
    assert "pixel_stats" not in st.last_path()[0]
    for bad in (-1, 3, 100):
        assert ctx._lib.ffs_ctx_set_pixel_stats(ctx._h, bad) != 0
        assert b"mode must be" in ctx._lib.ffs_last_error(ctx._h)
    with pytest.raises(ValueError, match="mode must be one of"):
        ctx.set_pixel_stats("on")
    with pytest.raises(ffs.FfsError, match="no statistics yet"):
        ctx.pixel_stats()
    ctx.set_pixel_stats("resume")                            # a start, since there was none
    st.process(f[0:2])
    ctx.set_pixel_stats("off")                               # off -> the values stay
    st.process(f[2:4])
    assert "pixel_stats" not in st.last_path()[0]
    want = P.pixel_stats(f[0:2])
    P.assert_equal(ctx.pixel_stats(), want, "off keeps")
    ctx.set_pixel_stats("resume")                            # resume continues
    st.process(f[4:6])
    want = P.fold(want, f[4:6])
    P.assert_equal(ctx.pixel_stats(), want, "resume")
    # a batch submitted under on and waited after off counts; start and get are refused while it is in flight, the state unchanged
    st.submit(f[2:4])
    ctx.set_pixel_stats("off")
    with pytest.raises(ffs.FfsError, match="in flight"):
        ctx.set_pixel_stats("start")
    with pytest.raises(ffs.FfsError, match="in flight"):
        ctx.pixel_stats()
    ctx.set_pixel_stats("resume")                            # (accepted in flight: nothing is zeroed)
    ctx.set_pixel_stats("off")
    st.wait()
    assert "pixel_stats" in st.last_path()[0]
    want = P.fold(want, f[2:4])
    P.assert_equal(ctx.pixel_stats(), want, "in flight across off")
    st.process(f[0:2])                                       # off: not counted
    P.assert_equal(ctx.pixel_stats(), want, "off")
    # NULL planes: only what is asked for is copied, n_frames always
    n, count, s, q, mx = ctx.pixel_stats(planes=("max",))
    assert n == want[0] and count is None and s is None and q is None and np.array_equal(mx, want[4])
    assert ctx.pixel_stats(planes=()) == (want[0], None, None, None, None)
    assert ctx._lib.ffs_ctx_get_pixel_stats(ctx._h, None) != 0
    # two contexts are independent
    other.set_pixel_stats("start")
    st_other.process(f[4:6])
    P.assert_equal(other.pixel_stats(), P.pixel_stats(f[4:6]), "the other context")
    P.assert_equal(ctx.pixel_stats(), want, "this one")
    # start zeroes
    ctx.set_pixel_stats("start")
    P.assert_equal(ctx.pixel_stats(), P.empty(H, W), "start zeroes")
    st.process(f[0:1])
    P.assert_equal(ctx.pixel_stats(), P.pixel_stats(f[0:1]), "after the second start")
    # the placement moves only while nothing is in flight
    st.submit(f[0:2])
    with pytest.raises(ffs.FfsError, match="stats_stream"):
        ctx.set_tuning(stats_stream=1)
    st.wait()
    ctx.set_tuning(stats_stream=1)


# ---- 8. the measurement entry point
def test_bench_pixel_stats(ffs):
    from util import _resident
    W, H = 517, 41
    frames = _frames(np.uint16, 2, H, W, seed=6)
    ctx = ffs.Context(W, H, np.uint16, max_batch=2)
    st, st2 = ctx.stream(), ctx.stream()
    mem, pitch, fstride = _resident(ctx, frames)
    ms = st.bench_pixel_stats(mem.data_ptr(), pitch, fstride, 2, 3)      # (allocates the accumulators: there has been no start)
    assert 0.0 < ms < 100.0
    with pytest.raises(ffs.FfsError, match="no statistics yet"):
        ctx.pixel_stats()
    ctx.set_pixel_stats("start")
    with pytest.raises(ffs.FfsError, match="accumulation is on"):
        st.bench_pixel_stats(mem.data_ptr(), pitch, fstride, 2, 3)
    st.process(frames)
    want = P.pixel_stats(frames)
    P.assert_equal(ctx.pixel_stats(), want)
    st2.submit(frames)
    ctx.set_pixel_stats("off")
    with pytest.raises(ffs.FfsError, match="in flight"):
        st.bench_pixel_stats(mem.data_ptr(), pitch, fstride, 2, 3)
    st2.wait()
    P.assert_equal(ctx.pixel_stats(), P.fold(want, frames))              # (the refusals left the state as it was)
    assert 0.0 < st.bench_pixel_stats(mem.data_ptr(), pitch, fstride, 2, 2) < 100.0
    ctx.set_pixel_stats("start")                                         # what the measurement left is gone
    st.process(frames)
    P.assert_equal(ctx.pixel_stats(), want)


# ---- 9. the driver
def _run(argv, cwd):
    proc = subprocess.run([SPOTFINDER, *argv], cwd=cwd, capture_output=True, text=True, timeout=300)
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", proc.stdout), proc.stderr


@pytest.mark.parametrize("devices", [[], ["--devices", "0,0"]], ids=["one_context", "devices_0_0"])
def test_driver_pixel_stats(ffs, tmp_path, devices):
    from ffs_amd import synth
    N = 6          # (three batches of two images)
    argv = ["synth:tiny:%d" % N, "--threads", "1", "--batch", "2", "--max-valid", "none", *devices]
    rc, out, err = _run(argv + ["--pixel-stats", "run1"], tmp_path)
    assert rc == 0 and not err, (out, err)
    line = [l for l in out.split("\n") if l.startswith("Pixel statistics:")]
    assert line == ["Pixel statistics: %d frames -> run1.{count.u32,sum.u64,sum_sq.u64,max.u32}" % N], line
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    n, count, s, q, mx = P.pixel_stats(frames)
    for suffix, dt, want in (("count.u32", "<u4", count), ("sum.u64", "<u8", s), ("sum_sq.u64", "<u8", q), ("max.u32", "<u4", mx)):
        got = np.fromfile(tmp_path / ("run1." + suffix), dt)
        assert got.size == 300 * 200, suffix
        assert np.array_equal(got.reshape(200, 300), want), suffix
    assert sorted(os.listdir(tmp_path)) == ["run1.count.u32", "run1.max.u32", "run1.sum.u64", "run1.sum_sq.u64"]
    # without the flag: no line, no file
    rc0, out0, err0 = _run(argv, tmp_path)
    assert rc0 == 0 and not err0 and "Pixel statistics" not in out0 and len(os.listdir(tmp_path)) == 4
