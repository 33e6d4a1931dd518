"""GPU: the per-frame radial profile (ffs_ctx_set_radial_bins / ffs_stream_radial_profile), held bit for bit to tests/radial_oracle.py.

The sums are integers and independent of order, so every comparison is array_equal on uint32 / uint64.  The shapes are where the
kernel can go wrong, not where the detector is: (517, 41) crosses one 512-pixel wave row with a tail, (1030, 3) three of them (32-bit
pixels: five loads a row) with fewer rows than a workgroup has waves, (8, 1) is one lane's load, (2, 2) less than that."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import radial_oracle as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
HOST = os.path.join(ROOT, "fast-feedback-service_amd", "host")
NO_BIN = R.NO_BIN
SHAPES = [(37, 29), (517, 41), (1030, 3), (8, 1), (2, 2)]


def _frames(dtype, B, H, W, seed):
    """B distinct frames: a low background, a sprinkle of bright pixels, some at the type's maximum; 32-bit: some at and above 2^24."""
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


def _maps(W, H, seed):
    """name -> (bin map, n_bins, frames are all 65535)."""
    rng = np.random.default_rng(seed)
    every_second = R.shell_bins(W, H, 5).copy()
    every_second.reshape(-1)[1::2] = NO_BIN
    ends = np.where(rng.random((H, W)) < 0.5, 0, 1023).astype(np.uint16)
    return {
        "shells": (R.shell_bins(W, H, 16, cx=W * 0.4, cy=H * 0.6), 16, False),
        "random": (rng.integers(0, 40, (H, W)).astype(np.uint16), 40, False),
        "constant_65535": (np.full((H, W), 1, np.uint16), 3, True),
        "one_bin": (np.zeros((H, W), np.uint16), 1, False),
        "bins_1024": (rng.integers(0, 1024, (H, W)).astype(np.uint16), 1024, False),
        "every_second_none": (every_second, 5, False),
        "all_none": (np.full((H, W), NO_BIN, np.uint16), 4, False),
        "only_0_and_1023": (ends, 1024, False),
    }


def _check(st, frames, bins, n_bins, mask=None, max_valid=-1):
    for f, img in enumerate(frames):
        count, s, q = st.radial_profile(f)
        wc, ws, wq = R.radial_profile(img, bins, n_bins, mask, max_valid)
        assert count.dtype == np.uint32 and s.dtype == np.uint64 and q.dtype == np.uint64 and len(count) == len(s) == len(q) == n_bins
        assert np.array_equal(count, wc), (f, count, wc)
        assert np.array_equal(s, ws), (f, s, ws)
        assert np.array_equal(q, wq), (f, q, wq)


# ---- 1. shapes x pixel types x batches of 1 and 3 x bin maps
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_maps(ffs, shape, dtype):
    W, H = shape
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    st = ctx.stream()
    frames = _frames(dtype, 3, H, W, seed=W * 31 + H)
    assert not np.array_equal(frames[0], frames[1]) or W * H < 8
    for name, (bins, n_bins, saturated) in _maps(W, H, seed=5).items():
        ctx.set_radial_bins(bins, n_bins)
        for B in (1, 3):
            batch = np.full((B, H, W), 65535, dtype) if saturated else frames[:B]
            st.process(batch)
            assert "radial" in st.last_path()[0], name
            _check(st, batch, bins, n_bins)
            if name == "all_none":
                assert all(not a.any() for a in st.radial_profile(0))
            if saturated:   # one bin takes every pixel: sum_sq carries out of 32 bits from the second pixel on
                count, s, q = st.radial_profile(B - 1)
                assert count[1] == W * H and int(q[1]) == W * H * 65535 * 65535 and not count[0] and not count[2]
            with pytest.raises(ffs.FfsError, match="out of range"):
                st.radial_profile(B)


# ---- 2. carries and the wrap of sum_sq
def test_sum_carries_and_sum_sq_wraps(ffs):
    W = H = 300
    bins = np.zeros((H, W), np.uint16)
    # 32-bit pixels at 2^24 - 1 in one bin: sum_sq = 90 000 (2^24 - 1)^2 is beyond 2^64 and comes back modulo 2^64
    ctx = ffs.Context(W, H, np.uint32)
    ctx.set_radial_bins(bins, 1)
    st = ctx.stream()
    img = np.full((1, H, W), (1 << 24) - 1, np.uint32)
    st.process(img)
    count, s, q = st.radial_profile(0)
    exact = 90000 * ((1 << 24) - 1) ** 2
    assert exact >= 1 << 64
    assert int(count[0]) == 90000 and int(s[0]) == 90000 * ((1 << 24) - 1) and int(q[0]) == exact % (1 << 64)
    _check(st, img, bins, 1)
    # 16-bit pixels at 65535: sum carries out of 32 bits, sum_sq is exact
    ctx = ffs.Context(W, H, np.uint16)
    ctx.set_radial_bins(bins, 1)
    st = ctx.stream()
    img = np.full((1, H, W), 65535, np.uint16)
    st.process(img)
    count, s, q = st.radial_profile(0)
    assert int(s[0]) == 90000 * 65535 > 1 << 32 and int(q[0]) == 90000 * 65535 ** 2
    _check(st, img, bins, 1)


# ---- 3. the inclusion rule
def _gappy_mask(W, H, seed):
    rng = np.random.default_rng(seed)
    m = np.ones((H, W), np.uint8)
    m[:, W // 3:W // 3 + 5] = 0
    m[H // 2:H // 2 + 3, :] = 0
    m[rng.random((H, W)) < 0.03] = 0
    return m


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_inclusion_rule(ffs, dtype):
    W, H = 517, 41
    bins, n_bins = R.shell_bins(W, H, 12), 12
    mask = _gappy_mask(W, H, 3)
    frames = _frames(dtype, 2, H, W, seed=11)
    assert (frames > 1000).sum() > 100 and (frames <= 1000).sum() > 1000
    if np.dtype(dtype) == np.dtype(np.uint32):
        assert (frames == 1 << 24).any() and (frames == (1 << 24) - 1).any() and (frames > 1 << 24).any()
    ctx = ffs.Context(W, H, dtype, max_batch=2)
    ctx.set_mask(mask)
    ctx.set_radial_bins(bins)          # n_bins defaults to max + 1
    st = ctx.stream()
    st.process(frames)
    _check(st, frames, bins, n_bins, mask)
    open_profile = [st.radial_profile(f) for f in range(2)]
    for scope in ("centre", "window"):
        ctx.set_max_valid_scope(scope)
        ctx.set_params(max_valid=1000)
        st.process(frames)
        _check(st, frames, bins, n_bins, mask, max_valid=1000)
        assert not np.array_equal(st.radial_profile(0)[1], open_profile[0][1])
    ctx.set_max_valid_scope("centre")
    ctx.set_params(max_valid=-1)       # kept across set_params, and the map is still there
    st.process(frames)
    for f in range(2):
        for a, b in zip(st.radial_profile(f), open_profile[f]):
            assert np.array_equal(a, b)
    # the resolution mask after the map: the profile follows the mask as it stands at submit
    ctx.apply_resolution_mask(1.0, 0.2, 250.0, 20.0, 75e-6, 75e-6, dmin=15.0, dmax=-1.0)
    now = ctx.get_mask()
    assert now.sum() < mask.sum() and now.sum() > 0
    st.process(frames)
    _check(st, frames, bins, n_bins, now)


# ---- 4. the profile does not depend on the threshold stage, and the threshold stage does not notice the map
def test_independence_of_the_threshold_stage(ffs):
    from util import make_frame
    W, H = 530, 97
    img, mask = make_frame(W, H, np.uint16, seed=4)
    frames = np.stack([img, np.ascontiguousarray(img[::-1])])
    bins, n_bins = R.shell_bins(W, H, 20), 20
    want = [R.radial_profile(f, bins, n_bins, mask) for f in frames]

    def run(with_map, tuning=None, gain=0.0, **params):
        ctx = ffs.Context(W, H, np.uint16, max_batch=2)
        ctx.set_mask(mask)
        if tuning:
            ctx.set_tuning(**tuning)
        ctx.set_params(want_strong_list=1, **params)
        ctx.set_gain(gain)
        if with_map:
            ctx.set_radial_bins(bins, n_bins)
        st = ctx.stream()
        res = st.process(frames)
        return st, res

    variants = {"default": {}, "window_kernel": {"tuning": {"window_kernel": 1}}, "kernel_half_x_5": {"kernel_half_x": 5},
                "extended": {"algorithm": ffs.ALGO_DISPERSION_EXTENDED}, "gain": {"gain": 2.5}, "grid_kernels": {"tuning": {"sparse_stage": 1}},
                "profile_in_the_dense_stream": {"tuning": {"radial_stream": 1}}}
    for name, kw in variants.items():
        st, res = run(True, **kw)
        path = st.last_path()[0]
        assert "radial" in path, name
        if name == "window_kernel" or name == "kernel_half_x_5" or name == "gain":
            assert "window" in path, (name, path)
        if name == "extended":
            assert "extended" in path
        if name == "grid_kernels":
            assert "grid_kernels" in path
        for f in range(2):
            for a, b in zip(st.radial_profile(f), want[f]):
                assert np.array_equal(a, b), (name, f)
        st0, res0 = run(False, **kw)
        assert "radial" not in st0.last_path()[0]
        for a, b in zip(res, res0):
            assert a.num_strong_pixels == b.num_strong_pixels and np.array_equal(a.strong_k, b.strong_k) and np.array_equal(a.boxes, b.boxes), name
        assert sum(r.num_strong_pixels for r in res) > 0, name


# ---- 4b. where the profile's launches run (tuning "radial_stream"), on maps whose edges run along the rows: all 64 lanes of a wave change
#          bin in one step and add into one or two bins
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("tuning", [{"radial_stream": 0}, {"radial_stream": 1}, {"radial_map8": 1}, {"radial_stream": 1, "radial_map8": 1}],
                         ids=lambda t: "+".join("%s_%d" % kv for kv in t.items()))
def test_row_edges_and_both_placements(ffs, dtype, tuning):
    W, H = 1030, 37
    rows = np.repeat((np.arange(H) // 3).astype(np.uint16)[:, None], W, axis=1)     # edges along the rows: all 64 lanes change bin in one step
    blocks = ((np.arange(H)[:, None] // 5) * 4 + np.arange(W)[None, :] // 300).astype(np.uint16)   # ... and 37 or 64 of them, in two bins
    frames = _frames(dtype, 3, H, W, seed=77)
    mask = _gappy_mask(W, H, 5)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    ctx.set_mask(mask)
    ctx.set_tuning(**tuning)
    st = ctx.stream()
    holes = R.shell_bins(W, H, 255).copy()          # the most bins the one-byte form of the map takes, every third entry in no bin
    holes.reshape(-1)[::3] = NO_BIN
    wide = np.random.default_rng(3).integers(0, 256, (H, W)).astype(np.uint16)   # 256 bins: two bytes an entry whatever the tuning says
    for bins in (rows, blocks, R.shell_bins(W, H, 30), holes, wide):
        n_bins = int(bins[bins != NO_BIN].max()) + 1
        ctx.set_radial_bins(bins, n_bins)
        for _ in range(2):
            st.process(frames)
            assert "radial" in st.last_path()[0]
            _check(st, frames, bins, n_bins, mask)


# ---- 5. every way in
def _resident_padded(ctx, frames):
    """The frames in the context's pitched device layout, the row padding and the tail of every frame filled with ones."""
    import torch
    pitch, fstride = ctx.device_layout()
    B, H, W = frames.shape
    item = frames.dtype.itemsize
    host = np.full((B, fstride // item), np.iinfo(frames.dtype).max, frames.dtype)
    rows = host[:, :H * (pitch // item)].reshape(B, H, pitch // item)
    rows[:, :, :W] = frames
    assert pitch // item > W
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).to("cuda:0"), pitch, fstride


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_every_way_in(ffs, dtype):
    from ffs_amd import bslz4, byteoffset
    W, H = 517, 41
    bins, n_bins = R.shell_bins(W, H, 9), 9
    mask = _gappy_mask(W, H, 8)
    frames = _frames(dtype, 3, H, W, seed=21)
    if np.dtype(dtype) == np.dtype(np.uint32):
        frames = np.minimum(frames, 0x7FFFFFFF).astype(dtype)   # (what a byte-offset section holds: int32)
    ctx = ffs.Context(W, H, dtype, max_batch=3)
    ctx.set_mask(mask)
    ctx.set_radial_bins(bins, n_bins)
    st = ctx.stream()
    st.submit(frames)
    st.wait()
    _check(st, frames, bins, n_bins, mask)
    mem, pitch, fstride = _resident_padded(ctx, frames)
    st.submit_device(mem.data_ptr(), pitch, fstride, 3)
    st.wait()
    _check(st, frames, bins, n_bins, mask)
    st.process_compressed([bslz4.compress(f) for f in frames[::-1]])
    _check(st, frames[::-1], bins, n_bins, mask)
    st.process_encoded([byteoffset.compress(f) for f in frames[1:]], ffs.CODEC_BYTE_OFFSET)
    _check(st, frames[1:], bins, n_bins, mask)
    assert "radial" in st.last_path()[0]


# ---- 6. a batch that ffs_wait runs again keeps the profile of its first pass
def test_reruns_neither_recompute_nor_double_count(ffs):
    rng = np.random.default_rng(9)
    W, H = 1000, 300
    base = rng.poisson(2.0, (H, W)).astype(np.uint16)
    fat = base.copy()
    fat[100:130, 200:240] = 3000          # a block whose rim is strong: a band beyond the band plan, a frame beyond the 100 pixels the lists hold
    frames = np.stack([base, fat])
    bins, n_bins = R.shell_bins(W, H, 100), 100
    ctx = ffs.Context(W, H, np.uint16, max_batch=2, max_strong_per_frame=100)
    ctx.set_params(min_spot_size=1)
    ctx.set_radial_bins(bins, n_bins)
    st = ctx.stream()
    res = st.process(frames)
    path, reruns = st.last_path()
    assert reruns >= 1 and "radial" in path, (path, reruns)
    assert res[1].num_strong_pixels > 100      # (that frame was run again on its own as well)
    _check(st, frames, bins, n_bins)


# ---- 7. two streams of one context, batches in flight together
def test_two_streams_keep_their_own_profiles(ffs):
    W, H = 517, 41
    bins, n_bins = R.shell_bins(W, H, 7), 7
    ctx = ffs.Context(W, H, np.uint16, max_batch=2)
    ctx.set_radial_bins(bins, n_bins)
    a, b = ctx.stream(), ctx.stream()
    fa, fb, fc = (_frames(np.uint16, 2, H, W, seed=s) for s in (1, 2, 3))
    a.submit(fa)
    b.submit(fb)
    a.wait()
    b.wait()
    _check(a, fa, bins, n_bins)
    _check(b, fb, bins, n_bins)
    a.submit(fc)            # a's next batch in flight: b's profile, and a's last one, stay as they are until a's next wait
    _check(b, fb, bins, n_bins)
    _check(a, fa, bins, n_bins)
    a.wait()
    _check(a, fc, bins, n_bins)   # ... which replaces it
    _check(b, fb, bins, n_bins)


# ---- 8. refusals leave the state as it was; NULL drops the map
def test_refusals_and_dropping_the_map(ffs):
    W, H = 37, 29
    bins, n_bins = R.shell_bins(W, H, 6), 6
    frames = _frames(np.uint16, 1, H, W, seed=4)
    ctx = ffs.Context(W, H, np.uint16)
    st = ctx.stream()
    with pytest.raises(ffs.FfsError, match="without a bin map"):
        st.radial_profile(0)                       # nothing waited for yet
    ctx.set_radial_bins(bins, n_bins)

    def still_the_map():
        st.process(frames)
        assert "radial" in st.last_path()[0]
        _check(st, frames, bins, n_bins)

    for bad in (0, 1025, 70000):
        with pytest.raises(ffs.FfsError, match="n_bins must be in 1..1024"):
            ctx.set_radial_bins(bins, bad)
        still_the_map()
    wrong = bins.copy()
    wrong[5, 7] = 6                                # == n_bins: not a bin, and not 0xFFFF
    wrong[20, 3] = 900
    with pytest.raises(ffs.FfsError, match=rf"ffs_ctx_set_radial_bins: entry {5 * W + 7} \(x = 7, y = 5\) is 6"):
        ctx.set_radial_bins(wrong, n_bins)
    still_the_map()
    for shape in ((W, H), (H, W - 1), (H * W,)):
        with pytest.raises(ValueError, match="bin map must have shape"):
            ctx.set_radial_bins(np.zeros(shape, np.uint16))
    with pytest.raises(ValueError, match="0..65535"):
        ctx.set_radial_bins(np.full((H, W), 70000, np.int64))
    # while a batch is in flight a map is refused; the batch keeps the one it was submitted with
    st.submit(frames)
    with pytest.raises(ffs.FfsError, match="in flight"):
        ctx.set_radial_bins(np.zeros((H, W), np.uint16), 1)
    st.wait()
    _check(st, frames, bins, n_bins)
    still_the_map()
    with pytest.raises(ffs.FfsError, match="out of range"):
        st.radial_profile(1)
    # NULL is accepted with a batch in flight, as for the gain map: that batch still hands out its profile, the next has none
    st.submit(frames)
    ctx.set_radial_bins(None)
    st.wait()
    assert "radial" in st.last_path()[0]
    _check(st, frames, bins, n_bins)
    plain = st.process(frames)
    assert "radial" not in st.last_path()[0]
    with pytest.raises(ffs.FfsError, match="without a bin map"):
        st.radial_profile(0)
    # a later map with more bins (the buffers grow), then a smaller one again
    big = np.random.default_rng(1).integers(0, 1024, (H, W)).astype(np.uint16)
    ctx.set_radial_bins(big, 1024)
    again = st.process(frames)
    _check(st, frames, big, 1024)
    assert again[0].num_strong_pixels == plain[0].num_strong_pixels
    ctx.set_radial_bins(bins, n_bins)
    still_the_map()


# ---- 9. the measurement entry point leaves the handed-out profile alone
def test_bench_radial(ffs):
    from util import _resident
    W, H = 517, 41
    bins, n_bins = R.shell_bins(W, H, 9), 9
    frames = _frames(np.uint16, 2, H, W, seed=6)
    ctx = ffs.Context(W, H, np.uint16, max_batch=2)
    st = ctx.stream()
    mem, pitch, fstride = _resident(ctx, frames)
    with pytest.raises(ffs.FfsError, match="no bin map"):
        st.bench_radial(mem.data_ptr(), pitch, fstride, 2, 2)
    ctx.set_radial_bins(bins, n_bins)
    st.process(frames)
    ms = st.bench_radial(mem.data_ptr(), pitch, fstride, 2, 3)
    assert 0.0 < ms < 100.0
    _check(st, frames, bins, n_bins)
    st.process(frames[::-1])
    _check(st, frames[::-1], bins, n_bins)


# ---- 10. the driver
def _run(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", out), err, lines


def _stable(text):
    """stdout without what the clock decides: durations and rates (every number with a decimal point, every number of ms)."""
    return re.sub(r"\d+\.\d+", "#", re.sub(r"\d+(?:\.\d+)? ms", "# ms", text)).split("\n")


def test_driver_radial_bins(ffs, tmp_path):
    from ffs_amd import synth
    N, SHELLS = 4, 8       # (two batches of two images: the second profile of a stream, after the buffers took turns)
    # the map of the driver's own builder (host/radial_bins.hpp), through its check program, with the geometry of synth:tiny
    exe = tmp_path / "radial_bins_check"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", HOST, os.path.join(ROOT, "tests", "radial_bins_check.cc"), "-o", str(exe)], check=True)
    dump = subprocess.run([str(exe), "dump", str(tmp_path / "map.u16"), "300", "200", str(SHELLS), "0.976", "0.3", "150", "100", "0.75e-4", "0.75e-4"],
                          capture_output=True, text=True, check=True)
    bins = np.fromfile(tmp_path / "map.u16", "<u2").reshape(200, 300)
    assert sorted(np.unique(bins)) == list(range(SHELLS))
    edges = [float(v) for v in dump.stdout.split()]
    common = ["synth:tiny:%d" % N, "--threads", "1", "--batch", "2", "--single-buffer", "--max-valid", "none"]
    rc, out, err, lines = _run(common + ["--radial-bins", str(SHELLS)], tmp_path)
    assert rc == 0 and not err, (out, err)
    head = [l for l in out.split("\n") if l.startswith("Radial bins:")]
    assert len(head) == 1 and head[0].startswith("Radial bins: %d shells, d edges (A): inf " % SHELLS), head
    shown = head[0].split(": ")[2].split()
    assert len(shown) == SHELLS + 1 and all(abs(float(a) - b) <= 1e-3 * b for a, b in zip(shown[1:], edges[1:]))
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    for i, img in enumerate(frames):
        count, s, q = R.radial_profile(img, bins, SHELLS)
        assert got[i]["radial_count"] == [int(v) for v in count]
        assert got[i]["radial_sum"] == [int(v) for v in s]
        assert got[i]["radial_sum_sq"] == [int(v) for v in q]
        assert list(got[i]) == sorted(got[i])       # keys in alphabetical order, as before
    # without the flag: stdout and the JSON lines of one run are those of the next
    rc1, out1, err1, lines1 = _run(common, tmp_path)
    rc2, out2, err2, lines2 = _run(common, tmp_path)
    assert rc1 == rc2 == 0 and sorted(lines1) == sorted(lines2) and "radial" not in "".join(lines1) and "Radial bins" not in out1
    assert _stable(out1) == _stable(out2)
    assert [l for l in _stable(out) if not l.startswith("Radial bins:")] == _stable(out1)   # the flag adds its one line to stdout, nothing else
    plain = {json.loads(l)["file-number"]: json.loads(l) for l in lines1}
    for i in range(N):
        assert {k: v for k, v in got[i].items() if not k.startswith("radial_")} == plain[i]
