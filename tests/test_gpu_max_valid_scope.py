"""GPU: the window scope of max_valid (ffs_ctx_set_max_valid_scope(FFS_MAX_VALID_WINDOW)): a pixel above max_valid is masked for its
frame.  Every comparison is exact equality with the oracle run on the per-frame mask `mask & (img <= max_valid)` -- the standard
algorithm through the general-window kernel at every window and through the gather of threshold_path 2, the extended algorithm
(flavour 0) with its debug planes, the per-batch snapshot, and the driver's --max-valid-scope."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import tie_windows as T
from oracle import oracle as O
from util import _blob_frame, assert_frame_matches_oracle, make_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOTFINDER = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "spotfinder")
BIG = 1 << 24


def _disp(kx, ky, min_count=2):
    return O.DispParams(kx, ky, min_count, 0.0, 6.0, 3.0)


def _mask2(img, mask, max_valid):
    return (mask & (img <= max_valid)).astype(np.uint8)


def _want_window(img, mask, max_valid, kx=3, ky=3, min_count=2):
    """What FFS_MAX_VALID_WINDOW must give: the oracle on the per-frame mask."""
    return O.dispersion(img, _mask2(img, mask, max_valid), _disp(kx, ky, min_count))


def _want_centre(img, mask, max_valid, kx=3, ky=3, min_count=2):
    """What FFS_MAX_VALID_CENTRE gives today: the oracle on the static mask, the pixels above max_valid cleared."""
    return (O.dispersion(img, mask, _disp(kx, ky, min_count)) & (img <= max_valid)).astype(np.uint8)


def _ctx(ffs, W, H, dtype, max_valid, scope="window", kx=3, ky=3, max_batch=1, tuning=None, mask=None, max_strong_per_frame=0, **kw):
    ctx = ffs.Context(W, H, dtype, max_batch=max_batch, max_strong_per_frame=max_strong_per_frame)
    if tuning:
        ctx.set_tuning(**tuning)
    kw.setdefault("want_strong_mask", 1)
    kw.setdefault("want_strong_list", 1)
    ctx.set_params(want_reflections=1, kernel_half_x=kx, kernel_half_y=ky, max_valid=max_valid, **kw)
    ctx.set_max_valid_scope(scope)
    if mask is not None:
        ctx.set_mask(mask)
    return ctx


def _limits(dtype):
    """(overload value, max_valid) of the two pixel types"""
    return (65535, 60000) if np.dtype(dtype) == np.uint16 else (BIG - 1, 1_000_000)


# ---- 1. the frame of the issue: 530 x 97, 12 overloads two columns to the right of strong pixels, 7 at corners and strip edges
_OVERLOAD_FRAMES = {}


def _overload_frame(dtype):
    key = np.dtype(dtype).name
    if key not in _OVERLOAD_FRAMES:
        W, H = 530, 97
        img, mask = make_frame(W, H, dtype, seed=12, n_spots=40, masked=True)
        over, _ = _limits(dtype)
        ys, xs = np.nonzero(O.dispersion(img, mask))
        pick = np.random.default_rng(5).choice(len(ys), 12, replace=False)
        img = img.copy()
        for y, x in zip(ys[pick], xs[pick]):
            img[y, min(x + 2, W - 1)] = over
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (40, 495), (40, 496), (41, 0)):
            img[y, x] = over
        img.setflags(write=False)
        mask.setflags(write=False)
        _OVERLOAD_FRAMES[key] = (img, mask)
    return _OVERLOAD_FRAMES[key]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", [(3, 3), (1, 1), (5, 2), (7, 7)], ids=["3x3", "1x1", "5x2", "7x7"])
def test_overloads_leave_every_window(ffs, kx, ky, dtype):
    img, static = _overload_frame(dtype)
    H, W = img.shape
    _, max_valid = _limits(dtype)
    for mask in (static, np.ones((H, W), np.uint8)):
        want_w, want_c = _want_window(img, mask, max_valid, kx, ky), _want_centre(img, mask, max_valid, kx, ky)
        assert want_w.sum() > 0 and not np.array_equal(want_w, want_c)   # (from the oracle alone: the scope matters on this frame)
        ctx = _ctx(ffs, W, H, dtype, max_valid, "window", kx, ky, mask=mask)
        st = ctx.stream()
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want_w)
        assert "window" in st.last_path()[0]
        # the default scope is today's behaviour, on the same stream and on a context that never heard of the setter
        ctx.set_max_valid_scope("centre")
        assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want_c)
        assert ("window" in st.last_path()[0]) == ((kx, ky) != (3, 3))
        ctx0 = ffs.Context(W, H, dtype)
        ctx0.set_params(want_strong_mask=1, want_strong_list=1, kernel_half_x=kx, kernel_half_y=ky, max_valid=max_valid)
        ctx0.set_mask(mask)
        assert_frame_matches_oracle(ctx0.stream().process(img[None])[0], img, mask, strong=want_c)


def test_scope_without_max_valid_changes_nothing(ffs):
    """max_valid < 0: the batch takes the paths it takes today."""
    img, mask = _overload_frame(np.uint16)
    H, W = img.shape
    ctx = _ctx(ffs, W, H, np.uint16, -1, "window", mask=mask)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask)
    assert "window" not in st.last_path()[0]


# ---- 2. the cross-check path of `spotfinder --validate`
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", [(3, 3), (2, 5)], ids=["3x3", "2x5"])
def test_threshold_path_2(ffs, kx, ky, dtype):
    W, H = 301, 77
    img, mask = make_frame(W, H, dtype, seed=21, n_spots=30, masked=True)
    over, max_valid = _limits(dtype)
    rng = np.random.default_rng(3)
    img[rng.random((H, W)) < 0.01] = over
    want = _want_window(img, mask, max_valid, kx, ky)
    assert want.sum() > 0 and not np.array_equal(want, _want_centre(img, mask, max_valid, kx, ky))
    ctx = _ctx(ffs, W, H, dtype, max_valid, "window", kx, ky, tuning={"threshold_path": 2}, mask=mask)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" not in st.last_path()[0]


# ---- 3. strip edges of the kernel, frames narrower or shorter than the window
@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (9, 5), (495, 6), (496, 9), (497, 4), (64, 1), (1, 40)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_edge_shapes(ffs, W, H, dtype):
    rng = np.random.default_rng(W * 1000 + H)
    over, max_valid = _limits(dtype)
    base = rng.poisson(2.0, size=(H, W)).astype(dtype)
    hot = rng.random((H, W)) < 0.05
    base[hot] = rng.integers(50, 3000, size=hot.sum()).astype(dtype)
    mask = (rng.random((H, W)) > 0.1).astype(np.uint8)
    some = base.copy()
    some[rng.random((H, W)) < 0.05] = over            # about 5 % overloads
    every = np.full((H, W), over, dtype)              # every pixel overloaded: no strong pixel, no fault
    under = base.copy()
    under[mask == 0] = over                           # overloads only under the static mask: the scope changes nothing
    frames = np.stack([some, every, under])
    ctx = _ctx(ffs, W, H, dtype, max_valid, "window", max_batch=3, mask=mask)
    st = ctx.stream()
    for kx, ky in ((3, 3), (5, 5), (7, 2)):
        ctx.set_params(kernel_half_x=kx, kernel_half_y=ky)
        res = st.process(frames)
        assert "window" in st.last_path()[0]
        for fr, img in zip(res, frames):
            assert_frame_matches_oracle(fr, img, mask, strong=_want_window(img, mask, max_valid, kx, ky))
        assert res[1].num_strong_pixels == 0
        assert np.array_equal(_want_window(under, mask, max_valid, kx, ky), _want_centre(under, mask, max_valid, kx, ky))


# ---- 4. limits
def test_max_valid_zero(ffs):
    W, H = 200, 50
    rng = np.random.default_rng(17)
    for dtype in (np.uint16, np.uint32):
        img = (rng.poisson(0.3, (H, W)) * (rng.random((H, W)) < 0.5)).astype(dtype)
        mask = (rng.random((H, W)) > 0.1).astype(np.uint8)
        ctx = _ctx(ffs, W, H, dtype, 0, "window", mask=mask)
        fr = ctx.stream().process(img[None])[0]
        assert_frame_matches_oracle(fr, img, mask, strong=_want_window(img, mask, 0))
        assert fr.num_strong_pixels == 0   # (only zeros are left: threshold 0 refuses them)


def test_max_valid_65535_on_u16_masks_nothing(ffs):
    img, mask = _overload_frame(np.uint16)
    H, W = img.shape
    want = _want_window(img, mask, 65535)
    assert np.array_equal(want, _want_centre(img, mask, 65535)) and np.array_equal(want, O.dispersion(img, mask))
    ctx = _ctx(ffs, W, H, np.uint16, 65535, "window", mask=mask)
    st = ctx.stream()
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=want)
    assert "window" in st.last_path()[0]


@pytest.mark.parametrize("max_valid", [BIG - 1, BIG, BIG + 100, (1 << 32) - 1], ids=["2^24-1", "2^24", "2^24+100", "2^32-1"])
def test_u32_max_valid_at_or_above_2_24(ffs, max_valid):
    """The oracle's p < 2^24 rule holds on top: the neighbour limit is min(max_valid, 2^24 - 1); a centre at 2^24 <= max_valid stays valid."""
    W, H = 257, 60
    rng = np.random.default_rng(9)
    img = rng.poisson(5.0, size=(H, W)).astype(np.uint32)
    sel = rng.random((H, W))
    img[sel < 0.03] = BIG - 1
    img[(sel >= 0.03) & (sel < 0.06)] = BIG
    img[(sel >= 0.06) & (sel < 0.08)] = BIG + 101
    img[(sel >= 0.08) & (sel < 0.1)] = rng.integers(1 << 20, BIG, size=((sel >= 0.08) & (sel < 0.1)).sum())
    mask = (rng.random((H, W)) > 0.05).astype(np.uint8)
    for kx, ky in ((3, 3), (2, 5)):
        want = _want_window(img, mask, max_valid, kx, ky)
        assert want.sum() > 0
        ctx = _ctx(ffs, W, H, np.uint32, max_valid, "window", kx, ky, mask=mask)
        assert_frame_matches_oracle(ctx.stream().process(img[None])[0], img, mask, strong=want)


def test_min_count_40_with_dense_overloads(ffs):
    """Overloads dense enough that 7x7 windows fall on both sides of min_count = 40."""
    W, H = 300, 80
    rng = np.random.default_rng(23)
    for dtype in (np.uint16, np.uint32):
        over, max_valid = _limits(dtype)
        img, _ = make_frame(W, H, dtype, seed=31, n_spots=60)
        img = img.copy()
        img[rng.random((H, W)) < 0.15] = over
        mask = np.ones((H, W), np.uint8)
        valid = np.pad((img <= max_valid).astype(np.int64), 3)
        m = sum(valid[3 + dy:3 + dy + H, 3 + dx:3 + dx + W] for dy in range(-3, 4) for dx in range(-3, 4))
        inner = m[3:-3, 3:-3]
        assert (inner < 40).sum() > 100 and (inner >= 40).sum() > 100
        want = _want_window(img, mask, max_valid, min_count=40)
        assert want.sum() > 0 and not np.array_equal(want, _want_window(img, mask, max_valid, min_count=2))
        ctx = _ctx(ffs, W, H, dtype, max_valid, "window", min_count=40)
        assert_frame_matches_oracle(ctx.stream().process(img[None])[0], img, mask, strong=want)


# ---- 5. the scope is a per-batch snapshot taken at submit
def test_scope_changed_between_batches_in_flight(ffs):
    img, mask = _overload_frame(np.uint16)
    H, W = img.shape
    frames = np.stack([img, img[::-1].copy()])
    mask = np.ones((H, W), np.uint8)
    ctx = _ctx(ffs, W, H, np.uint16, 60000, "window", max_batch=2)
    a, b = ctx.stream(), ctx.stream()
    a.submit(frames)
    ctx.set_max_valid_scope("centre")
    b.submit(frames)
    ctx.set_max_valid_scope("window")
    ctx.set_params(max_valid=60000)   # the scope is kept across ffs_ctx_set_params
    for fr, f in zip(a.wait(), frames):
        assert_frame_matches_oracle(fr, f, mask, strong=_want_window(f, mask, 60000))
    for fr, f in zip(b.wait(), frames):
        assert_frame_matches_oracle(fr, f, mask, strong=_want_centre(f, mask, 60000))
    assert "window" in a.last_path()[0] and "window" not in b.last_path()[0]
    for fr, f in zip(b.process(frames), frames):
        assert_frame_matches_oracle(fr, f, mask, strong=_want_window(f, mask, 60000))
    assert "window" in b.last_path()[0]


def test_overflow_rerun_keeps_the_scope(ffs):
    """A frame with more strong pixels than the stream's lists is run again inside ffs_wait, on a one-frame stream: under the
    scope its batch was submitted with, whatever the context says by then."""
    W, H = 300, 200
    img = T.dense_frame((H, W), np.uint16).copy()   # Poisson(300) with 1 % of the pixels near 20300: they are strong under either scope
    sel = np.random.default_rng(8).random((H, W))
    img[sel < 0.01] = 700                            # weaker peaks, which an overload in their window hides under the centre scope
    img[(sel >= 0.01) & (sel < 0.015)] = 65535
    max_valid = 60000
    mask = np.ones((H, W), np.uint8)
    want = _want_window(img, mask, max_valid)
    assert want.sum() > 500 and not np.array_equal(want, _want_centre(img, mask, max_valid))
    other = make_frame(W, H, np.uint16, seed=3)[0]
    frames = np.stack([img, other])
    ctx = _ctx(ffs, W, H, np.uint16, max_valid, "window", max_batch=2, max_strong_per_frame=500)
    st = ctx.stream()
    st.submit(frames)
    ctx.set_max_valid_scope("centre")   # the context moves on; the batch in flight and its re-run keep the window scope
    res = st.wait()
    assert_frame_matches_oracle(res[0], img, mask, strong=want)
    assert_frame_matches_oracle(res[1], other, mask, strong=_want_window(other, mask, max_valid))
    # The stream's lists hold 500 entries: a complete list of more (held to the oracle entry by entry above) can only have come from
    # the frame's re-run on the one-frame stream, which rerun_overflow_frames enqueues with the batch's own snapshot.
    assert res[0].num_strong_pixels == int(want.sum()) > 500 and len(res[0].strong_k) == int(want.sum())


@pytest.mark.parametrize("codec", ["bslz4", "byte_offset"])
def test_encoded_submit_keeps_the_scope(ffs, codec):
    """ffs_submit_compressed / ffs_submit_encoded enqueue from a helper thread: with the snapshot taken at the submit call, whatever
    the context is set to before the wait."""
    from ffs_amd import bslz4, byteoffset
    img, mask = _overload_frame(np.uint16)
    H, W = img.shape
    frames = [np.ascontiguousarray(img), np.ascontiguousarray(img[::-1])]
    ctx = _ctx(ffs, W, H, np.uint16, 60000, "window", max_batch=2, mask=mask)
    st = ctx.stream()
    if codec == "bslz4":
        st.submit_compressed([bslz4.compress(f) for f in frames])
    else:
        st.submit_encoded([byteoffset.compress(f) for f in frames], ffs.CODEC_BYTE_OFFSET)
    ctx.set_max_valid_scope("centre")
    res = st.wait()
    for fr, f in zip(res, frames):
        assert_frame_matches_oracle(fr, f, mask, strong=_want_window(f, mask, 60000))
    assert "window" in st.last_path()[0]


@pytest.mark.parametrize("want_mask,want_list", [(0, 0), (0, 1), (1, 0)])
def test_three_streams_in_flight(ffs, want_mask, want_list):
    W, H, B = 700, 130, 3
    rng = np.random.default_rng(41)
    frames = np.stack([make_frame(W, H, np.uint16, seed=40 + i, n_spots=50)[0] for i in range(3 * B)])
    frames[rng.random(frames.shape) < 0.002] = 65535
    mask = make_frame(W, H, np.uint16, seed=40, masked=True)[1]
    ctx = _ctx(ffs, W, H, np.uint16, 60000, "window", max_batch=B, mask=mask, want_strong_mask=want_mask, want_strong_list=want_list)
    streams = [ctx.stream() for _ in range(3)]
    for i, st in enumerate(streams):
        st.submit(frames[i * B:(i + 1) * B], first_frame_id=i * B)
    for i, st in enumerate(streams):
        res = st.wait()
        for fr, img in zip(res, frames[i * B:(i + 1) * B]):
            assert_frame_matches_oracle(fr, img, mask, strong=_want_window(img, mask, 60000))
        assert (res[0].strong_mask is not None) == bool(want_mask)
        assert (res[0].strong_k is not None) == bool(want_list)
        assert "window" in st.last_path()[0]


# ---- 6. the extended algorithm, flavour 0
def _blob_frame_with_overloads(dtype, seed):
    """300 x 200 blobs; overloads inside blobs, beside them (two columns off their right edge) and far from any."""
    from ffs_amd import synth
    W, H = 300, 200
    over, _ = _limits(dtype)
    img = _blob_frame(W, H, seed, 25).astype(dtype)
    rng = np.random.default_rng(seed + 1)
    blob = img >= 200
    near = np.zeros_like(blob)
    for dy in range(-12, 13):
        for dx in range(-12, 13):
            near |= np.roll(np.roll(blob, dy, 0), dx, 1)
    beside = np.zeros_like(blob)
    beside[:, 2:] = blob[:, :-2] & ~blob[:, 2:] & ~blob[:, 1:-1]
    for where, n in ((blob, 10), (beside, 15), (~near, 10)):
        ys, xs = np.nonzero(where)
        assert len(ys) >= n
        pick = rng.choice(len(ys), n, replace=False)
        img[ys[pick], xs[pick]] = over
    mask = synth.mask_modules(W, H, 140, 90, 6, 8)
    return img, mask


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("tuning", [{}, {"ext_fused": 1}, {"ext_erode": 0}], ids=["default", "fused", "erode0"])
def test_extended_flavour_0(ffs, dtype, tuning):
    img, mask = _blob_frame_with_overloads(dtype, 5)
    H, W = img.shape
    _, max_valid = _limits(dtype)
    strong, first, eroded = O.dispersion_extended(img, _mask2(img, mask, max_valid), None, 0, float(max_valid), debug=True)
    assert strong.sum() > 100
    assert not np.array_equal(strong, O.dispersion_extended(img, mask, None, 0, float(max_valid)))   # (the scope matters here)
    ctx = _ctx(ffs, W, H, dtype, max_valid, "window", tuning=tuning, mask=mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED)
    st = ctx.stream()
    fr = st.process(img[None])[0]
    d = np.argwhere(st.debug_bitplane(0, 1) != first)
    assert d.size == 0, f"first pass: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"
    d = np.argwhere(st.debug_bitplane(0, 2) != eroded)
    assert d.size == 0, f"erosion: {len(d)} mismatches, first at (y,x)={d[:5].tolist()}"
    assert_frame_matches_oracle(fr, img, mask, strong=strong)
    assert "extended" in st.last_path()[0]
    # and the default scope still gives what it gave
    ctx.set_max_valid_scope("centre")
    assert_frame_matches_oracle(st.process(img[None])[0], img, mask, strong=O.dispersion_extended(img, mask, None, 0, float(max_valid)))


def test_refusals(ffs):
    ctx = ffs.Context(64, 64, np.uint16)
    for bad in (2, -1, 7):
        with pytest.raises(ffs.FfsError):
            ctx.set_max_valid_scope(bad)
    with pytest.raises(ValueError):
        ctx.set_max_valid_scope("both")
    # the window scope and the device flavour of the extended algorithm, whichever call comes second; the state stays what it was
    ctx.set_max_valid_scope("window")
    with pytest.raises(ffs.FfsError):
        ctx.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=1)
    ctx.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=0)   # flavour 0 is fine
    ctx2 = ffs.Context(64, 64, np.uint16)
    ctx2.set_params(algorithm=ffs.ALGO_DISPERSION_EXTENDED, extended_flavour=1, max_valid=100, want_strong_mask=1)
    with pytest.raises(ffs.FfsError):
        ctx2.set_max_valid_scope("window")
    ctx2.set_max_valid_scope("centre")
    img = _blob_frame(64, 64, 2, 3)
    mask = np.ones((64, 64), np.uint8)
    # (still flavour 1 under the centre scope: the refused call changed nothing)
    assert_frame_matches_oracle(ctx2.stream().process(img[None])[0], img, mask, strong=O.dispersion_extended(img, mask, None, 1, 100.0))


# ---- 7. the driver
def _run(argv, cwd):
    r, w = os.pipe()
    proc = subprocess.Popen([SPOTFINDER, *argv, "--pipe_fd", str(w)], pass_fds=[w], cwd=cwd,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    os.close(w)
    out, err = proc.communicate(timeout=300)
    with os.fdopen(r) as f:
        lines = [l for l in f.read().split("\n") if l]
    return proc.returncode, re.sub(r"\x1b\[[0-9;]*m", "", out), err, lines


def test_driver_max_valid_scope_window(ffs, tmp_path):
    """A low max_valid turns ordinary spot peaks into overloads; the driver's per-image counts are the Python API's."""
    from ffs_amd import synth
    N = 4
    rc, out, err, lines = _run(["synth:tiny:%d" % N, "--threads", "2", "--batch", "2", "--max-valid", "50", "--max-valid-scope", "window",
                                "--validate"], tmp_path)
    assert rc == 0 and not err, (out, err)
    assert "Trusted range: pixels above 50 are masked for their frame" in out
    matches = re.findall(r"Image\s+(\d+): Compared: Match (\d+) px", out)
    assert sorted(int(a) for a, _ in matches) == list(range(N)) and "Mismatch" not in out
    got = {json.loads(l)["file-number"]: json.loads(l) for l in lines}
    assert sorted(got) == list(range(N))
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    frames = synth.frames(p, range(N), threads=2)
    mask = np.ones((200, 300), np.uint8)
    ctx = _ctx(ffs, 300, 200, np.uint16, 50, "window", max_batch=N)
    res = ctx.stream().process(frames)
    differs = False
    for i, (fr, img) in enumerate(zip(res, frames)):
        assert_frame_matches_oracle(fr, img, mask, strong=_want_window(img, mask, 50))
        assert got[i]["num_strong_pixels"] == fr.num_strong_pixels
        assert got[i]["n_spots_total"] == len(fr.boxes)
        differs |= not np.array_equal(_want_window(img, mask, 50), _want_centre(img, mask, 50))
    assert differs
    # and the centre scope says so too
    rc, out, err, _ = _run(["synth:tiny:1", "--max-valid", "50", "--max-valid-scope", "centre"], tmp_path)
    assert rc == 0 and "Trusted range: centre pixels above 50 are not spots" in out
