"""GPU: the dispersion threshold at windows other than 7x7 (ffs_params.kernel_half_x / _y, the general-window kernel of
kernels_window.hpp) -- every pixel, the boxes and the reflections against the oracle's restatement of standalone.cc at that
window (oracle.DispParams(kx, ky, ...)); and the 7x7 window through the same kernel (tuning "window_kernel" = 1)."""
import numpy as np
import pytest

import tie_windows as T
import window_ties as WT
from oracle import oracle as O
from util import assert_frame_matches_oracle, make_frame

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (7, 7), (1, 7), (7, 1), (2, 5)]


def _disp(kx, ky, min_count=2, threshold=0.0, nsig_b=6.0, nsig_s=3.0):
    return O.DispParams(kx, ky, min_count, threshold, nsig_b, nsig_s)


def _ctx(ffs, W, H, dtype, kx, ky, max_batch=1, want_mask=1, want_list=1, tuning=None, **kw):
    ctx = ffs.Context(W, H, dtype, max_batch=max_batch)
    if tuning:
        ctx.set_tuning(**tuning)
    ctx.set_params(want_strong_mask=want_mask, want_strong_list=want_list, want_reflections=1,
                   kernel_half_x=kx, kernel_half_y=ky, **kw)
    return ctx


def _check(res, frames, mask, kx, ky, min_count=2):
    for fr, img in zip(res, frames):
        assert_frame_matches_oracle(fr, img, mask, strong=O.dispersion(img, mask, _disp(kx, ky, min_count)))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("kx,ky", SIZES, ids=[f"{a}x{b}" for a, b in SIZES])
def test_window_sizes_match_oracle(ffs, kx, ky, dtype):
    """Masked and unmasked frames, a width that crosses the kernel's strip edge (496 px), the path bit."""
    W, H = 530, 97
    frames, masks = [], []
    for seed, masked in ((11, False), (12, True)):
        img, mask = make_frame(W, H, dtype, seed=seed, n_spots=40, masked=masked)
        frames.append(img)
        masks.append(mask)
    for img, mask in zip(frames, masks):
        tuning = {"window_kernel": 1} if (kx, ky) == (3, 3) else None
        ctx = _ctx(ffs, W, H, dtype, kx, ky, tuning=tuning)
        ctx.set_mask(mask)
        st = ctx.stream()
        _check(st.process(img[None]), [img], mask, kx, ky)
        assert "window" in st.last_path()[0]


@pytest.mark.parametrize("kx,ky", [(2, 5), (5, 5), (7, 7)], ids=["2x5", "5x5", "7x7"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_threshold_path_2_matches_oracle(ffs, kx, ky, dtype):
    """The cross-check path of `spotfinder --validate` (every valid pixel's window gathered: k_exact_w) at other windows."""
    W, H = 301, 77
    img, mask = make_frame(W, H, dtype, seed=21, n_spots=30, masked=True)
    ctx = _ctx(ffs, W, H, dtype, kx, ky, tuning={"threshold_path": 2})
    ctx.set_mask(mask)
    st = ctx.stream()
    _check(st.process(img[None]), [img], mask, kx, ky)
    assert "window" not in st.last_path()[0]


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (9, 5), (14, 3), (62 * 8 - 1, 6), (62 * 8, 9), (62 * 8 + 1, 4), (62 * 16 + 3, 20),
                                 (64, 1), (1, 40)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_edges_and_narrow_frames(ffs, W, H, dtype):
    """Strip edges of the kernel, and frames narrower or shorter than the window (clipping, standalone.cc:126-130)."""
    rng = np.random.default_rng(W * 1000 + H)
    vmax = 65535 if dtype == np.uint16 else (1 << 24) + 5
    img = rng.poisson(2.0, size=(H, W)).astype(dtype)
    hot = rng.random((H, W)) < 0.05
    img[hot] = rng.integers(50, 3000, size=hot.sum()).astype(dtype)
    img[rng.random((H, W)) < 0.01] = vmax
    mask = (rng.random((H, W)) > 0.1).astype(np.uint8)
    for kx, ky in ((5, 5), (7, 2), (1, 7)):
        ctx = _ctx(ffs, W, H, dtype, kx, ky)
        ctx.set_mask(mask)
        _check(ctx.stream().process(img[None]), [img], mask, kx, ky)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("want_mask,want_list", [(0, 0), (0, 1), (1, 0)])
def test_batches_in_flight_and_outputs(ffs, dtype, want_mask, want_list):
    """Batches of several frames through three streams in flight; the byte mask and the lists on and off."""
    W, H, B = 700, 130, 3
    frames = np.stack([make_frame(W, H, dtype, seed=40 + i, n_spots=50)[0] for i in range(3 * B)])
    mask = make_frame(W, H, dtype, seed=40, masked=True)[1]
    ctx = _ctx(ffs, W, H, dtype, 4, 2, max_batch=B, want_mask=want_mask, want_list=want_list)
    ctx.set_mask(mask)
    streams = [ctx.stream() for _ in range(3)]
    for i, st in enumerate(streams):
        st.submit(frames[i * B:(i + 1) * B], first_frame_id=i * B)
    for i, st in enumerate(streams):
        res = st.wait()
        _check(res, frames[i * B:(i + 1) * B], mask, 4, 2)
        assert (res[0].strong_mask is not None) == bool(want_mask)
        assert (res[0].strong_k is not None) == bool(want_list)
        assert "window" in st.last_path()[0]


def test_bright_frames(ffs):
    """Sum p >= 2^16 in 16-bit windows; 32-bit pixels at 2^24 - 1 and 2^24, as neighbours and as centres."""
    W, H = 257, 60
    rng = np.random.default_rng(9)
    img16 = rng.integers(0, 65536, size=(H, W)).astype(np.uint16)
    img16[::3, ::2] = rng.integers(0, 40, size=img16[::3, ::2].shape)
    img32 = rng.poisson(5.0, size=(H, W)).astype(np.uint32)
    sel = rng.random((H, W))
    img32[sel < 0.04] = (1 << 24) - 1
    img32[(sel >= 0.04) & (sel < 0.08)] = 1 << 24
    img32[(sel >= 0.08) & (sel < 0.1)] = rng.integers(1 << 20, 1 << 24, size=((sel >= 0.08) & (sel < 0.1)).sum())
    mask = (rng.random((H, W)) > 0.05).astype(np.uint8)
    for img in (img16, img32):
        for kx, ky in ((7, 7), (2, 5)):
            ctx = _ctx(ffs, W, H, img.dtype, kx, ky)
            ctx.set_mask(mask)
            strong = O.dispersion(img, mask, _disp(kx, ky))
            assert strong.sum() > 0
            _check(ctx.stream().process(img[None]), [img], mask, kx, ky)


def test_dense_frame_overflow_rerun(ffs):
    """A frame with more strong pixels than the stream's lists: ffs_wait runs it again, at the batch's own window."""
    W, H = 300, 200
    img = T.dense_frame((H, W), np.uint16)
    mask = np.ones((H, W), np.uint8)
    ctx = ffs.Context(W, H, np.uint16, max_batch=2, max_strong_per_frame=500)
    ctx.set_params(want_strong_mask=1, want_strong_list=1, kernel_half_x=5, kernel_half_y=2)
    st = ctx.stream()
    frames = np.stack([img, make_frame(W, H, np.uint16, seed=3)[0]])
    st.submit(frames)
    ctx.set_params(kernel_half_x=1, kernel_half_y=1)   # the context moves on; the batch in flight keeps 5,2
    res = st.wait()
    assert O.dispersion(img, mask, _disp(5, 2)).sum() > 500
    _check(res, frames, mask, 5, 2)
    assert res[0].num_strong_pixels > 500   # (more than the stream's lists hold: the frame's list came from its re-run)


def test_resolution_mask_between_batches(ffs):
    W, H = 400, 300
    img, _ = make_frame(W, H, np.uint16, seed=77, n_spots=80)
    ctx = _ctx(ffs, W, H, np.uint16, 3, 6)
    ctx.set_mask(None)
    st = ctx.stream()
    _check(st.process(img[None]), [img], np.ones((H, W), np.uint8), 3, 6)
    ctx.apply_resolution_mask(1.0, 0.2, 200.0, 150.0, 75e-6, 75e-6, dmin=15.0, dmax=-1.0)   # (d = 15 A about 178 px out)
    mask = ctx.get_mask()
    assert 0 < mask.sum() < W * H
    _check(st.process(img[None]), [img], mask, 3, 6)


def test_window_changed_between_batches_in_flight(ffs):
    """One context, three streams in flight: the window is a per-batch snapshot taken at submit; FFS_PATH_WINDOW follows it."""
    W, H = 520, 120
    frames = np.stack([make_frame(W, H, np.uint16, seed=90 + i, n_spots=40)[0] for i in range(2)])
    mask = np.ones((H, W), np.uint8)
    ctx = _ctx(ffs, W, H, np.uint16, 6, 1, max_batch=2)
    a, b, c = ctx.stream(), ctx.stream(), ctx.stream()
    a.submit(frames)
    ctx.set_params(kernel_half_x=2, kernel_half_y=2)
    b.submit(frames)
    ctx.set_params(kernel_half_x=3, kernel_half_y=3)
    c.submit(frames)
    _check(a.wait(), frames, mask, 6, 1)
    _check(b.wait(), frames, mask, 2, 2)
    _check(c.wait(), frames, mask, 3, 3)
    assert "window" in a.last_path()[0] and "window" in b.last_path()[0]
    assert "window" not in c.last_path()[0]          # the default window keeps the 7x7 streaming kernels
    ctx.set_params(kernel_half_x=0, kernel_half_y=0)  # 0 means 3
    _check(c.process(frames), frames, mask, 3, 3)
    assert "window" not in c.last_path()[0]


def test_refusals(ffs):
    ctx = ffs.Context(64, 64, np.uint16)
    for kw in (dict(kernel_half_x=8), dict(kernel_half_y=-1), dict(kernel_half_x=1, kernel_half_y=1, min_count=10),
               dict(kernel_half_x=5, algorithm=ffs.ALGO_DISPERSION_EXTENDED)):
        ctx2 = ffs.Context(64, 64, np.uint16)
        with pytest.raises(ffs.FfsError):
            ctx2.set_params(**kw)
    ctx.set_params(kernel_half_x=1, kernel_half_y=1, min_count=9)   # (2kx+1)(2ky+1) itself is allowed
    ctx.set_params(kernel_half_x=7, kernel_half_y=7, min_count=225)


@pytest.mark.parametrize("kx,ky", [(2, 5), (5, 5)], ids=["2x5", "5x5"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_tie_cells(ffs, kx, ky, dtype):
    """Cells of (2kx+1) x (2ky+1) at the signal and dispersion ties and at min_count (tie_windows families a, b, f)."""
    prm = T.Params(min_count=(2 * kx + 1) * (2 * ky + 1) // 2)
    img, mask, cells = WT.frame(kx, ky, dtype, prm)
    H, W = img.shape
    strong = O.dispersion(img, mask, _disp(kx, ky, prm.min_count))
    sides = {(c.family, c.side) for c in cells}
    assert {("a", "at"), ("b", "at"), ("f", "at"), ("f", "below")} <= sides
    for c in cells:
        assert bool(strong[c.row, c.col]) == c.exact == c.f64, (c.family, c.side, c.m, c.x, c.y, c.p)
    for tuning in ({}, {"sparse_stage": 1}):
        ctx = _ctx(ffs, W, H, dtype, kx, ky, tuning=tuning, min_count=prm.min_count)
        ctx.set_mask(mask)
        _check(ctx.stream().process(img[None]), [img], mask, kx, ky, prm.min_count)
    ctx = _ctx(ffs, W, H, dtype, kx, ky, tuning={"threshold_path": 2}, min_count=prm.min_count)
    ctx.set_mask(mask)
    _check(ctx.stream().process(img[None]), [img], mask, kx, ky, prm.min_count)


def test_fullsize_eiger_pair_5x5(ffs):
    from ffs_amd import synth
    p = synth.params(4148, 4362, np.uint16, seed=2000, background=1.0, n_spots=400)
    frames = synth.frames(p, range(2))
    mask = synth.mask_modules(4148, 4362, 1030, 514, 10, 37)
    ctx = _ctx(ffs, 4148, 4362, np.uint16, 5, 5, max_batch=2, want_mask=0, want_list=1)
    ctx.set_mask(mask)
    st = ctx.stream()
    _check(st.process(frames), frames, mask, 5, 5)
    assert "window" in st.last_path()[0]


def test_stack3d_at_2x2(ffs):
    """3D sweep: ffs_stack3d_add_batch reads the batch's lists; the result equals O.cc3d fed the oracle's own 2,2 lists."""
    from ffs_amd import synth
    W, H, NZ = 300, 200, 10
    p = synth.sweep_params(seed=78, n_frames=NZ, n_spots=60, width=W, height=H)
    frames = synth.frames(p, range(NZ))
    mask = np.ones((H, W), np.uint8)
    ctx = ffs.Context(W, H, np.uint16, max_batch=5)
    ctx.set_params(min_spot_size_3d=3, kernel_half_x=2, kernel_half_y=2)
    st = ctx.stream()
    stack = ffs.Stack3D(ctx)
    for z0 in range(0, NZ, 5):
        st.process(frames[z0:z0 + 5], first_frame_id=z0)
        stack.add_batch(st)
    refl, n_calc, fs, fp = stack.finish()
    slices = []
    for img in frames:
        cc = O.cc2d(O.dispersion(img, mask, _disp(2, 2)), img, 3)
        slices.append((cc.k.astype(np.uint32), cc.intensity))
    want = O.cc3d(slices, W, H, 3, 2.0)
    assert n_calc == want.n_calculated and fs == want.n_filtered_size and fp == want.n_filtered_sep
    from util import assert_reflections_equal
    assert_reflections_equal(refl, want.reflections)
    assert len(refl) > 5
