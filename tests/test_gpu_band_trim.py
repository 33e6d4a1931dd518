"""The streaming threshold kernels trim the rows a mask leaves without a valid pixel off their bands' two ends (csrc/launch_geometry.hpp:
trim_band).  Held to the oracle on one small geometry -- 1203 x 517, seven bands of 74 rows (tuning `stream_bands`),
batches of four frames, so the super row has separator groups and a partly filled last strip -- with a mask that holds every shape of
run that can go wrong, and spots planted on the valid rows next to each run so that their 7x7 windows straddle it:

  rows   0 ..   4   a run at the frame's first rows
  rows  68 ..  79   a run over a band boundary (74): band 0 ends early, band 1 starts late
  rows 148 .. 221   a run that is exactly band 2: its waves do nothing, band 3 starts on its own first row
  rows 250 .. 259   a run strictly inside band 3: untouched
  rows 360 .. 368, 370 .. 380   one valid row (369, band 4's last) between two runs: band 4 keeps its end, band 5 starts at 381
  rows 436 .. 443, 445 .. 450   band 5 ends early; row 444, band 6's first, is valid, so the run behind it stays inside
  rows 510 .. 516   a run at the frame's last rows

and a second mask with more runs (21) than the kernels' arguments hold (16).  Paths: 16-bit standard (wave logs with the band stage, and
with the pixel lists), 16-bit extended (the first pass's plane too), 32-bit (with pixels >= 2^24 next to the runs), and 16-bit with the
strong byte mask (the kernels that zero-fill it keep the whole band: the rows inside the runs must be zero, whatever the batch before
left there).  The mask changes between batches on one stream: the runs travel with each launch."""
import numpy as np
import pytest

from oracle import oracle as O
from util import assert_frame_matches_oracle, oracle_frame

pytestmark = pytest.mark.gpu

W, H, BANDS, ROWS = 1203, 517, 7, 74
RUNS = [(0, 5), (68, 80), (148, 222), (250, 260), (360, 369), (370, 381), (436, 444), (445, 451), (510, 517)]   # (first, end)
SHORT = [(y, y + 2) for y in range(84, 140, 6)] + [(294, 296), (300, 302)]   # twelve two-row runs more, one of them band 3's last rows


def build_mask(runs, seed):
    rng = np.random.default_rng(seed)
    mask = np.ones((H, W), np.uint8)
    mask[:, 496:500] = 0
    mask[rng.random((H, W)) < 0.001] = 0
    for first, end in runs:
        mask[first:end] = 0
    mask[369, :] = 0; mask[369, 700:900] = 1    # the single valid row: a part of it
    return mask


def build_frames(dtype, n, seed):
    """Spots on the last valid rows before every run and the first valid rows behind it, one to four rows out, at columns that move with
    the frame; saturated cores next to two runs; 32-bit pixels: one pixel >= 2^24 on the rows that touch a run."""
    rng = np.random.default_rng(seed)
    hi = 60000 if dtype == np.uint16 else 900000
    frames = []
    for f in range(n):
        img = rng.poisson(2.0, (H, W)).astype(dtype)
        for _ in range(60):
            y, x = rng.integers(0, H - 4), rng.integers(0, W - 6)
            img[y:y + rng.integers(1, 4), x:x + rng.integers(1, 6)] = rng.integers(200, 3000)
        for k, (first, end) in enumerate(RUNS + SHORT):
            for d in range(1, 5):
                x = 30 + 97 * ((k + 3 * f) % 11) + 13 * d
                for y in (first - d, end + d - 1):
                    if 0 <= y < H:
                        img[y, x] = 400 + 100 * d
                        xb, xc = (x + 300) % 1100, (x + 520) % 1100
                        img[y, xb:xb + d] = 900                        # a short bar
                        if d == 2:
                            img[max(y - 1, 0):y + 2, xc:xc + 3] = 1500   # a 3x3 blob over the rows around it
        img[369, 700:900:7] = 700                                   # the single valid row between two runs
        img[64:68, 200 + 50 * f:206 + 50 * f] = rng.integers(hi // 3, hi)     # window sums >= 65536 next to a run
        img[222:226, 820 + 50 * f:826 + 50 * f] = rng.integers(hi // 3, hi)
        if dtype == np.uint32:
            img[67, 900 + f] = 1 << 24                                # the window rule for 32-bit pixels, next to the runs
            img[80, 40 + f] = (1 << 24) + 5
            img[222, 600 + f] = 1 << 25
            img[381, 610 + f] = 1 << 24
        frames.append(img)
    frames[-1][:] = rng.poisson(2.0, (H, W)).astype(dtype)           # ... and a frame with nothing on it
    return np.stack(frames)


_cache = {}


def case(dtype, which):
    """(frames, mask, what the oracle finds in each frame) -- computed once a mask and pixel type"""
    key = (np.dtype(dtype).name, which)
    if key not in _cache:
        mask = {"runs": build_mask(RUNS, 1), "many": build_mask(RUNS + SHORT, 2), "none": build_mask([], 3)}[which]
        frames = build_frames(dtype, 4, 11)
        _cache[key] = (frames, mask, [oracle_frame(img, mask, min_spot_size=1) for img in frames])
    return _cache[key]


def context(ffs, dtype, mask, **params):
    ctx = ffs.Context(W, H, dtype, max_batch=4)
    ctx.set_tuning(stream_bands=BANDS)
    ctx.set_mask(mask)
    ctx.set_params(min_spot_size=1, **params)
    return ctx


def check(res, frames, mask, want):
    for fr, img, w in zip(res, frames, want):
        assert_frame_matches_oracle(fr, img, mask, min_spot_size=1, precomputed=w)


def test_the_masks_hold_the_shapes():
    for which, n_runs in (("runs", 9), ("many", 21)):
        mask = case(np.uint16, which)[1]
        empty = ~mask.any(axis=1)
        starts = [y for y in range(H) if empty[y] and (y == 0 or not empty[y - 1])]
        assert len(starts) == n_runs
    empty = ~case(np.uint16, "runs")[1].any(axis=1)
    assert -(-H // BANDS) == ROWS
    assert empty[2 * ROWS:3 * ROWS].all() and not empty[2 * ROWS - 1] and not empty[3 * ROWS]      # exactly one band
    assert empty[ROWS - 1] and empty[ROWS]                                                          # over a boundary
    assert not empty[5 * ROWS - 1] and empty[5 * ROWS - 2] and empty[5 * ROWS]                      # one valid row between two runs
    assert not case(np.uint16, "none")[1].all(axis=1).any() and case(np.uint16, "none")[1].any(axis=1).all()
    assert all(w[1].num_strong_pixels > 50 for w in case(np.uint16, "runs")[2][:3])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
@pytest.mark.parametrize("which", ["runs", "many"])
def test_standard_matches_oracle(ffs, dtype, which):
    frames, mask, want = case(dtype, which)
    ctx = context(ffs, dtype, mask, want_strong_list=0)
    st = ctx.stream()
    for rep in range(2):
        order = np.roll(np.arange(len(frames)), rep)          # (a frame's place in the super row moves: other strips)
        res = st.process(frames[order])
        path, reruns = st.last_path()
        assert "bands" in path and "wave_logs" in path and reruns == 0, (path, reruns)
        check(res, frames[order], mask, [want[i] for i in order])
    res = st.process(frames[:3])                               # three frames: other strips, another last one
    check(res, frames[:3], mask, want[:3])
    ctx.set_params(min_spot_size=1, want_strong_list=1)        # the pixel lists: the one-workgroup launch reads the logs
    res = st.process(frames)
    assert "bands" not in st.last_path()[0]
    check(res, frames, mask, want)
    ctx.set_tuning(strong_log=0)                               # ... and without wave logs: plane bytes, counters and the occupancy bitmap
    res = st.process(frames)
    assert "wave_logs" not in st.last_path()[0]
    check(res, frames, mask, want)


@pytest.mark.parametrize("which", ["runs", "many"])
def test_extended_matches_oracle(ffs, which):
    frames, mask, _ = case(np.uint16, which)
    ctx = context(ffs, np.uint16, mask, algorithm=ffs.ALGO_DISPERSION_EXTENDED)
    st = ctx.stream()
    res = st.process(frames)
    for f, (fr, img) in enumerate(zip(res, frames)):
        strong, first, eroded = O.dispersion_extended(img, mask, debug=True)
        assert np.array_equal(st.debug_bitplane(f, 1), first), f        # the first pass's plane: the streaming kernel's own output
        assert_frame_matches_oracle(fr, img, mask, min_spot_size=1, strong=strong)


def test_byte_mask_is_whole_and_follows_the_mask(ffs):
    """want_strong_mask: the kernels that zero-fill the byte mask.  The batch before (no runs) leaves strong bytes on the rows the next
    mask empties; the whole byte mask must equal the oracle's each time.  Then back and forth without the byte mask: a mask with runs, one
    without, one with more runs than the arguments hold, on one stream."""
    frames, m_runs, w_runs = case(np.uint16, "runs")
    _, m_none, w_none = case(np.uint16, "none")
    _, m_many, w_many = case(np.uint16, "many")
    assert any(w[0][150:220].any() for w in w_none)            # strong pixels where the other masks have their longest run
    ctx = context(ffs, np.uint16, m_none, want_strong_mask=1)
    st = ctx.stream()
    for mask, want in ((m_none, w_none), (m_runs, w_runs), (m_none, w_none), (m_many, w_many)):
        ctx.set_mask(mask)
        res = st.process(frames)
        assert all(fr.strong_mask is not None for fr in res)
        check(res, frames, mask, want)
    ctx.set_params(min_spot_size=1, want_strong_mask=0, want_strong_list=0)
    for mask, want in ((m_runs, w_runs), (m_none, w_none), (m_runs, w_runs), (m_many, w_many), (m_none, w_none)):
        ctx.set_mask(mask)
        res = st.process(frames)
        assert "bands" in st.last_path()[0]
        check(res, frames, mask, want)


def test_resolution_mask_rebuilds_the_runs(ffs):
    """The resolution mask is made on the device: the runs are derived from the plane there.  A d_min that empties the frame's upper
    and lower rows (the beam centre in the middle), set on top of the mask with runs."""
    frames, m_runs, _ = case(np.uint16, "runs")
    ctx = context(ffs, np.uint16, m_runs, want_strong_list=0)
    st = ctx.stream()
    st.process(frames)
    # (1 A, 0.2 m, 75 um pixels: 12.3 A lies 217 pixels from the beam centre)
    ctx.apply_resolution_mask(1.0, 0.2, W / 2.0, H / 2.0, 75e-6, 75e-6, dmin=12.3)
    mask = ctx.get_mask()
    empty = ~mask.any(axis=1)
    assert empty[:30].all() and empty[-30:].all() and not empty[60:68].any() and not empty[230:250].any()
    res = st.process(frames)
    for fr, img in zip(res, frames):
        assert_frame_matches_oracle(fr, img, mask, min_spot_size=1)
