"""GPU: what one batch leaves behind on a stream, read by the next -- every ordered pair of batch kinds (tests/batch_walk.py), every
frame of every batch against the oracle.

The path of a batch follows its parameters, the context's tuning, the pipeline depth and what the stream's earlier batches left:
dirty plane / counts / occupancy, the extended planes that take turns, the byte mask that is zero-filled only when asked for,
`dense_batch`, the sticky decisions of ffs_wait (flags 32, 16, 128, the kept one-frame stream), tables per mask and window.  The
rest of the suite meets each path on a fresh context; here one stream walks a de Bruijn sequence over the kinds, so that each kind
follows each kind (itself included) once -- on a fresh stream, on a stream whose wave logs are off for good (flag 32), on one whose
run-based launch is (flag 16), and with a 3D stack alive.  Then: a failed or refused batch as the predecessor of every kind, and the
kinds that parameters alone tell apart in flight together on the streams of one context."""
import contextlib
import time

import numpy as np
import pytest

import batch_walk as BW
from oracle import oracle as O
from util import _blob_frame, _resident, assert_frame_matches_oracle, assert_reflections_equal, oracle_frame

pytestmark = pytest.mark.gpu

W, H = BW.W, BW.H
SPARSE_LAUNCHES = {"frame_chain", "bands", "grid_kernels"}      # a batch's sparse stage is exactly one of them
ALL_PATHS = {"wave_logs", "frame_chain", "bands", "runs", "grid_kernels", "extended", "window"}


@pytest.fixture(scope="module")
def want():
    return BW.OracleCache()


@contextlib.contextmanager
def _at(*where):
    """A failure names its place: (state, step, previous kind, kind[, frame])."""
    try:
        yield
    except (AssertionError, RuntimeError) as e:
        raise AssertionError(f"{where}: {e}") from e


def _context(ffs):
    from ffs_amd import bslz4
    ctx = ffs.Context(W, H, np.uint16, max_batch=BW.MAX_BATCH, max_strong_per_frame=BW.MAX_STRONG)
    return ctx, BW.Walker(ctx, resident=_resident, compress=bslz4.compress)


def _check_batch(st, kind, res, first_id, want, where, stack_alive=False):
    """One batch of `kind` as it came back from `st`: every frame, the frame ids, the history-independent path bits, the planes of the
    extended algorithm.  Returns (path, reruns)."""
    path, reruns = st.last_path()
    p = kind.all_params
    with _at(*where):
        assert [r.frame_id for r in res] == list(range(first_id, first_id + len(kind.frames)))
        assert path <= ALL_PATHS and len(path & SPARSE_LAUNCHES) == 1, path
        assert ("extended" in path) == kind.extended and ("window" in path) == kind.window, path
        if kind.all_tuning["sparse_stage"] == 1:
            assert "grid_kernels" in path, path
        if kind.all_tuning["strong_log"] == 0 or kind.all_tuning["threshold_path"] != 0 or kind.extended or kind.window:
            assert "wave_logs" not in path, path
        if kind.wants_lists_or_bytes or stack_alive:
            assert "bands" not in path, path
        if "runs" in path:
            assert "frame_chain" in path and "wave_logs" not in path, path
    mask = BW.masks()[kind.mask]
    for f, fr in enumerate(res):
        with _at(*where, f"frame {f}"):
            w = want(kind, f)
            # what was asked for came back (and is compared), what was not did not
            assert (fr.strong_k is not None) == bool(p["want_strong_list"]) and (fr.strong_mask is not None) == bool(p["want_strong_mask"])
            assert fr.reflections is not None
            assert_frame_matches_oracle(fr, BW.frame(kind.frames[f]), mask, precomputed=w.precomputed)
            if kind.extended:       # the planes that take turns between the batches of a stream
                assert np.array_equal(st.debug_bitplane(f, 1), w.first), "first-pass plane"
                assert np.array_equal(st.debug_bitplane(f, 2), w.eroded), "eroded signal region"
    return path, reruns


def _history_bits(state, prev_dense, kind):
    """What the documented history says about the batch's path (ffs_submit.hip, plan_batch): the wave logs serve the standard 16-bit path of
    the one launch unless the stream's PREVIOUS batch held a frame beyond the LDS forest or flag 32 switched them off; a batch behind
    such a frame takes the run-based launch unless flag 16 switched that off, and then the grid-wide kernels.  (A batch that is run
    again reports its second pass, which follows its OWN counts: a dense batch that arrived on the logs reports the run-based launch.)
    -> {bit: expected}"""
    t = kind.all_tuning
    dense_data = kind.name in ("dense", "overflow")
    one_launch = t["sparse_stage"] == 2
    logs = (one_launch and not kind.extended and not kind.window and t["threshold_path"] == 0 and t["strong_log"] == 1
            and not prev_dense and state != "after_flag32")
    behind_dense = prev_dense or (dense_data and logs)          # (the second pass of a dense batch that arrived on the logs)
    runs = one_launch and behind_dense and state != "after_flag16"
    grid = not one_launch or (behind_dense and state == "after_flag16")
    return {"wave_logs": logs and not dense_data, "runs": runs, "grid_kernels": grid}


# ---- a. the walk on one stream, in four stream states ----------------------------------------------------------------------------
def _busy_frames():
    """Frames whose streaming waves find more strong groups than a wave's log holds (256): flag 32.  Built as
    test_wave_log_of_several_register_runs builds its frames, with eight times the spots per pixel, in the frame's first 480 rows."""
    rng = np.random.default_rng(12)
    frames = []
    for _ in range(2):
        img = rng.poisson(2.0, (H, W)).astype(np.uint16)
        for _ in range(4000):
            y, x = rng.integers(0, 480 - 3), rng.integers(0, W - 3)
            img[y:y + rng.integers(1, 3), x:x + rng.integers(1, 4)] = rng.integers(200, 3000)
        for _ in range(6):
            y, x = rng.integers(0, 480 - 8), rng.integers(0, W - 8)
            img[y:y + 6, x:x + 6] = rng.integers(20000, 65535)
        frames.append(img)
    return np.stack(frames)


def _enter_state(ffs, state, ctx, st):
    """What the stream has processed before the walk.  Returns the 3D stack of the `stack` state."""
    ones = np.ones((H, W), np.uint8)
    if state == "after_flag32":
        frames = _busy_frames()
        ctx.set_params(want_strong_list=1, want_reflections=1, min_spot_size=1)
        res = st.process(frames, first_frame_id=0)
        path, reruns = st.last_path()
        assert reruns == 1 and "wave_logs" not in path, (path, reruns)
        for fr, img in zip(res, frames):
            assert 3000 < fr.num_strong_pixels < BW.CHAIN_LDS_ENTRIES       # (not the dense fall-back of flag 64: the logs themselves overflowed)
            assert_frame_matches_oracle(fr, img, ones, min_spot_size=1)
    elif state == "after_flag16":
        rng = np.random.default_rng(17)
        noisy = rng.poisson(1.0, (H, W)).astype(np.uint16)
        noisy[rng.random((H, W)) < 0.024] += 60                             # ~27 k isolated strong pixels: as many runs
        frames = np.stack([noisy, _blob_frame(W, H, 62, 520)])
        wants = [oracle_frame(img, ones, min_spot_size=1) for img in frames]
        assert BW.run_counts(wants[0][0])[0] > BW.CHAIN_MAX_RUNS and wants[0][1].num_strong_pixels <= BW.MAX_STRONG
        # The noisy batch must not arrive on the wave logs (its waves would overflow them: flag 32 as well, the state of the walk before
        # this one): behind a dense batch that the logs can carry it takes the run-based launch directly, and overflows only that.
        dense = np.stack([BW.frame(n) for n in BW.BY_NAME["dense"].frames])
        ctx.set_params(want_reflections=1)
        for fr, img in zip(st.process(dense), dense):
            assert_frame_matches_oracle(fr, img, ones)
        path, reruns = st.last_path()                                       # (flag 64: again through the plane; the logs stay)
        assert path == {"frame_chain", "runs"} and reruns >= 1, (path, reruns)
        ctx.set_params(want_reflections=1, min_spot_size=1)
        seen = []
        for rep in range(2):
            res = st.process(frames, first_frame_id=2 * rep)
            seen.append(st.last_path())
            for fr, img, w in zip(res, frames, wants):
                assert_frame_matches_oracle(fr, img, ones, min_spot_size=1, precomputed=w)
        assert seen[0] == ({"grid_kernels"}, 1), seen                       # the run-based launch overflowed: again through the grid-wide kernels
        assert seen[1] == ({"grid_kernels"}, 0), seen                       # ... and the stream goes there directly from then on
    elif state == "stack":
        return ffs.Stack3D(ctx)
    else:
        assert state == "fresh"
    return None


def _run_walk(ffs, want, state):
    """The walk over all kinds on one stream in `state` -> ({(previous kind, kind): (path set, reruns)}, the same in walk order)."""
    ctx, walker = _context(ffs)
    st = ctx.stream()
    stack = _enter_state(ffs, state, ctx, st)
    table, order, slices = {}, [], []
    prev_dense = state == "after_flag16"                                     # (that state's last batch held 27 k strong pixels)
    steps = BW.walk()
    for step, (prev, kind) in enumerate(steps):
        where = (state, step, prev.name if prev else None, kind.name)
        first_id = 1000 + 3 * step                                           # strictly increasing, gaps behind the short batches
        with _at(*where):
            res = walker.run(st, kind, first_id)
        path, reruns = _check_batch(st, kind, res, first_id, want, where, stack_alive=stack is not None)
        with _at(*where, "path", sorted(path), reruns):
            for bit, expected in _history_bits(state, prev_dense, kind).items():
                assert (bit in path) == expected, bit
        prev_dense = kind.name in ("dense", "overflow")
        order.append((kind.name, frozenset(path), reruns))
        if prev is not None:
            assert (prev.name, kind.name) not in table
            table[(prev.name, kind.name)] = (frozenset(path), reruns)
        if stack is not None and kind.name not in ("dense", "overflow"):
            with _at(*where, "add_batch"):
                stack.add_batch(st)
            slices += [(want(kind, f).cc.k, want(kind, f).cc.intensity) for f in range(len(kind.frames))]
    n = len(BW.KINDS)
    assert n >= 19 and len(table) == n * n and len(steps) == n * n + 1      # all N^2 pairs ran on this stream
    if state == "fresh":
        assert order[0][1:] == (frozenset({"wave_logs", "bands"}), 0), order[0]       # the shape is one the default kind takes the hot path on
    if stack is not None:
        # the 3D components of everything the stack took, against the oracle's labelling of the ORACLE's lists of those frames
        walker.prepare(BW.BY_NAME["default"])
        refl, n_calc, fs, fp = stack.finish()
        w3 = O.cc3d(slices, W, H, BW.DEFAULT_PARAMS["min_spot_size_3d"], BW.DEFAULT_PARAMS["max_peak_centroid_separation"])
        with _at(state, "finish", len(slices)):
            assert (n_calc, fs, fp) == (w3.n_calculated, w3.n_filtered_size, w3.n_filtered_sep)
            assert len(refl) > 100
            assert_reflections_equal(refl, w3.reflections)
        stack.close()
    st.close()
    ctx.close()
    return table, order


def _summary(table):
    """The table in a few lines (DESIGN.md section 9 quotes them)."""
    sets = {}
    for (prev, kind), (path, reruns) in table.items():
        sets.setdefault(path, []).append((prev, kind))
    lines = [f"{len(table)} pairs, {len(sets)} distinct path sets"]
    for path, pairs in sorted(sets.items(), key=lambda kv: -len(kv[1])):
        lines.append(f"  {len(pairs):4d}  {'+'.join(sorted(path))}   kinds: {','.join(sorted({k for _, k in pairs}))}")
    for r in sorted({r for _, r in table.values()} - {0}):
        pairs = sorted(pk for pk, (_, rr) in table.items() if rr == r)
        lines.append(f"  reruns == {r}: " + ", ".join(f"{a}->{b}" for a, b in pairs))
    return "\n".join(lines)


_tables = {}


def _fresh_table(ffs, want):
    if "fresh" not in _tables:
        _tables["fresh"] = _run_walk(ffs, want, "fresh")
    return _tables["fresh"]


def test_walk_on_a_fresh_stream(ffs, want):
    t0 = time.time()
    table, order = _fresh_table(ffs, want)
    print(_summary(table))
    print(f"walk: {time.time() - t0:.1f} s")
    # coverage: the walk exercised what it is there for
    seen = set().union(*(path for path, _ in table.values()))
    assert seen == ALL_PATHS, ALL_PATHS - seen
    assert any(reruns == 1 for _, reruns in table.values())                 # a dense batch that arrived on the logs (flag 64)
    assert any("bands" in order[i][1] and "bands" not in order[i - 1][1] for i in range(1, len(order))), "bands never came back"
    # the logs are back after dense data: not in the batch right behind it (a batch's path follows what the batch BEFORE it held, so that one
    # takes the plane), but in the one after
    assert any(order[i][0] == "dense" and "wave_logs" in order[i + 2][1] for i in range(len(order) - 2)), "the logs never came back after dense data"
    assert "runs" in table[("dense", "dense")][0]


def test_walk_is_repeatable(ffs, want):
    """The plan follows the documented history alone: the same walk on a second fresh context takes the same paths and re-runs."""
    first, _ = _fresh_table(ffs, want)
    second, _ = _run_walk(ffs, want, "fresh")
    diff = {pk: (first[pk], second[pk]) for pk in first if first[pk] != second[pk]}
    assert not diff, diff


@pytest.mark.parametrize("third", ["compressed", "default", "device_in"])
def test_plan_reads_the_previous_batch_alone(ffs, want, third):
    """dense (3 frames), short (1 frame), then three frames again: frames 1 and 2 of the DENSE batch's counts are still in the stream's
    host counters, and the third batch must not take them for the previous batch's (ffs_submit_compressed used to set the stream's
    frame count before the batch was planned, so a compressed batch did: it went to the run-based launch instead of the logs)."""
    ctx, walker = _context(ffs)
    st = ctx.stream()
    for step, name in enumerate(["default", "dense", "short", third]):
        kind = BW.BY_NAME[name]
        res = walker.run(st, kind, 10 * step)
        path, reruns = _check_batch(st, kind, res, 10 * step, want, ("plan", step, name))
    assert "wave_logs" in path and "runs" not in path and reruns == 0, (path, reruns)


def test_walk_after_the_wave_logs_overflowed(ffs, want):
    """Flag 32 is for good: no batch of the walk is given wave logs (or the bands that read them) again, and every one is right."""
    table, _ = _run_walk(ffs, want, "after_flag32")
    print(_summary(table))
    assert not any({"wave_logs", "bands"} & path for path, _ in table.values())


def test_walk_after_the_run_based_launch_overflowed(ffs, want):
    """Flag 16 is for good: dense batches take the grid-wide kernels, none the run-based launch."""
    table, _ = _run_walk(ffs, want, "after_flag16")
    print(_summary(table))
    assert not any("runs" in path for path, _ in table.values())
    assert "grid_kernels" in table[("dense", "dense")][0]
    assert any("wave_logs" in path for path, _ in table.values())          # (the logs are a decision of their own: still on)


def test_walk_with_a_stack_alive(ffs, want):
    """A 3D stack alive for the whole walk: every batch keeps its lists on the device (no bands), and the stack's components are the
    oracle's for the oracle's lists."""
    table, _ = _run_walk(ffs, want, "stack")
    print(_summary(table))


# ---- b. a refused or failed batch is also a predecessor --------------------------------------------------------------------------
def _corrupt_chunk(img):
    """test_bad_chunks_are_refused's construction: the first sequence of the first block becomes "no literals, then a match" whose offset
    points before the start of the block.  The decode kernel flags the block and leaves zeros; ffs_wait reports it."""
    from ffs_amd import bslz4
    bad = bytearray(bslz4.compress(img))
    bad[16], bad[17], bad[18] = 0x0F, 0xFF, 0xFF
    return bytes(bad)


@pytest.mark.parametrize("failure", ["corrupt_payload", "wrong_header", "too_many_frames"])
def test_failed_batch_then_every_kind(ffs, want, failure):
    from ffs_amd import bslz4
    ctx, walker = _context(ffs)
    st = ctx.stream()
    names = BW.BY_NAME["compressed"].frames
    good = [bslz4.compress(BW.frame(n)) for n in names]
    prev = None
    for step, kind in enumerate(BW.KINDS):
        where = (failure, step, prev, kind.name)
        # the batch that fails runs under the parameters, tuning and mask of the kind before (the first: the context's defaults)
        with _at(*where, "the failing batch"):
            if failure == "corrupt_payload":
                st.submit_compressed([good[0], _corrupt_chunk(BW.frame(names[1])), good[2]], first_frame_id=7)
                with pytest.raises(ffs.FfsError, match="corrupt"):
                    st.wait()
            elif failure == "wrong_header":
                with pytest.raises(ffs.FfsError, match="header says"):
                    st.submit_compressed([good[0], bslz4.compress(BW.frame(names[1])[:50])], first_frame_id=7)
            else:
                with pytest.raises(ffs.FfsError, match="max_batch"):
                    st.submit(np.zeros((BW.MAX_BATCH + 1, H, W), np.uint16), first_frame_id=7)
            if failure != "corrupt_payload":
                with pytest.raises(ffs.FfsError, match="nothing submitted"):
                    st.wait()                                                # refused at submit: nothing is in flight
        first_id = 50 + 3 * step
        with _at(*where):
            res = walker.run(st, kind, first_id)
        _check_batch(st, kind, res, first_id, want, where)
        prev = kind.name


# ---- c. transitions with batches in flight ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [4, 2])
def test_transitions_with_batches_in_flight(ffs, want, n_streams):
    """The kinds that parameters, data, input form and batch length tell apart (tuning and mask stay as they are while anything is in
    flight: the parameter snapshot at submit is what the header promises), on the streams of ONE context, each stream at its own
    offset into the sequence: batches of different algorithms, windows and outputs are in flight together, and each stream still
    sees every ordered pair.  Four streams: bands at every depth; two: the one-workgroup launch with `chain_first` for the second."""
    kinds = BW.in_flight_kinds()
    n = len(kinds)
    ctx, walker = _context(ffs)
    ctx.set_tuning(**BW.DEFAULT_TUNING)
    ctx.set_mask(BW.masks()[0])
    streams = [ctx.stream() for _ in range(n_streams)]
    walks = [BW.walk(kinds, i * (n * n // 4)) for i in range(n_streams)]
    paths = set()
    for rnd in range(n * n + 1):
        ids = [10 * (rnd * n_streams + i) for i in range(n_streams)]
        for i, st in enumerate(streams):
            prev, kind = walks[i][rnd]
            with _at(n_streams, i, rnd, prev.name if prev else None, kind.name, "submit"):
                walker.prepare(kind, tuning=False, mask=False)
                walker.submit(st, kind, ids[i])
        for i, st in enumerate(streams):
            prev, kind = walks[i][rnd]
            where = (f"{n_streams} streams, stream {i}", rnd, prev.name if prev else None, kind.name)
            with _at(*where):
                res = st.wait()
            path, _ = _check_batch(st, kind, res, ids[i], want, where)
            paths.add(frozenset(path))
    assert any("bands" in p for p in paths) and any("frame_chain" in p for p in paths) and any("extended" in p for p in paths)
    assert any("window" in p for p in paths)
