"""GPU: k_bshuf_lz4_decode (csrc/kernels_decode.hpp) on the hand-built LZ4 blocks of tests/lz4_blocks.py -- sequence structures no
encoder is known to emit: length fields that end on either side of every reload of the parser's 8-byte window, tokens at every
address mod 4, the three match-copy loops at their switching points, in-place literal copies below, at and above the 64-lane stride,
and one input per bounds check.

A case is one block of a small frame (u16 97 x 127: three full blocks, 24 elements, 7 raw; u32 61 x 101: three full blocks, 16
elements, 1 raw) whose other blocks are fillers chosen so that the case's bytes begin at every residue mod 4.  The expected frame is
the model decoder's output un-shuffled (lz4_blocks.frame); tests/test_lz4_blocks.py holds that model to liblz4.  Every comparison is
bit for bit.  Class A must decode; class B (blocks liblz4 refuses but a lenient decoder reads) may decode, then to the model's pixels,
or be refused as corrupt; class C must be refused, by the kernel ("corrupt") or by the host's planning ("run past", "header")."""
from collections import Counter

import numpy as np
import pytest

import lz4_blocks as L
from util import assert_frame_matches_oracle

pytestmark = pytest.mark.gpu
BATCH = 128
KEYS = list(L.FRAMES)


def _assert_same(got, want, what):
    d = np.argwhere(got != want)
    assert d.size == 0, f"{what}: {len(d)} pixels differ, first at (y, x) = {tuple(d[0])}: got {got[tuple(d[0])]}, want {want[tuple(d[0])]}"


def _assert_refused(ffs, st, chunks, word, what):
    try:
        st.decode_only(chunks)
    except ffs.FfsError as e:
        assert word in str(e), f"{what}: refused with another text: {e}"
        return
    raise AssertionError(f"{what}: decoded without a refusal")


def _stream(ffs, key, max_batch):
    W, H, dtype = L.FRAMES[key]
    return ffs.Context(W, H, dtype, max_batch=max_batch).stream()


@pytest.mark.parametrize("key", KEYS)
def test_class_a_decodes_to_the_models_pixels(ffs, key):
    """Every conforming case, four times: as full block 0, 1 or 2 (short cases: as the last block) and at a byte offset of each
    residue mod 4, 128 frames per launch."""
    cases = L.cases_for(key, "A")
    st = _stream(ffs, key, BATCH)
    seen, frames = Counter(), 0
    for rot in range(4):
        built = [(c, (i + rot) % 3) + L.chunk_with(key, c, (i + rot) % 3, (i + rot) % 4) for i, c in enumerate(cases)]
        for b in range(0, len(built), BATCH):
            part = built[b:b + BATCH]
            try:
                _, got = st.decode_only([p[2] for p in part])
            except ffs.FfsError:      # a conforming block was refused: find out which, one call per case
                refused = []
                for c, pos, chunk, _, res in part:
                    try:
                        st.decode_only([chunk])
                    except ffs.FfsError as e:
                        refused.append(f"{c.name} (block {pos}, offset {res} mod 4: {c.note}): {e}")
                raise AssertionError(f"{key}: the kernel refused {len(refused)} conforming blocks: " + "; ".join(refused[:8]))
            for (c, pos, _, want, res), g in zip(part, got):
                seen[res] += 1
                frames += 1
                _assert_same(g, want, f"{key} {c.name} (block {pos}, offset {res} mod 4: {c.note})")
    print(f"{key}: class A: {len(cases)} cases in {frames} frames decoded exactly; byte offsets mod 4 seen: {dict(sorted(seen.items()))}")
    assert set(seen) == {0, 1, 2, 3}


@pytest.mark.parametrize("key", KEYS)
def test_class_b_decodes_exactly_or_is_refused(ffs, key):
    """Blocks liblz4 refuses and the host decoder reads.  The kernel guarantees: the model's pixels or a refusal, nothing else.
    Today it refuses none of them: ends_on_match, final_literals_0 .. 4, match_in_last_12 and match_off8187_len4 / len5 all decode
    (its loop ends where the input ends, after a match as well as after literals)."""
    cases = L.cases_for(key, "B")
    st = _stream(ffs, key, 1)
    refused, seen = [], Counter()
    for i, c in enumerate(cases):
        for res in range(4):
            chunk, want, got_res = L.chunk_with(key, c, 1 + (i + res) % 2, res)
            seen[got_res] += 1
            try:
                _, got = st.decode_only([chunk])
            except ffs.FfsError as e:
                assert "corrupt" in str(e), f"{key} {c.name}: {e}"
                refused.append(c.name)
                continue
            _assert_same(got[0], want, f"{key} {c.name} (offset {got_res} mod 4: {c.note})")
    print(f"{key}: class B: {len(cases)} cases, refused: {sorted(set(refused)) or 'none'}; byte offsets mod 4 seen: {dict(sorted(seen.items()))}")
    assert set(seen) == {0, 1, 2, 3}


@pytest.mark.parametrize("key", KEYS)
def test_class_c_is_refused_and_the_stream_survives(ffs, key):
    """One malformed input per call, as frame 1 of a batch whose frame 0 is good.  Each is rejected by a bounds check on reading (the
    case's note names the line); the short-block cases whose length field runs into the 0xFF tail run at every byte offset, so that
    the parser meets 1, 2, 3 and no 0xFF bytes behind the block's end."""
    st = _stream(ffs, key, 2)
    good, want, _ = L.chunk_with(key)
    n = 0
    for i, c in enumerate(L.cases_for(key, "C")):
        for res in (range(4) if c.cap < L.BLOCK else [i % 4]):
            bad, frame, _ = L.chunk_with(key, c, i % 3, res)
            assert frame is None
            _assert_refused(ffs, st, [good, bad], "corrupt", f"{key} {c.name} (offset {res} mod 4: {c.note})")
            n += 1
    for cc in L.chunk_cases(key):
        _assert_refused(ffs, st, [good, cc.data], cc.match, f"{key} {cc.name} ({cc.note})")
        n += 1
    _, got = st.decode_only([good, good])
    _assert_same(got[0], want, f"{key}: a good chunk after {n} refusals")
    _assert_same(got[1], want, f"{key}: a good chunk after {n} refusals, frame 1")
    print(f"{key}: class C: {n} inputs refused, the stream then decodes a good chunk exactly")


def test_hot_path_from_hand_built_chunks(ffs):
    """Two malformed and two conforming cases through ffs_submit_compressed: the refusals reach ffs_wait, and the conforming chunks
    give the oracle's answers for the frames they stand for."""
    key = "u16"
    W, H, dtype = L.FRAMES[key]
    by_name = {c.name: c for c in L.catalogue()}
    ctx = ffs.Context(W, H, dtype, max_batch=2)
    ctx.set_params(want_strong_mask=1, want_strong_list=1)
    st = ctx.stream()
    for name in ("offset_0", "lit_field_unterminated_longest"):
        with pytest.raises(ffs.FfsError, match="corrupt"):
            st.process_compressed([L.chunk_with(key)[0], L.chunk_with(key, by_name[name], 1, 1)[0]])
    built = [L.chunk_with(key, by_name[name], pos, 3) for name, pos in (("real_encoder", 2), ("max_expansion", 1))]
    res = st.process_compressed([b[0] for b in built], first_frame_id=5)
    assert [r.frame_id for r in res] == [5, 6]
    mask = np.ones((H, W), np.uint8)
    for fr, b in zip(res, built):
        assert_frame_matches_oracle(fr, b[1], mask)
