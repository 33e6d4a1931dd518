"""GPU: what csrc/ffs_encoded.hip does with a batch's chunks before a decode kernel sees them, for both codecs: chunks the caller placed in
two far-apart clusters of the staging area (two copies), a batch with one chunk in the staging area and one outside (refused), and a small
batch followed by one that outgrows the device-side buffers the first one sized.  The expected pixels are the frames that were encoded;
the expected spots are the oracle's.  The decisions themselves are held against literals without a GPU (test_encoded_plan.py)."""
import functools

import numpy as np
import pytest

from ffs_amd import bslz4, byteoffset
from ffs_amd.api import CODEC_BSLZ4, CODEC_BYTE_OFFSET
from util import assert_frame_matches_oracle, make_frame, oracle_frame

pytestmark = pytest.mark.gpu

N = 4   # frames of a full batch
CASES = [(67, 45, np.uint32, CODEC_BSLZ4), (67, 45, np.uint32, CODEC_BYTE_OFFSET), (200, 100, np.uint16, CODEC_BSLZ4), (200, 100, np.uint16, CODEC_BYTE_OFFSET)]
IDS = ["67x45-u32-lz4", "67x45-u32-byteoffset", "200x100-u16-lz4", "200x100-u16-byteoffset"]


@functools.lru_cache(maxsize=None)
def frames_and_oracle(W, H, dtype):
    frames = [make_frame(W, H, dtype, seed=50 + i, n_spots=12)[0] for i in range(N)]
    mask = np.ones((H, W), np.uint8)
    return frames, mask, [oracle_frame(f, mask) for f in frames]


@functools.lru_cache(maxsize=None)
def chunks_of(W, H, dtype, codec):
    encode = byteoffset.compress if codec == CODEC_BYTE_OFFSET else bslz4.compress
    return [encode(f) for f in frames_and_oracle(W, H, dtype)[0]]


def open_stream(ffs, W, H, dtype):
    ctx = ffs.Context(W, H, dtype, max_batch=N)
    ctx.set_params(want_strong_mask=1, want_strong_list=1)
    return ctx.stream()


def check_decode(st, chunks, codec, frames, what):
    _, got = st.decode_only(chunks, codec=codec)
    for i, (g, f) in enumerate(zip(got, frames)):
        assert np.array_equal(g, f), f"{what}: frame {i} differs in {int((g != f).sum())} pixels"


def check_spots(st, chunks, codec, W, H, dtype, first=0):
    frames, mask, oracle = frames_and_oracle(W, H, dtype)
    res = st.process_encoded(chunks, codec)
    assert len(res) == len(chunks)
    for i, fr in enumerate(res):
        assert_frame_matches_oracle(fr, frames[first + i], mask, precomputed=oracle[first + i])


def place(hb, chunks, offsets):
    views = []
    for c, at in zip(chunks, offsets):
        hb[at:at + len(c)] = np.frombuffer(c, np.uint8)
        views.append(hb[at:at + len(c)])
    return views


@pytest.mark.parametrize("W,H,dtype,codec", CASES, ids=IDS)
def test_two_clusters_far_apart(ffs, W, H, dtype, codec):
    """Chunks 0 and 2 at the start of the staging area, 3 and 1 (in that order) a MiB further: the gap between the clusters is more than the
    512 KiB below which copy ranges are merged, so the chunks cross in two copies and nothing of the gap does."""
    frames = frames_and_oracle(W, H, dtype)[0]
    chunks = chunks_of(W, H, dtype, codec)
    longest = max(map(len, chunks))
    far = (1 << 20) + 2 * longest
    offsets = [1, far + longest + 7, longest + 6, far + 3]
    assert offsets[3] - (offsets[2] + len(chunks[2])) > 524288 + 16
    st = open_stream(ffs, W, H, dtype)
    st.reserve_host(far + 2 * longest + 4096)
    hb = st.host_bytes()
    hb[:] = 0xA5
    views = place(hb, chunks, offsets)
    check_decode(st, views, codec, frames, "two clusters")
    check_spots(st, views, codec, W, H, dtype)


@pytest.mark.parametrize("W,H,dtype,codec", CASES, ids=IDS)
def test_mixed_placement_is_refused(ffs, W, H, dtype, codec):
    frames = frames_and_oracle(W, H, dtype)[0]
    chunks = chunks_of(W, H, dtype, codec)
    st = open_stream(ffs, W, H, dtype)
    inside = place(st.host_bytes(), chunks[:1], [5])
    for mixed in (inside + [chunks[1]], [chunks[1]] + inside):
        with pytest.raises(ffs.FfsError, match="either all chunks"):
            st.decode_only(mixed, codec=codec)
        with pytest.raises(ffs.FfsError, match="either all chunks"):
            st.submit_encoded(mixed, codec)
    # the stream works afterwards: copied, in place, and through the hot path
    check_decode(st, chunks[:2], codec, frames, "copied, after the refusal")
    check_decode(st, place(st.host_bytes(), chunks[:2], [3, len(chunks[0]) + 20]), codec, frames, "in place, after the refusal")
    check_spots(st, chunks, codec, W, H, dtype)


@pytest.mark.parametrize("W,H,dtype,codec", CASES, ids=IDS)
@pytest.mark.parametrize("path", ["decode_only", "process_encoded"])
def test_a_larger_batch_regrows_the_device_buffers(ffs, W, H, dtype, codec, path):
    """One chunk first: the device side of the staging area is sized for it with a quarter and 4096 bytes to spare (or for the whole
    staging area, if that is larger), the byte-offset summary tables for its tiles with a quarter and 16 to spare.  Then a full batch whose
    chunks carry trailers of 7 W H bytes -- as many as are ever parsed behind a chunk's start -- which fits neither."""
    frames = frames_and_oracle(W, H, dtype)[0]
    chunks = chunks_of(W, H, dtype, codec)
    st = open_stream(ffs, W, H, dtype)

    def run(cs, first, what):
        if path == "decode_only":
            check_decode(st, cs, codec, frames[first:], what)
        else:
            check_spots(st, cs, codec, W, H, dtype, first)

    run(chunks[3:], 3, "one chunk")
    staged1 = (len(chunks[3]) + 15) // 16 * 16
    room = max(staged1 + staged1 // 4 + 4096, st.host_bytes().size) + 64
    trailer = b"\0" * 700 + b"\r\n--CIF-BINARY-FORMAT-SECTION----\r\n;\r\n" + b"\x80" * (7 * W * H)
    big = [c + trailer for c in chunks]
    assert sum((len(c) + 15) // 16 * 16 for c in big) + 64 > room
    if codec == CODEC_BYTE_OFFSET:
        tiles1 = -(-min(len(chunks[3]), 7 * W * H) // 4096)
        assert N * -(-7 * W * H // 4096) > tiles1 + tiles1 // 4 + 16
    run(big, 0, "full batch with trailers")
    run(chunks[3:], 3, "one chunk again")
