"""GPU: CBF byte-offset chunks decoded on the device (csrc/kernels_byteoffset.hpp: summarise, compose, emit).  The expected pixels
are always the array that was encoded, truncated to the pixel type, or hand-written bytes with hand-written answers -- never
the output of a decoder.  Round trips over shapes and token mixes that put a cut of any segment size at every offset inside a
token; chunk placement and trailing bytes; the hot path from byte-offset input; chunks that end early."""
import numpy as np
import pytest

from ffs_amd import bslz4, byteoffset, synth
from ffs_amd.api import CODEC_BSLZ4, CODEC_BYTE_OFFSET
from util import assert_frame_matches_oracle, make_frame

pytestmark = pytest.mark.gpu

KNOWN = bytes.fromhex("01 80 2C 01 80 00 80 90 EE FE FF")     # 1, 301, 301 - 70000 (the host tool's self-test)
TRAILER_TEXT = b"\r\n--CIF-BINARY-FORMAT-SECTION----\r\n;\r\n"
# deltas whose encodings hold 0x80 at every payload position: 80 80 00 | 80 80 FF | 80 80 80 | 80 00 80 00 80 00 00 |
# 80 00 80 80 80 80 80 | 80 00 80 00 00 00 80 | 7F | 81
LOOKALIKES = np.array([128, -128, -32640, 32768, -2139062144, -2**31, 127, -127], np.int64)


def trailer(n=4096):
    return b"\0" * 700 + TRAILER_TEXT + b"\x80" * (n - 700 - len(TRAILER_TEXT))


def as_int32(values):
    """A chain of values given as (wide) integers, as the int32 the codec accumulates."""
    return (np.asarray(values, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def truncated(v, dtype):
    return (v.astype(np.int64) & (2 ** (8 * np.dtype(dtype).itemsize) - 1)).astype(dtype)


def frame_kinds(W, H, dtype):
    """int32 value chains of W * H elements: a detector image, zeros, the type's whole range, escape look-alikes, and for
    p in 0..6 p one-byte tokens followed by 7-byte tokens only / by 3-byte tokens only."""
    n = W * H
    rng = np.random.default_rng(W * 1000 + H)
    img, _ = make_frame(W=max(W, 16), H=max(H, 16), dtype=dtype, seed=W + H, n_spots=10)
    kinds = [np.ascontiguousarray(img[:H, :W]).reshape(-1).astype(np.int64),
             np.zeros(n, np.int64),
             rng.integers(0, np.iinfo(dtype).max, n, dtype=dtype, endpoint=True).astype(np.int64),
             np.cumsum(LOOKALIKES[np.arange(n) % len(LOOKALIKES)])]
    for p in range(7):
        alt = np.where(np.arange(n) % 2 == 0, 1, -1)
        for big in (100000, 1000):
            d = alt * big
            d[:p] = 1
            kinds.append(np.cumsum(d))
    return [as_int32(k) for k in kinds]


def assert_same(got, want, what=""):
    d = np.argwhere(got != want)
    assert d.size == 0, f"{what}: {len(d)} pixels differ, first at (y,x)={d[:4].tolist()}: got {got[tuple(d[0])]} want {want[tuple(d[0])]}"


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_known_answer(ffs, dtype):
    ctx = ffs.Context(3, 1, dtype, max_batch=1)
    _, got = ctx.stream().decode_only([KNOWN], codec=CODEC_BYTE_OFFSET)
    assert got[0, 0].tolist() == [1, 301, (301 - 70000) & (0xFFFF if dtype == np.uint16 else 0xFFFFFFFF)]


SHAPES = [
    (7, 1, np.uint16),
    (1, 300, np.uint16),       # every element starts a new row
    (67, 45, np.uint32),       # a width unrelated to any segment size
    (487, 195, np.uint16),     # Pilatus 100K
    (487, 195, np.uint32),
    (1043, 981, np.uint32),
]


@pytest.mark.parametrize("W,H,dtype", SHAPES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_round_trip(ffs, W, H, dtype):
    kinds = frame_kinds(W, H, dtype)
    chunks = [byteoffset.compress(v) for v in kinds]
    assert max(map(len, chunks)) >= (6 if W * H > 100 else 2) * min(map(len, chunks))   # one launch, very different lengths
    ctx = ffs.Context(W, H, dtype, max_batch=len(kinds))
    _, got = ctx.stream().decode_only(chunks, codec=CODEC_BYTE_OFFSET)
    for i, (g, v) in enumerate(zip(got, kinds)):
        assert_same(g, truncated(v, dtype).reshape(H, W), f"frame kind {i}")


@pytest.mark.parametrize("W,H,dtype", [(67, 45, np.uint32), (487, 195, np.uint16)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_placement_and_trailing_bytes(ffs, W, H, dtype):
    kinds = frame_kinds(W, H, dtype)[:6]
    want = [truncated(v, dtype).reshape(H, W) for v in kinds]
    chunks = [byteoffset.compress(v) for v in kinds]
    with_trailer = [c + trailer() for c in chunks]
    ctx = ffs.Context(W, H, dtype, max_batch=len(kinds))
    st = ctx.stream()
    st.reserve_host(sum(len(c) + 64 for c in with_trailer) + 4096)
    for name, cs in (("bytes", chunks), ("bytes + trailer", with_trailer)):
        _, got = st.decode_only(cs, codec=CODEC_BYTE_OFFSET)
        for g, w in zip(got, want):
            assert_same(g, w, name)
        # placed by the caller in the stream's staging area, at odd offsets
        hb = st.host_bytes()
        cur, views = 1, []
        for i, c in enumerate(cs):
            hb[cur:cur + len(c)] = np.frombuffer(c, np.uint8)
            views.append(hb[cur:cur + len(c)])
            cur += len(c) + (1, 2, 3, 5, 7, 11)[i % 6]
        _, got = st.decode_only(views, codec=CODEC_BYTE_OFFSET)
        for g, w in zip(got, want):
            assert_same(g, w, name + ", in place")


def tiny_frames(n):
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    return synth.frames(p, range(n), threads=2)


def test_hot_path(ffs):
    frames = tiny_frames(4)
    chunks = [byteoffset.compress(f) + trailer(256) for f in frames]
    ctx = ffs.Context(300, 200, np.uint16, max_batch=4)
    ctx.set_params(want_strong_mask=1, want_strong_list=1)
    st = ctx.stream()
    mask = np.ones((200, 300), np.uint8)
    res = st.process_encoded(chunks, CODEC_BYTE_OFFSET, first_frame_id=11)
    assert [r.frame_id for r in res] == [11, 12, 13, 14]
    for fr, img in zip(res, frames):
        assert_frame_matches_oracle(fr, img, mask)
    # raw, byte-offset, LZ4, byte-offset in turn on one stream
    lz4 = [bslz4.compress(f) for f in frames]
    for batch in (st.process(frames), st.process_encoded(chunks, CODEC_BYTE_OFFSET), st.process_encoded(lz4, CODEC_BSLZ4),
                  st.process_encoded(chunks, CODEC_BYTE_OFFSET)):
        for a, b in zip(res, batch):
            assert a.num_strong_pixels == b.num_strong_pixels and len(a.boxes) == len(b.boxes)
            for f in ("l", "t", "r", "b", "num_pixels"):
                np.testing.assert_array_equal(a.boxes[f], b.boxes[f], err_msg=f)


def test_flagged_pixels_truncate_and_are_masked(ffs):
    """miniCBF marks flagged pixels -1 / -2: 65535 / 65534 as 16-bit pixels, masked out by the reader's mask."""
    W, H = 300, 200
    img, mask = make_frame(W, H, np.uint16, seed=12, n_spots=30, masked=True)
    v = img.astype(np.int32)
    v[mask == 0] = np.where(np.arange((mask == 0).sum()) % 2 == 0, -1, -2)
    want = truncated(v.reshape(-1), np.uint16).reshape(H, W)
    assert set(np.unique(want[mask == 0])) == {65534, 65535}
    ctx = ffs.Context(W, H, np.uint16, max_batch=1)
    ctx.set_mask(mask)
    ctx.set_params(want_strong_mask=1, want_strong_list=1)
    st = ctx.stream()
    _, got = st.decode_only([byteoffset.compress(v)], codec=CODEC_BYTE_OFFSET)
    assert_same(got[0], want)
    assert_frame_matches_oracle(st.process_encoded([byteoffset.compress(v)], CODEC_BYTE_OFFSET)[0], want, mask)


def test_bad_chunks_are_refused(ffs):
    W, H = 200, 100
    n = W * H
    img, _ = make_frame(W=W, H=H, seed=3, n_spots=10)
    ctx = ffs.Context(W, H, np.uint16, max_batch=2)
    st = ctx.stream()
    good = byteoffset.compress(img)

    def still_works():
        _, got = st.decode_only([good], codec=CODEC_BYTE_OFFSET)
        assert_same(got[0], img, "after an error")
        assert st.process_encoded([good], CODEC_BYTE_OFFSET)[0].num_strong_pixels == st.process(img)[0].num_strong_pixels

    # one byte short of the shortest possible frame
    short = bytes(n - 1)
    with pytest.raises(ffs.FfsError, match="byte-offset"):
        st.submit_encoded([short], CODEC_BYTE_OFFSET)
    with pytest.raises(ffs.FfsError, match="byte-offset"):
        st.decode_only([short], codec=CODEC_BYTE_OFFSET)
    still_works()
    # long enough in bytes, but 3-byte tokens only: it ends after a third of the frame
    m = (n + 2) // 3
    early = byteoffset.compress(np.cumsum(np.where(np.arange(m) % 2 == 0, 1000, -1000)).astype(np.int32))
    assert len(early) == 3 * m >= n
    # the last token the frame needs is cut inside its payload
    v = img.astype(np.int32).reshape(-1).copy()
    v[-1] = v[-2] + 100000
    cut = byteoffset.compress(v)[:-2]
    assert len(cut) >= n
    for bad in (early, cut):
        with pytest.raises(ffs.FfsError, match="byte-offset"):
            st.decode_only([bad], codec=CODEC_BYTE_OFFSET)
        still_works()
        with pytest.raises(ffs.FfsError, match="byte-offset"):
            st.process_encoded([good, bad], CODEC_BYTE_OFFSET)
        still_works()
    for call in (lambda: st.submit_encoded([good], 7), lambda: st.decode_only([good], codec=7)):
        with pytest.raises(ffs.FfsError, match="codec"):
            call()
    still_works()
