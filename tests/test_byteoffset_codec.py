"""CPU: the Python statement of the CBF byte-offset codec (ffs_amd/byteoffset.py) -- the known answer of the host tool's
self-test, round trips over deltas of every size, and byte-for-byte agreement with the C++ encoder that writes miniCBF files."""
import os
import subprocess

import numpy as np

from ffs_amd import byteoffset, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
MARKER = b"\x0c\x1a\x04\xd5"


def test_known_answer():
    want = bytes.fromhex("01 80 2C 01 80 00 80 90 EE FE FF")
    assert byteoffset.compress(np.array([1, 301, 301 - 70000], np.int32)) == want
    np.testing.assert_array_equal(byteoffset.decompress(want, 3), [1, 301, 301 - 70000])
    np.testing.assert_array_equal(byteoffset.decompress(want, 3, np.uint16), np.array([1, 301, (301 - 70000) & 0xFFFF], np.uint16))


def test_round_trip_all_token_sizes():
    rng = np.random.default_rng(5)
    n = 20000
    small = np.cumsum(rng.integers(-127, 128, n)).astype(np.int32)                       # one byte each
    medium = np.cumsum(rng.integers(-32767, 32768, n)).astype(np.int32)                  # one and three bytes
    wide = rng.integers(-2**31, 2**31, n).astype(np.int32)                               # seven bytes, deltas beyond +-2^31
    edges = np.array([0, 127, 0, -127, 1, 129, 1, -127, 0, 32767, 0, -32767, 0, 32768, 0, -32768, -2**31, 2**31 - 1, -2**31, 0],
                     np.int32)
    mixed = np.concatenate([small[:50], wide[:50], medium[:50], edges, small[50:100]])
    for v in (small, medium, wide, edges, mixed):
        c = byteoffset.compress(v)
        np.testing.assert_array_equal(byteoffset.decompress(c, v.size), v)
    assert len(byteoffset.compress(small)) == n
    d = np.diff(wide.astype(np.int64), prepend=0)
    assert (np.abs(d) > 2**31).any() and len(byteoffset.compress(wide)) == int(np.where(np.abs(d) <= 127, 1, np.where(np.abs(d) <= 32767, 3, 7)).sum())
    # shortest form at the escape values themselves: -128 and -32768 take the next size up
    assert byteoffset.compress(np.array([-128], np.int32)) == bytes.fromhex("80 80 FF")
    assert byteoffset.compress(np.array([-32768], np.int32)) == bytes.fromhex("80 00 80 00 80 FF FF")
    # a token cut by the end of the buffer emits nothing
    c = byteoffset.compress(np.array([5, 1000, 100000], np.int32))
    assert byteoffset.decompress(c[:-1], 3).tolist() == [5, 1000] and byteoffset.decompress(c[:3], 3).tolist() == [5]
    # uint32 pixels are taken by their bit pattern
    u = np.array([0, 4000000000, 5], np.uint32)
    np.testing.assert_array_equal(byteoffset.decompress(byteoffset.compress(u), 3, np.uint32), u)


def test_matches_the_host_tools_encoder(tmp_path):
    """`ffs_hosttool mkcbf` writes byte_offset_compress (host/codecs.hpp) of each frame behind the binary marker."""
    assert subprocess.run([TOOL, "mkcbf", "synth:tiny:2", str(tmp_path / "img_")]).returncode == 0
    p = synth.params(300, 200, np.uint16, seed=7, background=2.0, n_spots=40, sigma=(0.8, 1.6), peak=(30.0, 5000.0), max_value=65535)
    for i, frame in enumerate(synth.frames(p, range(2), threads=2)):
        data = (tmp_path / ("img_%04d.cbf" % (i + 1))).read_bytes()
        section = data[data.index(MARKER) + len(MARKER):]
        assert byteoffset.compress(frame) == section
        np.testing.assert_array_equal(byteoffset.decompress(section, frame.size, np.uint16).reshape(frame.shape), frame)
