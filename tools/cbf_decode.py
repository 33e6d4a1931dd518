#!/usr/bin/env python3
"""CBF byte-offset decode on the GPU against uploading the same frames raw.

8 synthetic frames of Pilatus-6M shape (2463 x 2527), 16- and 32-bit pixels.  Per pixel type, five rounds that alternate
between the three measurements, each reported as the median of its five values:
  decode_ms_per_frame   the three decode launches alone (ffs_decode_only_encoded, HIP events, `--iters` decodes per round)
  encoded_batch         timings() of a batch submitted as byte-offset chunks ([0]: chunks over PCIe + decode)
  raw_batch             timings() of the same frames submitted raw ([0]: frames over PCIe)
The goal of section 5c: decode_ms_per_frame * 8 below raw_batch h2d.

    python tools/cbf_decode.py [--frames 8] [--rounds 5] [--iters 10] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))

import numpy as np  # noqa: E402

try:
    import torch  # noqa: F401,E402  (its HIP runtime has to be in the process first: tests/conftest.py)
except ImportError:
    pass
import ffs_amd  # noqa: E402
from ffs_amd import byteoffset, synth  # noqa: E402
from ffs_amd.api import CODEC_BYTE_OFFSET  # noqa: E402

W, H = 2463, 2527


def measure(dtype, n_frames, rounds, iters):
    p = synth.params(W, H, dtype, seed=31, background=2.0, n_spots=400, sigma=(0.7, 1.8), peak=(30.0, 3000.0),
                     max_value=65535 if dtype == np.uint16 else (1 << 20))
    frames = synth.frames(p, range(n_frames), threads=8)
    chunks = [byteoffset.compress(f) for f in frames]
    ctx = ffs_amd.Context(W, H, dtype, max_batch=n_frames)
    st = ctx.stream()
    _, got = st.decode_only(chunks, codec=CODEC_BYTE_OFFSET)
    assert np.array_equal(got, frames), "decode is wrong: nothing to measure"
    st.process_encoded(chunks, CODEC_BYTE_OFFSET)   # (warm: staging area, tables, code)
    st.process(frames)
    dec, enc, raw = [], [], []
    for _ in range(rounds):
        ms, _ = st.decode_only(chunks, iters=iters, want_frames=False, codec=CODEC_BYTE_OFFSET)
        dec.append(ms / n_frames)
        st.process_encoded(chunks, CODEC_BYTE_OFFSET)
        enc.append(st.timings())
        st.process(frames)
        raw.append(st.timings())
    med = lambda rows, k: statistics.median(r[k] for r in rows)   # noqa: E731
    out = {
        "dtype": np.dtype(dtype).name, "frames": n_frames, "shape": [H, W],
        "chunk_bytes_mean": int(np.mean([len(c) for c in chunks])), "raw_bytes": int(frames[0].nbytes),
        "decode_ms_per_frame": statistics.median(dec), "decode_ms_per_frame_all": dec,
        "encoded_batch": {k: med(enc, k) for k in enc[0]}, "raw_batch": {k: med(raw, k) for k in raw[0]},
    }
    out["decode_ms_batch"] = out["decode_ms_per_frame"] * n_frames
    out["goal_met"] = out["decode_ms_batch"] < out["raw_batch"]["h2d"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"device": ffs_amd.device_name(0), "results": [measure(dt, a.frames, a.rounds, a.iters) for dt in (np.uint16, np.uint32)]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
