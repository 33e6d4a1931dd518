#!/usr/bin/env python3
"""What measuring Jungfrau pedestals costs (ffs_stream_jungfrau_pedestal_fold), on Jungfrau-9M (3072 x 3072): one JSON
line per measurement, all from this one process (the driver rows start the driver).

  kernel   ms_fold -- HIP events on the fold launch, the upload is not in it -- at 1, 8, 32 and 64 frames, chunks in the stream's host buffer:
           after a warm-up call the median of `--rounds` (20) calls, for frames uniform in stage (the dark run: G0) and for frames mixed in
           stage (every lane sees the three stages).  must_move_bytes = W H (2 frames + 40 per stage present), the stages counted from the
           words that were sent.  fraction_of_read_ceiling / fraction_of_mix_ceiling = those bytes per second over ffs_bench_hbm's read-only
           and 2:1 read / write figures of the same process; bound says which applies (the frames are read only, the accumulators are read
           and written one to one).  After the timed calls the accumulators are held to what the calls must have left (counts and sums are
           multiples of one call's).
  call     frames/s of the synchronous call over PCIe, 32 frames a fold from the streams' host buffers, with 1 and 4 streams on their own
           threads; against the driver's pedestal mode on synth:jungfrau9mdark:N on the GPU and with --cpu-decode, `--alternations` times
           in turn.  The driver rows contain the synthetic generator, the library rows do not.

    python tools/jungfrau_pedestal_cost.py --out profiles/NAME.jsonl [--only kernel,call] [--driver-images 384]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))

import numpy as np  # noqa: E402

try:
    import torch  # noqa: F401,E402  (its HIP runtime has to be in the process first: tests/conftest.py)
except ImportError:
    pass
import ffs_amd  # noqa: E402
from ffs_amd import synth  # noqa: E402

W = H = 3072
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
SEED = 4000


def emit(out, row):
    text = json.dumps(row)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def frames_of(kind, distinct):
    """`distinct` frames: the first frames of a long dark run (all G0), or words whose stage changes from pixel to pixel."""
    if kind == "uniform":
        ped, _ = synth.jungfrau_calibration(W, H, SEED)
        return np.stack([synth.jungfrau_dark(W, H, ped, SEED, i, 3 * distinct) for i in range(distinct)])
    rng = np.random.default_rng(1)
    k = np.arange(W * H, dtype=np.uint32)
    out = []
    for i in range(distinct):
        code = np.array([0, 1, 3, 0, 1, 3, 0, 1], np.uint16)[(k + i) % 8]
        out.append(((code << 14) | rng.integers(1, 0x3FFF, W * H).astype(np.uint16)).reshape(H, W))
    return np.stack(out)


def stages_present(frames):
    valid = ~(((frames >> 14) == 2) | (frames == 0xFFFF) | (frames == 0xC000))
    return len(np.unique(np.minimum(frames[valid] >> 14, 2)))


def place(st, frames, n):
    hb = st.host_bytes()
    size = W * H * 2
    views = []
    for i in range(n):
        hb[i * size:(i + 1) * size] = frames[i % len(frames)].reshape(-1).view(np.uint8)
        views.append(hb[i * size:(i + 1) * size])
    return views


def kernel(args):
    ctx = ffs_amd.Context(W, H, np.uint32, max_batch=64)
    st = ctx.stream()
    st.reserve_host(64 * W * H * 2 + 4096)
    hbm = [st.bench_hbm(5) for _ in range(args.rounds)]
    read_gbps, mix_gbps = (statistics.median(h[k] for h in hbm) for k in (0, 1))
    for kind in ("uniform", "mixed"):
        frames = frames_of(kind, args.distinct)
        present = stages_present(frames)
        valid = [~(((f >> 14) == 2) | (f == 0xFFFF) | (f == 0xC000)) for f in frames]
        words = [int(v.sum()) for v in valid]                                            # per frame: the words that count ...
        adcs = [int((f & 0x3FFF)[v].astype(np.uint64).sum()) for f, v in zip(frames, valid)]   # ... and the sum of their ADCs
        for n in (1, 8, 32, 64):
            views = place(st, frames, n)
            ctx.jungfrau_pedestal_begin()
            st.jungfrau_pedestal_fold(views)
            ms = [st.jungfrau_pedestal_fold(views, want_ms=True) for _ in range(args.rounds)]
            folded, count, total, _ = ctx.jungfrau_pedestal(planes=("count", "sum"))
            calls = args.rounds + 1
            times = [len(range(j, n, len(frames))) for j in range(len(frames))]      # how often frame j is among the n of a call
            checked = bool(folded == calls * n and int(count.sum()) == calls * sum(t * w for t, w in zip(times, words))
                           and int(total.sum()) == calls * sum(t * a for t, a in zip(times, adcs)))
            med = statistics.median(ms)
            frame_bytes, acc_bytes = W * H * 2 * n, W * H * 40 * present
            must = frame_bytes + acc_bytes
            emit(args.out, {"measurement": "kernel", "device": ffs_amd.device_name(0), "frames_are": kind, "stages_present": present, "frames": n, "ms_fold": med,
                            "ms_min": min(ms), "ms_max": max(ms), "rounds": args.rounds, "must_move_bytes": must, "gbps": must / med / 1e6, "read_gbps": read_gbps,
                            "mix_gbps": mix_gbps, "fraction_of_read_ceiling": must / med / 1e6 / read_gbps, "fraction_of_mix_ceiling": must / med / 1e6 / mix_gbps,
                            "bound": "the frames: read only, against the read ceiling" if frame_bytes > acc_bytes else
                                     "the accumulators: one byte written per byte read, against the 2:1 read/write ceiling (the nearest measured)",
                            "accumulators_as_expected": checked})
    ctx.jungfrau_pedestal_end()


def library_leg(n_streams, args, frames):
    batch = 32
    ctx = ffs_amd.Context(W, H, np.uint32, max_batch=batch)
    streams = [ctx.stream() for _ in range(n_streams)]
    for st in streams:
        st.reserve_host(batch * W * H * 2 + 4096)
    views = [place(st, frames, batch) for st in streams]
    ctx.jungfrau_pedestal_begin()
    for st, v in zip(streams, views):
        st.jungfrau_pedestal_fold(v)
    barrier = threading.Barrier(n_streams + 1)

    def work(k):
        barrier.wait()
        for _ in range(args.steps):
            streams[k].jungfrau_pedestal_fold(views[k])
        barrier.wait()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(n_streams)]
    for t in threads:
        t.start()
    barrier.wait()
    t0 = time.perf_counter()
    barrier.wait()
    dt = time.perf_counter() - t0
    for t in threads:
        t.join()
    folded = ctx.jungfrau_pedestal(planes=())[0]
    ctx.jungfrau_pedestal_end()
    n = n_streams * args.steps * batch
    return {"streams": n_streams, "frames_per_fold": batch, "folds": n_streams * args.steps, "seconds": dt, "frames_per_s": n / dt, "pcie_gbps": n * W * H * 2 / dt / 1e9,
            "frames_in_the_accumulators": folded, "as_expected": folded == n + n_streams * batch}


def driver_leg(extra, args, d):
    source = "synth:jungfrau9mdark:%d" % args.driver_images
    p = subprocess.run([os.path.join(BIN, "spotfinder"), source, "--jungfrau-pedestal", os.path.join(d, "ped"), "--threads", str(args.driver_threads), *extra],
                       capture_output=True, text=True, cwd=d, timeout=900)
    m = re.search(r"Jungfrau pedestals: (\d+) frames.*?; ([0-9.]+) frames/s", p.stdout)
    return {"argv": [source, "--jungfrau-pedestal", "PREFIX", "--threads", str(args.driver_threads), *extra], "exit": p.returncode,
            "frames": int(m.group(1)) if m else None, "frames_per_s": float(m.group(2)) if m else None}


def call(args):
    frames = frames_of("uniform", args.distinct)
    with tempfile.TemporaryDirectory() as d:
        for turn in range(args.alternations):
            row = {"measurement": "call", "turn": turn, "device": ffs_amd.device_name(0),
                   "library_1_stream": library_leg(1, args, frames), "library_4_streams": library_leg(4, args, frames),
                   "driver_gpu": driver_leg([], args, d), "driver_cpu_decode": driver_leg(["--cpu-decode"], args, d)}
            emit(args.out, row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", default="kernel,call")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=4, help="different frames among those of a fold")
    ap.add_argument("--steps", type=int, default=10, help="timed folds per stream of a library leg")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--driver-images", type=int, default=384)
    ap.add_argument("--driver-threads", type=int, default=16)
    args = ap.parse_args()
    only = args.only.split(",")
    if "kernel" in only:
        kernel(args)
    if "call" in only:
        call(args)


if __name__ == "__main__":
    main()
