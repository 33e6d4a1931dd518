#!/usr/bin/env python3
"""What raw Jungfrau input costs and saves (FFS_CODEC_JUNGFRAU_RAW), on Jungfrau-9M (3072 x 3072): one JSON line per
measurement, all from this one process (the driver rows start the driver).

  kernel   the conversion launch alone (ffs_decode_only_encoded, HIP events around `--iters` launches, chunks in the stream's host buffer) at
           B = 1, 8 and 32 frames: after a warm-up call the median of `--rounds` (20) calls.  must_move_bytes = W H (24 + 6 B): the six
           calibration planes once per launch, 2 B read and 4 B written per pixel and frame.  fraction_of_mix_ceiling = those bytes per second
           over ffs_bench_hbm's 2:1 read / write figure of the same process (the median of `--rounds` calls); the read-only figure is beside it.
           bound: which term of must_move_bytes is the larger at that B.  The first launch is held to the conversion of the host's rule
           (jungfrau_model.hpp through `ffs_hosttool jfconvert`) on `--check` frames.
  legs     frames/s over PCIe with four streams of 32 frames, `--steps` batches after `--warmup`: raw words converted on the GPU
           (submit_encoded from the streams' host buffers) against the same frames as 32-bit photon counts, converted beforehand, uploaded
           by submit from the same buffers.  The host's conversion time is NOT in the second leg: it is what the driver rows add.
  driver   spotfinder synth:jungfrau9mraw:N --jungfrau-calibration F, with and without --cpu-decode: its own "images in ... fps" line.  The
           synthetic source computes every frame (Poisson background, spots, the encoding) on the reader threads: where that is the slower
           side, both rows show the generator, not PCIe -- and by default at most eight of the threads read when chunks are decoded on the
           GPU (--driver-extra=--all-threads lifts that for both rows).

    python tools/jungfrau_cost.py --out profiles/NAME.jsonl [--only kernel,legs,driver] [--driver-images 256]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
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
from ffs_amd.api import CODEC_JUNGFRAU_RAW  # noqa: E402

W = H = 3072
B = 32
BIN = os.path.join(ROOT, "fast-feedback-service_amd", "bin")
TOP = (1 << 24) - 1


def emit(out, row):
    text = json.dumps(row)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def raw_batch(distinct):
    """B raw frames (`distinct` different ones, repeated) and their calibration."""
    p = synth.jungfrau9m_params()
    ped, fac = synth.jungfrau_calibration(W, H, p.seed)
    raw = synth.raw_frames(p, range(distinct))
    return np.concatenate([raw] * (B // distinct)), ped, fac


def place(st, raw):
    """The frames into the stream's host buffer, 16-aligned; -> the views to submit."""
    hb = st.host_bytes()
    size = W * H * 2
    views = []
    for i, f in enumerate(raw):
        hb[i * size:(i + 1) * size] = f.reshape(-1).view(np.uint8)
        views.append(hb[i * size:(i + 1) * size])
    return views


def host_converted(raw, ped, fac):
    with tempfile.TemporaryDirectory() as d:
        raw.tofile(os.path.join(d, "raw"))
        np.concatenate([ped, fac]).astype("<f4").tofile(os.path.join(d, "cal"))
        subprocess.run([os.path.join(BIN, "ffs_hosttool"), "jfconvert", os.path.join(d, "raw"), os.path.join(d, "cal"), str(W), str(H), os.path.join(d, "out")], check=True)
        return np.fromfile(os.path.join(d, "out"), "<u4").reshape(raw.shape)


def kernel(args, raw, ped, fac):
    ctx = ffs_amd.Context(W, H, np.uint32, max_batch=B)
    ctx.set_jungfrau_calibration(ped, fac)
    st = ctx.stream()
    views = place(st, raw)
    _, got = st.decode_only(views[:args.check], codec=CODEC_JUNGFRAU_RAW)
    checked = bool(np.array_equal(got, host_converted(raw[:args.check], ped, fac)))
    hbm = [st.bench_hbm(args.iters) for _ in range(args.rounds)]
    read_gbps, mix_gbps = (statistics.median(h[k] for h in hbm) for k in (0, 1))
    for n in (1, 8, 32):
        st.decode_only(views[:n], iters=args.iters, want_frames=False, codec=CODEC_JUNGFRAU_RAW)
        ms = [st.decode_only(views[:n], iters=args.iters, want_frames=False, codec=CODEC_JUNGFRAU_RAW)[0] for _ in range(args.rounds)]
        med = statistics.median(ms)
        must = W * H * (24 + 6 * n)
        emit(args.out, {"measurement": "kernel", "device": ffs_amd.device_name(0), "frames": n, "ms": med, "ms_min": min(ms), "ms_max": max(ms), "rounds": args.rounds,
                        "iters": args.iters, "must_move_bytes": must, "gbps": must / med / 1e6, "read_gbps": read_gbps, "mix_gbps": mix_gbps,
                        "fraction_of_mix_ceiling": must / med / 1e6 / mix_gbps, "fraction_of_read_ceiling": must / med / 1e6 / read_gbps,
                        "bound": "calibration planes (24 B a pixel per launch)" if 24 > 6 * n else "frames (2 B read, 4 B written a pixel and frame)",
                        "matches_host_converter": checked, "checked_frames": args.check})


def legs(args, raw, ped, fac):
    ctx = ffs_amd.Context(W, H, np.uint32, max_batch=B)
    ctx.set_params(max_valid=TOP)
    ctx.set_jungfrau_calibration(ped, fac)
    streams = [ctx.stream() for _ in range(4)]
    for st in streams:   # (room for the 32-bit frames of the second leg, before the chunks of the first size the area)
        st.reserve_host(B * (W * H * 4 + 4096))
    _, photons = streams[0].decode_only(list(raw), codec=CODEC_JUNGFRAU_RAW)
    rows = {}
    for leg in ("raw words, converted on the GPU", "32-bit photon counts, uploaded"):
        gpu = leg.startswith("raw")
        inputs = []
        for st in streams:
            if gpu:
                inputs.append(place(st, raw))
            else:
                hb = st.host_buffer()
                hb[:] = photons
                inputs.append(hb)
        submit = (lambda st, x: st.submit_encoded(x, CODEC_JUNGFRAU_RAW)) if gpu else (lambda st, x: st.submit(x))
        counts = None
        for phase, steps in (("warmup", args.warmup), ("timed", args.steps)):
            busy = [False] * 4
            t0 = time.perf_counter()
            for i in range(steps):
                k = i % 4
                if busy[k]:
                    counts = streams[k].wait_counts()
                submit(streams[k], inputs[k])
                busy[k] = True
            for k in range(4):
                if busy[k]:
                    counts = streams[k].wait_counts()
            dt = time.perf_counter() - t0
        rows[leg] = {"frames_per_s": args.steps * B / dt, "seconds": dt, "bytes_per_frame_over_pcie": W * H * (2 if gpu else 4),
                     "pcie_gbps": args.steps * B * W * H * (2 if gpu else 4) / dt / 1e9, "last_batch_counts": counts}
    a, b = rows["raw words, converted on the GPU"], rows["32-bit photon counts, uploaded"]
    emit(args.out, {"measurement": "legs", "device": ffs_amd.device_name(0), "streams": 4, "frames_per_batch": B, "steps": args.steps, "warmup": args.warmup,
                    "legs": rows, "ratio": a["frames_per_s"] / b["frames_per_s"], "same_counts": a["last_batch_counts"] == b["last_batch_counts"]})


def driver(args):
    with tempfile.TemporaryDirectory() as d:
        cal = os.path.join(d, "cal.f32")
        source = "synth:jungfrau9mraw:%d" % args.driver_images
        subprocess.run([os.path.join(BIN, "ffs_hosttool"), "jfcal", source, cal], check=True)
        for extra in ([], ["--cpu-decode"]):
            extra = extra + args.driver_extra.split()
            p = subprocess.run([os.path.join(BIN, "spotfinder"), source, "--jungfrau-calibration", cal, "--threads", str(args.driver_threads), *extra],
                               capture_output=True, text=True, cwd=d, timeout=900)
            txt = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout)
            m = re.search(r"(\d+) images in ([0-9.]+) s \(([0-9.]+) GBps\) \(([0-9.]+) fps\)", txt)
            emit(args.out, {"measurement": "driver", "argv": [source, "--jungfrau-calibration", "FILE", "--threads", str(args.driver_threads), *extra], "exit": p.returncode,
                            "images": int(m.group(1)) if m else None, "seconds": float(m.group(2)) if m else None, "fps": float(m.group(4)) if m else None,
                            "reader_threads": args.driver_threads,
                            "conversion": next((l.replace(cal, "FILE") for l in txt.split("\n") if l.startswith("Jungfrau calibration:")), None),
                            "batches": next((l for l in txt.split("\n") if l.startswith("GPU batches:")), None)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", default="kernel,legs,driver")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--distinct", type=int, default=8, help="different frames in the batch of 32")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--driver-images", type=int, default=256)
    ap.add_argument("--driver-threads", type=int, default=16)
    ap.add_argument("--driver-extra", default="", help="further driver arguments for both rows, e.g. --all-threads (by default at most eight threads read when the GPU decodes)")
    args = ap.parse_args()
    only = args.only.split(",")
    if "kernel" in only or "legs" in only:
        raw, ped, fac = raw_batch(args.distinct)
        if "kernel" in only:
            kernel(args, raw, ped, fac)
        if "legs" in only:
            legs(args, raw, ped, fac)
    if "driver" in only:
        driver(args)


if __name__ == "__main__":
    main()
