#!/usr/bin/env python3
"""What the per-spot background (ffs_stream_spot_backgrounds) costs, on bench.py's resident frames: Eiger-16M (16-bit pixels) and
Jungfrau-9M (32-bit pixels), 32 frames a batch, border 3 (--border).  One process, one JSON line per measurement, appended to --out
(profiles/NAME.jsonl) and printed.

  call      one batch (want_reflections on) is submitted and waited for once; then the call alone, --reps times after --warmup-calls: the
            kernel's time from its HIP events (kernel_ms) and the wall time of the whole call (boxes to pinned memory, their copy, the launch,
            the event wait, the means), medians and extremes; the number of reflections and the statuses' counts.
  pipeline  --streams streams of one context, every one with a batch in flight (submit_device / wait in a Python loop, the oldest batch
            first), --steps steps after --warmup, WITHOUT and WITH the call after every wait, alternating in this one process --rounds
            times: frames/s and ms per step of either, and the ratio.  Both variants run with want_reflections on, so the difference is the
            call; neither is comparable with bench.py's figure (a native loop, no reflections).

  --model glm: the call is ffs_stream_spot_backgrounds_glm (the robust Poisson GLM of the same ring).  Its `call` line stands beside a
            line of the Tukey call measured in the same process on the same batch, and adds the GLM's status census, how many of the spots
            the Tukey fence leaves without an estimate (status 3) get one, and the median and maximum n_iter.

  python3 tools/spot_background_cost.py --out profiles/NAME.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def resident(torch, frames, B, H, W, dt, pitch):
    host = np.zeros((B, H, pitch // np.dtype(dt).itemsize), dt)
    for i in range(B):
        host[i, :, :W] = frames[i % len(frames)]
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()


def emit(args, record):
    line = json.dumps(record)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def pipeline(streams, d, pitch, fstride, B, steps, border, model="constant"):
    """`steps` batches through the streams, all of them in flight; border > 0: the call after every wait.  -> seconds, spots measured."""
    inflight, spots = [], 0
    t0 = time.perf_counter()
    for step in range(steps + len(streams)):
        if len(inflight) == len(streams) or step >= steps:
            st = inflight.pop(0)
            st.wait_counts()
            if border:
                spots += len(st.spot_backgrounds_glm(border, copy=False) if model == "glm" else st.spot_backgrounds(border, copy=False))
        else:
            st = streams[step % len(streams)]
        if step < steps:
            st.submit_device(d.data_ptr(), pitch, fstride, B, step * B)
            inflight.append(st)
    return time.perf_counter() - t0, spots


def workload(name, args):
    import torch
    import ffs_amd
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[name]
    frames, mask = make_inputs(name, args.frames, 0)
    B = args.batch
    c = ffs_amd.Context(W, H, dt, max_batch=B)
    c.set_mask(mask)
    c.set_params(want_reflections=1)
    streams = [c.stream() for _ in range(args.streams)]
    pitch, fstride = c.device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    common = {"workload": name, "batch": B, "unique_frames": len(frames), "border": args.border, "label": args.label}

    st = streams[0]
    st.submit_device(d.data_ptr(), pitch, fstride, B)
    st.wait_counts()
    tukey = None
    for model in (["constant", "glm"] if args.model == "glm" else ["constant"]):
        call = st.spot_backgrounds_glm if model == "glm" else st.spot_backgrounds
        kernel, wall = [], []
        for i in range(args.warmup_calls + args.reps):
            t0 = time.perf_counter()
            bg, ms = call(args.border, copy=False, want_ms=True)
            t1 = time.perf_counter()
            if i >= args.warmup_calls:
                kernel.append(ms)
                wall.append((t1 - t0) * 1e3)
        status = np.bincount(bg["status"], minlength=8 if model == "glm" else 5)
        extra = {}
        if model == "glm":
            fitted = bg["n_iter"][bg["status"] == 0]
            extra = dict(tukey_status3=int((tukey["status"] == 3).sum()), tukey_status3_with_glm_estimate=int(((tukey["status"] == 3) & (bg["status"] == 0)).sum()),
                         n_iter_median=float(np.median(fitted)) if len(fitted) else 0.0, n_iter_max=int(bg["n_iter"].max()) if len(bg) else 0)
        else:
            tukey = bg.copy()
        emit(args, dict(common, mode="call", model=model, reps=args.reps, reflections=int(len(bg)), status_counts=[int(v) for v in status],
                        ring_pixels_median=float(np.median(bg["n_pixels"])) if len(bg) else 0.0,
                        kernel_ms_median=round(statistics.median(kernel), 4), kernel_ms_min=round(min(kernel), 4), kernel_ms_max=round(max(kernel), 4),
                        call_wall_ms_median=round(statistics.median(wall), 4), call_wall_ms_min=round(min(wall), 4), call_wall_ms_max=round(max(wall), 4), **extra))

    if "pipeline" not in args.modes:
        for s in streams:
            s.close()
        c.close()
        return
    pipeline(streams, d, pitch, fstride, B, args.warmup, 0)
    pipeline(streams, d, pitch, fstride, B, args.warmup, args.border, args.model)
    rates = {"without": [], "with": []}
    for r in range(args.rounds):
        for variant, border in (("without", 0), ("with", args.border)):
            secs, spots = pipeline(streams, d, pitch, fstride, B, args.steps, border, args.model)
            rates[variant].append(B * args.steps / secs)
            emit(args, dict(common, mode="pipeline", model=args.model, variant=variant, round=r, streams=args.streams, steps=args.steps, warmup=args.warmup,
                            frames_per_s=round(B * args.steps / secs, 1), ms_per_step=round(secs / args.steps * 1e3, 4), spots_measured=spots))
    mean = {k: statistics.mean(v) for k, v in rates.items()}
    emit(args, dict(common, mode="pipeline_ab", model=args.model, rounds=args.rounds, streams=args.streams, steps=args.steps,
                    frames_per_s_mean={k: round(v, 1) for k, v in mean.items()},
                    ms_per_step_mean={k: round(B / v * 1e3, 4) for k, v in mean.items()}, ratio_with_to_without=round(mean["with"] / mean["without"], 4)))
    for s in streams:
        s.close()
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="the file the lines are appended to (profiles/NAME.jsonl)")
    ap.add_argument("--border", type=int, default=3)
    ap.add_argument("--model", default="constant", choices=["constant", "glm"], help="glm: ffs_stream_spot_backgrounds_glm, beside the Tukey call in `call`")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8, help="unique synthetic frames (bench.py's: seeds from 2000)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["eiger16m", "jungfrau9m"])
    ap.add_argument("--modes", nargs="+", default=["call", "pipeline"], choices=["call", "pipeline"], help="call: always measured; pipeline: the A/B as well")
    ap.add_argument("--label", default="", help="copied into every line (which build of the library this is)")
    args = ap.parse_args()
    import torch  # noqa: F401  (before libffs_hip.so: one HIP runtime in the process)
    for name in args.workloads:
        workload(name, args)


if __name__ == "__main__":
    main()
