#!/usr/bin/env python3
"""What the per-pixel statistics over a run (ffs_ctx_set_pixel_stats) cost, on bench.py's resident frames: Eiger-16M (16-bit pixels) and
Jungfrau-9M (32-bit pixels), 32 frames a batch.

  kernel    the kernel alone (ffs_bench_pixel_stats: k_pixel_stats, HIP events on the dispatch) beside the memory ceilings of the same run
            (ffs_bench_hbm: read-only and the 2:1 read / write mix) and the threshold stage's dense kernel.  must_move_gbytes = the bytes a
            batch must move: n x W x H x pixel_bytes of frames, read once, plus 48 x W x H of accumulators (24 B a pixel, read and written).
            fraction_of_mix_ceiling = those bytes per second over mix_gbps.  Then one batch through the pipeline, held to
            tests/pixel_stats_oracle.py on --check frames' worth of rows.
  pipeline  one process: ffs_bench_pipeline at the driver's shape (four streams, 32 frames, --steps after --warmup), with --stats 1 or 0;
            prints frames/s.
  ab        `pipeline` in alternating child processes on one box: the --variants (name:stats:tuning; default off, on in the context's own
            stream, on in the dense stream), --rounds times in that order and --rounds times in the reverse order; the means and each
            variant's ratio to the first.
  prof      one process, one workload: a few launches of the kernel alone -- what a counter pass wraps.

  python3 tools/pixel_stats_cost.py kernel --rounds 5 --iters 10 > profiles/...jsonl
  python3 tools/pixel_stats_cost.py ab --rounds 3 >> profiles/...jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def tuning_of(text):
    return {k: int(v) for k, v in (pair.split("=") for pair in text.split(",") if pair)}


def resident(torch, frames, B, H, W, dt, pitch):
    host = np.zeros((B, H, pitch // np.dtype(dt).itemsize), dt)
    for i in range(B):
        host[i, :, :W] = frames[i % len(frames)]
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()


def oracle_match(c, frames, B, rows):
    """One batch's statistics against the oracle, on the first `rows` rows of the detector."""
    import pixel_stats_oracle as P
    batch = np.stack([frames[i % len(frames)][:rows] for i in range(B)])
    want = P.pixel_stats(batch)
    got = c.pixel_stats()
    return bool(got[0] == B and all(np.array_equal(a[:rows], b) for a, b in zip(got[1:], want[1:])))


def kernel_workload(workload, args):
    import torch
    import ffs_amd
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[workload]
    frames, mask = make_inputs(workload, args.frames, 0)
    B = args.batch
    c = ffs_amd.Context(W, H, dt, max_batch=B)
    c.set_mask(mask)
    c.set_tuning(**tuning_of(args.tune))
    st = c.stream()
    pitch, fstride = c.device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    ms, dense, read, mix = [], [], [], []
    for _ in range(args.rounds):
        ms.append(st.bench_pixel_stats(d.data_ptr(), pitch, fstride, B, args.iters))
        dense.append(st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)[0])
        r, m = st.bench_hbm(args.iters)
        read.append(r)
        mix.append(m)
    match = None
    if args.check > 0:
        c.set_pixel_stats("start")
        st.submit_device(d.data_ptr(), pitch, fstride, B)
        st.wait()
        match = oracle_match(c, frames, B, args.check)
    path = sorted(st.last_path()[0])
    npx = float(W) * H
    t = statistics.median(ms)
    must = npx * np.dtype(dt).itemsize * B + 48.0 * npx
    print(json.dumps({"mode": "kernel", "workload": workload, "tune": args.tune, "batch": B, "unique_frames": len(frames), "label": args.label,
                      "launches_per_round": args.iters, "ms_pixel_stats": round(t, 4), "ms_pixel_stats_rounds": [round(v, 4) for v in ms],
                      "ms_dense_threshold": round(statistics.median(dense), 4), "read_gbps": round(statistics.median(read), 1),
                      "mix_gbps": round(statistics.median(mix), 1), "must_move_gbytes": round(must / 1e9, 4), "gbps_must_move": round(must / t / 1e6, 1),
                      "fraction_of_read_ceiling": round(must / t / 1e6 / statistics.median(read), 3),
                      "fraction_of_mix_ceiling": round(must / t / 1e6 / statistics.median(mix), 3), "path": path, "oracle_match": match}), flush=True)
    st.close()
    c.close()


def pipeline_once(args):
    import torch
    import ffs_amd
    from ffs_amd import api
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[args.workload]
    frames, mask = make_inputs(args.workload, args.frames, 0)
    B = args.batch
    c = ffs_amd.Context(W, H, dt, max_batch=B)
    c.set_mask(mask)
    c.set_tuning(**tuning_of(args.tune))
    if args.stats:
        c.set_pixel_stats("start")
    streams = [c.stream() for _ in range(args.streams)]
    pitch, fstride = c.device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    api.bench_pipeline(streams, d.data_ptr(), pitch, fstride, B, args.warmup)
    t0 = time.perf_counter()
    boxes, strong = api.bench_pipeline(streams, d.data_ptr(), pitch, fstride, B, args.steps)
    dt_s = time.perf_counter() - t0
    n_folded = c.pixel_stats(planes=())[0] if args.stats else 0
    print(json.dumps({"mode": "pipeline", "workload": args.workload, "stats": args.stats, "tune": args.tune, "batch": B, "streams": args.streams, "steps": args.steps,
                      "warmup": args.warmup, "label": args.label, "frames_per_s": round(B * args.steps / dt_s, 1), "ms_per_step": round(dt_s / args.steps * 1e3, 4),
                      "boxes": int(boxes), "strong_pixels": int(strong), "frames_folded": n_folded, "path": sorted(streams[0].last_path()[0])}), flush=True)


def prof_once(args):
    import torch
    import ffs_amd
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[args.workload]
    frames, mask = make_inputs(args.workload, args.frames, 0)
    c = ffs_amd.Context(W, H, dt, max_batch=args.batch)
    st = c.stream()
    pitch, fstride = c.device_layout()
    d = resident(torch, frames, args.batch, H, W, dt, pitch)
    ms = st.bench_pixel_stats(d.data_ptr(), pitch, fstride, args.batch, args.iters)
    print(json.dumps({"mode": "prof", "workload": args.workload, "launches": args.iters, "ms_pixel_stats": round(ms, 4)}), flush=True)


def pipeline_ab(args):
    """Child processes: the variants in their order --rounds times, then in the reverse order --rounds times."""
    variants = [v.split(":") for v in args.variants]
    rates = {name: [] for name, _, _ in variants}
    for r in range(2 * args.rounds):
        for name, stats, tune in (variants if r < args.rounds else variants[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "pipeline", "--workload", args.workload, "--stats", stats, "--tune", tune, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--streams", str(args.streams), "--batch", str(args.batch), "--frames", str(args.frames), "--label", name]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=150)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-2000:])
                sys.exit(out.returncode or 1)      # (nothing more is started on the GPU after a child that failed)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            rates[name].append(json.loads(line)["frames_per_s"])
    first = statistics.mean(rates[variants[0][0]])
    print(json.dumps({"mode": "ab", "workload": args.workload, "rounds_per_order": args.rounds, "label": args.label, "variants": args.variants,
                      "frames_per_s": rates, "mean": {k: round(statistics.mean(v), 1) for k, v in rates.items()},
                      "ratio_to_first": {k: round(statistics.mean(v) / first, 4) for k, v in rates.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "pipeline", "ab", "prof"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8, help="unique synthetic frames (bench.py's: seeds from 2000)")
    ap.add_argument("--stats", type=int, default=1, help="pipeline: accumulate (1) or not (0)")
    ap.add_argument("--check", type=int, default=64, help="kernel: rows of the detector on which one batch is held to tests/pixel_stats_oracle.py (0: none)")
    ap.add_argument("--workload", default="eiger16m")
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into every line (which checkout this is, which round)")
    ap.add_argument("--no-j9", action="store_true")
    ap.add_argument("--tune", default="", help="ffs_ctx_set_tuning pairs, 'key=value,key=value' (results are the same)")
    ap.add_argument("--variants", nargs="+", default=["off:0:", "own_stream:1:stats_stream=0", "dense_stream:1:stats_stream=1"],
                    help="ab: name:stats:tuning of every variant")
    args = ap.parse_args()
    if args.mode == "ab":
        pipeline_ab(args)
        return
    import torch  # noqa: F401  (before libffs_hip.so: one HIP runtime in the process)
    if args.mode == "pipeline":
        pipeline_once(args)
        return
    if args.mode == "prof":
        prof_once(args)
        return
    kernel_workload("eiger16m", args)
    if not args.no_j9:
        kernel_workload("jungfrau9m", args)


if __name__ == "__main__":
    main()
