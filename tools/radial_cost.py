#!/usr/bin/env python3
"""What the per-frame radial profile (ffs_ctx_set_radial_bins) costs, on bench.py's resident frames: Eiger-16M (16-bit pixels) and
Jungfrau-9M (32-bit pixels), 32 frames a batch, concentric shells about the detector's middle.

  kernel    the profile alone (ffs_bench_radial: k_radial + k_radial_sum, HIP events on the dispatches) with 100 and with 1024 shells,
            beside the memory ceiling of the same run (ffs_bench_hbm's read_gbps) and the threshold stage's dense kernel
            (ffs_bench_threshold's ms_dense).  fraction_of_read_ceiling = the bytes the kernel must read -- pixels, bin entries and mask
            bits of every frame -- per second, over read_gbps; fraction_map_once counts the bin map and the mask once per batch (what
            HBM has to deliver when the caches hold them for the batch's other frames).  The first frames of every row are held to
            tests/radial_oracle.py.
  pipeline  one process: ffs_bench_pipeline at the driver's shape (four streams, 32 frames, --steps after --warmup), with --shells N
            or without a map (--shells 0); prints frames/s.
  ab        `pipeline` in alternating child processes on one box: the --variants (name:shells:tuning, default no map, the profile in the
            sparse stream, the profile in the dense stream), --rounds times in that order and --rounds times in the reverse order; the
            means and each variant's ratio to the first.
  prof      one process, one row (--shells N, --workload, --tune): a few launches of the profile alone -- what a counter pass wraps.

  python3 tools/radial_cost.py kernel --rounds 5 --iters 10 > profiles/...jsonl
  python3 tools/radial_cost.py ab --rounds 3 >> profiles/...jsonl
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


def oracle_match(st, frames, bins, n_bins, mask, n_check):
    import radial_oracle as R
    ok = True
    for f in range(n_check):
        got = st.radial_profile(f)
        want = R.radial_profile(frames[f % len(frames)], bins, n_bins, mask)
        ok = ok and all(np.array_equal(a, b) for a, b in zip(got, want))
    return bool(ok)


def kernel_workload(workload, args):
    import torch
    import ffs_amd
    import radial_oracle as R
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[workload]
    frames, mask = make_inputs(workload, args.frames, 0)
    B = args.batch
    rows = {}
    for shells in args.shells:
        c = ffs_amd.Context(W, H, dt, max_batch=B)
        c.set_mask(mask)
        c.set_tuning(**tuning_of(args.tune))
        bins = R.shell_bins(W, H, shells)
        c.set_radial_bins(bins, shells)
        rows[shells] = (c, c.stream(), bins)
    c0 = next(iter(rows.values()))[0]
    pitch, fstride = c0.device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    ms = {k: [] for k in rows}
    dense = {k: [] for k in rows}
    hbm = {k: [] for k in rows}
    for _ in range(args.rounds):                 # alternating: every row once per round
        for k, (c, st, bins) in rows.items():
            ms[k].append(st.bench_radial(d.data_ptr(), pitch, fstride, B, args.iters))
            dense[k].append(st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)[0])
            hbm[k].append(st.bench_hbm(args.iters)[0])
    npx = float(W) * H
    for k, (c, st, bins) in rows.items():
        st.submit_device(d.data_ptr(), pitch, fstride, B)
        st.wait()
        match = oracle_match(st, frames, bins, k, mask, args.check) if args.check > 0 else None
        path = sorted(st.last_path()[0])
        t, read = statistics.median(ms[k]), statistics.median(hbm[k])
        entry = 1 if tuning_of(args.tune).get("radial_map8") and k <= 255 else 2   # bytes of a bin entry
        per_frame = npx * (np.dtype(dt).itemsize + entry + 0.125)        # pixels + bin entries + mask bits
        must = per_frame * B
        once = npx * np.dtype(dt).itemsize * B + npx * (entry + 0.125)
        print(json.dumps({"mode": "kernel", "workload": workload, "shells": k, "tune": args.tune, "bin_entry_bytes": entry, "batch": B, "unique_frames": len(frames), "label": args.label,
                          "launches_per_round": args.iters, "ms_radial": round(t, 4), "ms_radial_rounds": [round(v, 4) for v in ms[k]],
                          "ms_dense_threshold": round(statistics.median(dense[k]), 4), "read_gbps": round(read, 1),
                          "must_read_gbytes": round(must / 1e9, 4), "gbps_must_read": round(must / t / 1e6, 1),
                          "fraction_of_read_ceiling": round(must / t / 1e6 / read, 3),
                          "fraction_map_once": round(once / t / 1e6 / read, 3), "path": path, "oracle_match": match}), flush=True)
    for c, st, _ in rows.values():
        st.close()
        c.close()


def pipeline_once(args):
    import torch
    import ffs_amd
    import radial_oracle as R
    from ffs_amd import api
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[args.workload]
    frames, mask = make_inputs(args.workload, args.frames, 0)
    B = args.batch
    c = ffs_amd.Context(W, H, dt, max_batch=B)
    c.set_mask(mask)
    shells = args.shells[0]
    c.set_tuning(**tuning_of(args.tune))
    if shells:
        c.set_radial_bins(R.shell_bins(W, H, shells), shells)
    streams = [c.stream() for _ in range(args.streams)]
    pitch, fstride = c.device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    api.bench_pipeline(streams, d.data_ptr(), pitch, fstride, B, args.warmup)
    t0 = time.perf_counter()
    boxes, strong = api.bench_pipeline(streams, d.data_ptr(), pitch, fstride, B, args.steps)
    dt_s = time.perf_counter() - t0
    print(json.dumps({"mode": "pipeline", "workload": args.workload, "shells": shells, "tune": args.tune, "batch": B, "streams": args.streams, "steps": args.steps,
                      "warmup": args.warmup, "label": args.label, "frames_per_s": round(B * args.steps / dt_s, 1), "ms_per_step": round(dt_s / args.steps * 1e3, 4),
                      "boxes": int(boxes), "strong_pixels": int(strong), "path": sorted(streams[0].last_path()[0])}), flush=True)


def prof_once(args):
    import torch
    import ffs_amd
    import radial_oracle as R
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[args.workload]
    frames, mask = make_inputs(args.workload, args.frames, 0)
    c = ffs_amd.Context(W, H, dt, max_batch=args.batch)
    c.set_mask(mask)
    c.set_tuning(**tuning_of(args.tune))
    c.set_radial_bins(R.shell_bins(W, H, args.shells[0]), args.shells[0])
    st = c.stream()
    pitch, fstride = c.device_layout()
    d = resident(torch, frames, args.batch, H, W, dt, pitch)
    ms = st.bench_radial(d.data_ptr(), pitch, fstride, args.batch, args.iters)
    print(json.dumps({"mode": "prof", "workload": args.workload, "shells": args.shells[0], "tune": args.tune, "launches": args.iters, "ms_radial": round(ms, 4)}), flush=True)


def pipeline_ab(args):
    """Child processes: the variants in their order --rounds times, then in the reverse order --rounds times."""
    variants = [v.split(":") for v in args.variants]
    rates = {name: [] for name, _, _ in variants}
    for r in range(2 * args.rounds):
        for name, shells, tune in (variants if r < args.rounds else variants[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "pipeline", "--workload", args.workload, "--shells", shells, "--tune", tune, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--streams", str(args.streams), "--batch", str(args.batch), "--frames", str(args.frames), "--label", name]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=150)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-2000:])
                sys.exit(out.returncode)      # (nothing more is started on the GPU after a child that failed)
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
    ap.add_argument("--shells", type=int, nargs="+", default=None, help="kernel: the rows (default 100 1024); pipeline / ab: one number (0: no map)")
    ap.add_argument("--check", type=int, default=2, help="frames of every row's batch held to tests/radial_oracle.py (0: none)")
    ap.add_argument("--workload", default="eiger16m")
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into every line (which checkout this is, which round)")
    ap.add_argument("--no-j9", action="store_true")
    ap.add_argument("--tune", default="", help="ffs_ctx_set_tuning pairs, 'key=value,key=value' (results are the same)")
    ap.add_argument("--variants", nargs="+", default=["no_map:0:", "sparse_stream:100:radial_stream=0", "dense_stream:100:radial_stream=1"],
                    help="ab: name:shells:tuning of every variant")
    args = ap.parse_args()
    if args.shells is None:
        args.shells = [100, 1024] if args.mode == "kernel" else [100]
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
