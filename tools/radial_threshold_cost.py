#!/usr/bin/env python3
"""What the radial-profile threshold (FFS_ALGO_RADIAL_PROFILE, kernels_radthr.hpp) costs, on bench.py's resident frames: Eiger-16M (16-bit
pixels) and Jungfrau-9M (32-bit pixels), 32 frames a batch, 100 concentric shells about the detector's middle.  One JSON line a row.

  kernel    per workload and per form of the histogram's LDS add (tuning "radthr_form" 1, the plain add, and 2, the run in registers): the histogram launch and the cut + strong
            launches (ffs_bench_threshold's ms_dense and ms_rest: HIP events on the dispatches), medians of --rounds rounds, every row once
            per round; in the same run the radial profile (ffs_bench_radial), the streaming threshold kernel of the dispersion algorithm
            (ffs_bench_threshold's ms_dense on a context of algorithm 0) and the read ceiling (ffs_bench_hbm's read_gbps).
            fraction_of_read_ceiling = the bytes the stage must read -- the frames twice, the two-byte bin entries twice and the mask bits
            twice -- per second of the three launches, over read_gbps.  The first frames of every row are held to
            tests/radial_threshold_oracle.py.
  pipeline  one process: ffs_bench_pipeline at the driver's shape (four streams, 32 frames, --steps after --warmup) on a context of
            algorithm 2 and on one of algorithm 0, alternating, --pipeline-rounds times; frames/s of each and their ratio.

  blur      (--blur, instead of the two above) per workload and blur none | narrow | wide (ffs_ctx_set_radial_blur): the same two halves, the
            stage over the unblurred stage of the same run, the read ceiling of the same run; held to tests/radial_blur_oracle.py.

  python3 tools/radial_threshold_cost.py --out profiles/NAME.jsonl
  python3 tools/radial_threshold_cost.py --blur --out profiles/NAME.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def resident(torch, frames, B, H, W, dt, pitch):
    host = np.zeros((B, H, pitch // np.dtype(dt).itemsize), dt)
    for i in range(B):
        host[i, :, :W] = frames[i % len(frames)]
    return torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()


def emit(out, row):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def oracle_match(st, frames, bins, n_bins, mask, n_check):
    import radial_threshold_oracle as RT
    ok = True
    for f in range(n_check):
        want = RT.shells_hist(frames[f % len(frames)], bins, n_bins, 6.0, mask)
        got = st.radial_thresholds(f)
        ok = ok and all(np.array_equal(got[k], want[k]) for k in ("n_pixels", "n_overflow", "q1", "median", "q3", "cutoff", "status"))
    return bool(ok)


def kernel_workload(workload, args, out):
    import torch
    import ffs_amd
    import radial_oracle as R
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[workload]
    frames, mask = make_inputs(workload, args.frames, 0)
    B, shells = args.batch, args.shells
    bins = R.shell_bins(W, H, shells)
    rows = {}
    for form in (1, 2):
        c = ffs_amd.Context(W, H, dt, max_batch=B)
        c.set_mask(mask)
        c.set_tuning(radthr_form=form)
        c.set_radial_bins(bins, shells)
        c.set_params(algorithm=ffs_amd.ALGO_RADIAL_PROFILE)
        rows[form] = (c, c.stream())
    plain = ffs_amd.Context(W, H, dt, max_batch=B)       # the dispersion algorithm's streaming kernel, the same frames and mask
    plain.set_mask(mask)
    plain_st = plain.stream()
    pitch, fstride = plain.device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    hist = {k: [] for k in rows}
    rest = {k: [] for k in rows}
    profile, stream_kernel, hbm = [], [], []
    for _ in range(args.rounds):                         # alternating: every row once per round
        for form, (c, st) in rows.items():
            a, b = st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)
            hist[form].append(a)
            rest[form].append(b)
        profile.append(rows[1][1].bench_radial(d.data_ptr(), pitch, fstride, B, args.iters))
        stream_kernel.append(plain_st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)[0])
        hbm.append(plain_st.bench_hbm(args.iters)[0])
    read = statistics.median(hbm)
    must = 2.0 * float(W) * H * (np.dtype(dt).itemsize + 2 + 0.125) * B
    for form, (c, st) in rows.items():
        st.submit_device(d.data_ptr(), pitch, fstride, B)
        res = st.wait()
        match = oracle_match(st, frames, bins, shells, mask, args.check) if args.check > 0 else None
        t_hist, t_rest = statistics.median(hist[form]), statistics.median(rest[form])
        emit(out, {"mode": "kernel", "workload": workload, "shells": shells, "radthr_form": form, "batch": B, "unique_frames": len(frames), "label": args.label,
                   "rounds": args.rounds, "launches_per_round": args.iters, "ms_hist": round(t_hist, 4), "ms_cut_strong": round(t_rest, 4),
                   "ms_stage": round(t_hist + t_rest, 4), "ms_hist_rounds": [round(v, 4) for v in hist[form]],
                   "ms_radial_profile": round(statistics.median(profile), 4), "ms_stream_kernel": round(statistics.median(stream_kernel), 4),
                   "read_gbps": round(read, 1), "must_read_gbytes": round(must / 1e9, 4),
                   "fraction_of_read_ceiling": round(must / (t_hist + t_rest) / 1e6 / read, 3),
                   "strong_pixels": int(sum(r.num_strong_pixels for r in res)), "path": sorted(st.last_path()[0]), "oracle_match": match})
    for c, st in list(rows.values()) + [(plain, plain_st)]:
        st.close()
        c.close()


def blur_workload(workload, args, out):
    """--blur: the stage's two halves with blur none, narrow and wide (ffs_ctx_set_radial_blur), one context each on the same resident frames,
    every row once per round, beside the read ceiling of the same run.  The first frames of every row are held to tests/radial_blur_oracle.py."""
    import torch
    import ffs_amd
    import radial_blur_oracle as RB
    import radial_oracle as R
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[workload]
    frames, mask = make_inputs(workload, args.frames, 0)
    B, shells = args.batch, args.shells
    bins = R.shell_bins(W, H, shells)
    rows = {}
    for blur in ("none", "narrow", "wide"):
        c = ffs_amd.Context(W, H, dt, max_batch=B)
        c.set_mask(mask)
        c.set_radial_bins(bins, shells)
        c.set_radial_blur(blur)
        c.set_params(algorithm=ffs_amd.ALGO_RADIAL_PROFILE)
        rows[blur] = (c, c.stream())
    pitch, fstride = rows["none"][0].device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    hist = {k: [] for k in rows}
    rest = {k: [] for k in rows}
    hbm = []
    for _ in range(args.rounds):
        for blur, (c, st) in rows.items():
            a, b = st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)
            hist[blur].append(a)
            rest[blur].append(b)
        hbm.append(rows["none"][1].bench_hbm(args.iters)[0])
    read = statistics.median(hbm)
    must = 2.0 * float(W) * H * (np.dtype(dt).itemsize + 2 + 0.125) * B
    base = statistics.median(hist["none"]) + statistics.median(rest["none"])
    for blur, (c, st) in rows.items():
        st.submit_device(d.data_ptr(), pitch, fstride, B)
        res = st.wait()
        match = None
        if args.check > 0:
            match = True
            for f in range(args.check):
                want = RB.threshold(frames[f % len(frames)], bins, shells, {"none": RB.NONE, "narrow": RB.NARROW, "wide": RB.WIDE}[blur], 6.0, 0.0, mask)
                got = st.radial_thresholds(f)
                match = match and all(np.array_equal(got[k], want[1][k]) for k in ("n_pixels", "n_overflow", "q1", "median", "q3", "cutoff", "status"))
                match = bool(match and res[f].num_strong_pixels == int(want[0].sum()))
        t_hist, t_rest = statistics.median(hist[blur]), statistics.median(rest[blur])
        emit(out, {"mode": "blur", "workload": workload, "shells": shells, "blur": blur, "batch": B, "unique_frames": len(frames), "label": args.label,
                   "rounds": args.rounds, "launches_per_round": args.iters, "ms_hist": round(t_hist, 4), "ms_cut_strong": round(t_rest, 4),
                   "ms_stage": round(t_hist + t_rest, 4), "stage_over_unblurred": round((t_hist + t_rest) / base, 3),
                   "ms_hist_rounds": [round(v, 4) for v in hist[blur]], "ms_cut_strong_rounds": [round(v, 4) for v in rest[blur]],
                   "read_gbps": round(read, 1), "must_read_gbytes": round(must / 1e9, 4),
                   "fraction_of_read_ceiling": round(must / (t_hist + t_rest) / 1e6 / read, 3),
                   "strong_pixels": int(sum(r.num_strong_pixels for r in res)), "path": sorted(st.last_path()[0]), "oracle_match": match})
    for c, st in rows.values():
        st.close()
        c.close()


def pipeline(args, out):
    import torch
    import ffs_amd
    import radial_oracle as R
    from ffs_amd import api
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[args.workload]
    frames, mask = make_inputs(args.workload, args.frames, 0)
    B = args.batch
    sides = {}
    for name, algo in (("dispersion", ffs_amd.ALGO_DISPERSION), ("radial_profile", ffs_amd.ALGO_RADIAL_PROFILE)):
        c = ffs_amd.Context(W, H, dt, max_batch=B)
        c.set_mask(mask)
        if algo == ffs_amd.ALGO_RADIAL_PROFILE:      # (the dispersion side has no map: no profile either, the hot path as bench.py runs it)
            c.set_radial_bins(R.shell_bins(W, H, args.shells), args.shells)
        c.set_params(algorithm=algo)
        sides[name] = (c, [c.stream() for _ in range(args.streams)])
    pitch, fstride = sides["dispersion"][0].device_layout()
    d = resident(torch, frames, B, H, W, dt, pitch)
    rates = {k: [] for k in sides}
    for _ in range(args.pipeline_rounds):
        for name, (c, streams) in sides.items():
            api.bench_pipeline(streams, d.data_ptr(), pitch, fstride, B, args.warmup)
            t0 = time.perf_counter()
            boxes, strong = api.bench_pipeline(streams, d.data_ptr(), pitch, fstride, B, args.steps)
            rates[name].append(round(B * args.steps / (time.perf_counter() - t0), 1))
    emit(out, {"mode": "pipeline", "workload": args.workload, "shells": args.shells, "batch": B, "streams": args.streams, "steps": args.steps, "warmup": args.warmup,
               "label": args.label, "frames_per_s": rates, "mean": {k: round(statistics.mean(v), 1) for k, v in rates.items()},
               "ratio_radial_to_dispersion": round(statistics.mean(rates["radial_profile"]) / statistics.mean(rates["dispersion"]), 4),
               "path": {k: sorted(s[0].last_path()[0]) for k, (c, s) in sides.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="the lines are also appended to this file")
    ap.add_argument("--modes", nargs="+", default=["kernel", "pipeline"], choices=["kernel", "pipeline"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=1, help="launches per round and row")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8, help="unique synthetic frames (bench.py's: seeds from 2000)")
    ap.add_argument("--shells", type=int, default=100)
    ap.add_argument("--check", type=int, default=2, help="frames of every row's batch held to tests/radial_threshold_oracle.py (0: none)")
    ap.add_argument("--workload", default="eiger16m", help="pipeline: the workload")
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pipeline-rounds", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--no-j9", action="store_true")
    ap.add_argument("--blur", action="store_true", help="only this: the stage's two halves with blur none, narrow and wide, both workloads, in one process")
    args = ap.parse_args()
    import torch  # noqa: F401  (before libffs_hip.so: one HIP runtime in the process)
    out = open(args.out, "a") if args.out else None
    if args.blur:
        blur_workload("eiger16m", args, out)
        if not args.no_j9:
            blur_workload("jungfrau9m", args, out)
        return
    if "kernel" in args.modes:
        kernel_workload("eiger16m", args, out)
        if not args.no_j9:
            kernel_workload("jungfrau9m", args, out)
    if "pipeline" in args.modes:
        pipeline(args, out)


if __name__ == "__main__":
    main()
