#!/usr/bin/env python3
"""What the window scope of max_valid costs the threshold stage (ffs_bench_threshold, bench.py's resident frames, the 7x7 window):
the general-window kernel under FFS_MAX_VALID_WINDOW beside the same kernel forced under the centre scope (tuning
"window_kernel" = 1: the code of before the scope existed) and beside the streaming kernel the centre scope takes by default.
Eiger-16M (16-bit pixels: the TRUSTED instantiation) and Jungfrau-9M (32-bit pixels: the neighbour limit as an argument); one
context per row, all in one process, the rows measured in alternating rounds.  One JSON line per row, as tools/window_sizes.py
prints them; the scope row's batch is also held to the oracle on the per-frame mask.  Eiger-16M also has two rows of the extended
algorithm, centre and window scope: its first pass (ms_per_launch) and erosion + final pass (ms_rest_rounds).

A checkout from before the setter has no scope row: run there (same box, alternating with this one) the other two rows are the
parent's figures.

  python3 tools/max_valid_scope_cost.py --rounds 5 --iters 10 > profiles/...jsonl
"""
import argparse
import json
import os
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ROWS = ["k_window_forced_centre", "k_window_scope_window", "k_stream_centre"]
# the extended algorithm (Eiger-16M only): its first pass (ms_per_launch) and erosion + final pass (ms_rest) under either scope
EXT_ROWS = ["extended_centre", "extended_scope_window"]
MAX_VALID = {"eiger16m": 60000, "jungfrau9m": 1_000_000}


def oracle_match(W, H, dt, frames, mask, max_valid, n_check):
    import ffs_amd
    from oracle import oracle as O
    c = ffs_amd.Context(W, H, dt, max_batch=n_check)
    c.set_mask(mask)
    c.set_params(want_strong_list=1, max_valid=max_valid)
    c.set_max_valid_scope("window")
    res = c.stream().process(np.ascontiguousarray(frames[:n_check]))
    with ThreadPoolExecutor(max_workers=min(16, n_check)) as ex:
        want = list(ex.map(lambda img: O.dispersion(img, (mask & (img <= max_valid)).astype(np.uint8)), frames[:n_check]))
    ok = True
    for r, s in zip(res, want):
        k = np.flatnonzero(s.reshape(-1))
        ok = ok and r.num_strong_pixels == len(k) and np.array_equal(r.strong_k.astype(np.int64), k)
    c.close()
    return bool(ok)


def run_workload(workload, args):
    import torch
    import ffs_amd
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[workload]
    frames, mask = make_inputs(workload, args.frames, 0)
    B = args.batch
    max_valid = MAX_VALID[workload]
    have_scope = hasattr(ffs_amd.Context, "set_max_valid_scope")
    ctxs = {}
    for kind in ROWS + (EXT_ROWS if workload == "eiger16m" else []):
        if kind.endswith("scope_window") and not have_scope:
            continue
        c = ffs_amd.Context(W, H, dt, max_batch=B)
        c.set_mask(mask)
        if kind == "k_window_forced_centre":
            c.set_tuning(window_kernel=1)
        c.set_params(max_valid=max_valid, algorithm=ffs_amd.ALGO_DISPERSION_EXTENDED if kind in EXT_ROWS else ffs_amd.ALGO_DISPERSION)
        if kind.endswith("scope_window"):
            c.set_max_valid_scope("window")
        ctxs[kind] = (c, c.stream())
    c0 = next(iter(ctxs.values()))[0]
    pitch, fstride = c0.device_layout()
    host = np.zeros((B, H, pitch // np.dtype(dt).itemsize), dt)
    for i in range(B):
        host[i, :, :W] = frames[i % len(frames)]
    d = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
    del host
    times = {key: [] for key in ctxs}
    rest = {key: [] for key in ctxs}
    for _ in range(args.rounds):                 # alternating: every row once per round
        for key, (c, st) in ctxs.items():
            a, b = st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)
            times[key].append(a)
            rest[key].append(b)
    alg = float(W) * H * np.dtype(dt).itemsize * B
    over = float(np.mean([(f > max_valid).mean() for f in frames]))
    for key, (c, st) in ctxs.items():
        ms = statistics.median(times[key])
        match = None
        if key == "k_window_scope_window" and args.check > 0:
            match = oracle_match(W, H, dt, frames, mask, max_valid, args.check)
        print(json.dumps({"workload": workload, "kernel": key, "max_valid": max_valid, "fraction_above_max_valid": over, "batch": B,
                          "label": args.label, "ms_per_launch": round(ms, 4), "ms_rounds": [round(t, 4) for t in times[key]],
                          "ms_rest_rounds": [round(t, 4) for t in rest[key]],
                          "algorithmic_gbps": round(alg / ms / 1e6, 1), "oracle_match": match}), flush=True)
    for c, st in ctxs.values():
        st.close()
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=32, help="unique synthetic frames (bench.py's: seeds from 2000)")
    ap.add_argument("--check", type=int, default=2, help="frames of the scope row's batch held to the oracle (0: none)")
    ap.add_argument("--label", default="", help="copied into every line (which checkout this is, which round)")
    ap.add_argument("--no-j9", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (before libffs_hip.so: one HIP runtime in the process)
    run_workload("eiger16m", args)
    if not args.no_j9:
        run_workload("jungfrau9m", args)


if __name__ == "__main__":
    main()
