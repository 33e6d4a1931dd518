#!/usr/bin/env python3
"""The threshold stage alone (ffs_bench_threshold) at every window size, on bench.py's resident frames: the general-window kernel
(kernels_window.hpp) for (k, k), k = 1..7, (1, 7), (7, 1) and forced at 3,3 (tuning "window_kernel" = 1), beside k_stream_u16 at
3,3 -- one context per row, all in one process, the rows measured in alternating rounds; then Jungfrau-9M (32-bit pixels) at 3,3
forced, 5,5 and k_stream_u32 at 3,3.  One JSON line per row: ms per launch (median over the rounds), algorithmic GB/s (pixel
bytes of the batch / time), and whether one batch (its first `--check` frames) matched the oracle at that window.

  python3 tools/window_sizes.py --rounds 5 --iters 10 > profiles/...jsonl
  rocprofv3 --kernel-trace --stats -d out -- python3 tools/window_sizes.py --rounds 2 --iters 5 --check 0
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

# (3,3 without forcing is the streaming kernel: the general kernel runs there only with "window_kernel" = 1)
EIGER_ROWS = [("k_window", k, k) for k in (1, 2, 4, 5, 6, 7)] + [("k_window", 1, 7), ("k_window", 7, 1), ("k_window_forced", 3, 3),
                                                                 ("k_stream", 3, 3)]
J9_ROWS = [("k_window_forced", 3, 3), ("k_window", 5, 5), ("k_stream", 3, 3)]


def oracle_match(ctx_args, frames, mask, kx, ky, n_check):
    """One batch of n_check frames through the hot path at (kx, ky), every strong pixel against the oracle."""
    import ffs_amd
    from oracle import oracle as O
    W, H, dt, tuning = ctx_args
    c = ffs_amd.Context(W, H, dt, max_batch=n_check)
    c.set_mask(mask)
    c.set_tuning(**tuning)
    c.set_params(want_strong_list=1, kernel_half_x=kx, kernel_half_y=ky)
    res = c.stream().process(np.ascontiguousarray(frames[:n_check]))
    prm = O.DispParams(kx, ky, 2, 0.0, 6.0, 3.0)
    with ThreadPoolExecutor(max_workers=min(16, n_check)) as ex:
        want = list(ex.map(lambda img: O.dispersion(img, mask, prm), frames[:n_check]))
    ok = True
    for r, s in zip(res, want):
        k = np.flatnonzero(s.reshape(-1))
        ok = ok and r.num_strong_pixels == len(k) and np.array_equal(r.strong_k.astype(np.int64), k)
    c.close()
    return bool(ok)


def run_workload(workload, rows, args):
    import torch
    import ffs_amd
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[workload]
    frames, mask = make_inputs(workload, args.frames, 0)
    B = args.batch
    ctxs = {}
    for kind, kx, ky in rows:
        c = ffs_amd.Context(W, H, dt, max_batch=B)
        c.set_mask(mask)
        tuning = {"window_kernel": 1} if kind == "k_window_forced" else {}
        c.set_tuning(**tuning)
        c.set_params(kernel_half_x=kx, kernel_half_y=ky)
        ctxs[(kind, kx, ky)] = (c, c.stream(), tuning)
    c0 = next(iter(ctxs.values()))[0]
    pitch, fstride = c0.device_layout()
    host = np.zeros((B, H, pitch // np.dtype(dt).itemsize), dt)
    for i in range(B):
        host[i, :, :W] = frames[i % len(frames)]
    d = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
    del host
    times = {key: [] for key in ctxs}
    for _ in range(args.rounds):                 # alternating: every row once per round
        for key, (c, st, _) in ctxs.items():
            a, _b = st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)
            times[key].append(a)
    alg = float(W) * H * np.dtype(dt).itemsize * B
    for key, (c, st, tuning) in ctxs.items():
        kind, kx, ky = key
        ms = statistics.median(times[key])
        match = oracle_match((W, H, dt, tuning), frames, mask, kx, ky, args.check) if args.check > 0 else None
        print(json.dumps({"workload": workload, "kernel": kind, "kernel_half_x": kx, "kernel_half_y": ky, "batch": B,
                          "ms_per_launch": round(ms, 4), "ms_rounds": [round(t, 4) for t in times[key]],
                          "algorithmic_gbps": round(alg / ms / 1e6, 1), "oracle_match": match}), flush=True)
    for c, st, _ in ctxs.values():
        st.close()
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=32, help="unique synthetic frames (bench.py's: seeds from 2000)")
    ap.add_argument("--check", type=int, default=2, help="frames of the batch held to the oracle per row (0: none)")
    ap.add_argument("--no-j9", action="store_true")
    ap.add_argument("--rows", default="", help="Eiger rows to run, e.g. '5x5,3x3f,3x3s' (f: forced general kernel, s: k_stream); default all")
    args = ap.parse_args()
    import torch  # noqa: F401  (before libffs_hip.so: one HIP runtime in the process)
    rows = EIGER_ROWS
    if args.rows:
        name = {"k_window": "", "k_window_forced": "f", "k_stream": "s"}
        rows = [r for r in EIGER_ROWS if f"{r[1]}x{r[2]}{name[r[0]]}" in args.rows.split(",")]
    run_workload("eiger16m", rows, args)
    if not args.no_j9:
        run_workload("jungfrau9m", J9_ROWS, args)


if __name__ == "__main__":
    main()
