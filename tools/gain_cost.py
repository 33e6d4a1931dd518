#!/usr/bin/env python3
"""What a detector gain (ffs_ctx_set_gain) costs the threshold stage (ffs_bench_threshold, bench.py's resident frames, the 7x7 window).
Standard algorithm: the general-window kernel's GAIN instantiation at gain 2.5 beside the same kernel without a gain (tuning
"window_kernel" = 1: the parent's code) and beside the streaming kernel a batch without a gain takes by default.  Extended algorithm:
the GAIN first pass (k_ext_first) beside the plain first pass without a gain (tuning "ext_first_pass" = 0: the same kernel) and
beside the default (16-bit pixels: the streaming first pass); erosion + final pass are each row's ms_rest_rounds.  Eiger-16M (16-bit
pixels) and Jungfrau-9M (32-bit pixels).  The gain rows run on the frames in ADU (rint(photons x gain), clipped to the pixel type's maximum), the others on the
photon frames, so that the strong sets, and with them the screens' loads, are comparable -- not identical: rounding and clipping
move some decisions (every row reports its own strong_pixels_per_frame).  One context per row, all in one process, the rows measured
in alternating rounds.  One JSON line per row; the gain row's first frames are also held to tests/gain_oracle.py.

The gain-map rows (ffs_ctx_set_gain_map: k_window_gain_map, extended_gain_map) reuse the scalar gain rows' frames in ADU and their
workloads, under a map of eight vertical stripes of gains around 2.5 (2.15 .. 2.85, mean 2.5) that the 32 frames of a batch share:
what the per-pixel load costs is the difference to the scalar row of the same run.  Held to tests/gain_map_oracle.py.

A checkout from before a setter has no rows of its kind: run there (same box, alternating with this one) the other rows are the
parent's figures.

  python3 tools/gain_cost.py --rounds 5 --iters 10 > profiles/...jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

GAIN = 2.5
ROWS = ["k_window_forced_gain0", "k_window_gain", "k_window_gain_map", "k_stream_gain0", "extended_default_gain0", "extended_first0_gain0",
        "extended_gain", "extended_gain_map"]
STRIPES = [2.15, 2.25, 2.35, 2.45, 2.55, 2.65, 2.75, 2.85]


def stripe_map(W, H):
    """Eight vertical stripes of equal width (the last takes the remainder), float32."""
    g = np.empty((H, W), np.float32)
    for i, v in enumerate(STRIPES):
        g[:, i * (W // 8):(W if i == 7 else (i + 1) * (W // 8))] = v
    return g


def oracle_match(W, H, dt, adu_frames, mask, n_check, extended, gain_map=None):
    import ffs_amd
    import gain_oracle as G
    c = ffs_amd.Context(W, H, dt, max_batch=n_check)
    c.set_mask(mask)
    c.set_params(want_strong_list=1, algorithm=ffs_amd.ALGO_DISPERSION_EXTENDED if extended else ffs_amd.ALGO_DISPERSION)
    if gain_map is None:
        c.set_gain(GAIN)
    else:
        import gain_map_oracle as M
        c.set_gain_map(gain_map)
    res = c.stream().process(np.ascontiguousarray(adu_frames[:n_check]))
    ok = True
    for r, img in zip(res, adu_frames[:n_check]):
        if gain_map is not None:
            want = M.dispersion_extended_gain_map(img, mask, gain_map)[0] if extended else M.dispersion_gain_map(img, mask, gain_map)
        else:
            want = G.dispersion_extended_gain(img, mask, GAIN)[0] if extended else G.dispersion_gain(img, mask, GAIN)
        k = np.flatnonzero(want.reshape(-1))
        ok = ok and r.num_strong_pixels == len(k) and np.array_equal(r.strong_k.astype(np.int64), k)
    c.close()
    return bool(ok)


def run_workload(workload, args):
    import torch
    import ffs_amd
    from bench import WORKLOADS, make_inputs
    W, H, dt, bpp = WORKLOADS[workload]
    frames, mask = make_inputs(workload, args.frames, 0)
    adu_frames = np.minimum(np.rint(frames.astype(np.float64) * GAIN), np.iinfo(dt).max).astype(dt)   # (a saturated pixel stays one)
    B = args.batch
    have_gain, have_map = hasattr(ffs_amd.Context, "set_gain"), hasattr(ffs_amd.Context, "set_gain_map")
    gmap = stripe_map(W, H)
    ctxs = {}
    for kind in ROWS:
        if (kind.endswith("_gain") and not have_gain) or (kind.endswith("_gain_map") and not have_map):
            continue
        c = ffs_amd.Context(W, H, dt, max_batch=B)
        c.set_mask(mask)
        if kind == "k_window_forced_gain0":
            c.set_tuning(window_kernel=1)
        if kind == "extended_first0_gain0":
            c.set_tuning(ext_first_pass=0)
        c.set_params(algorithm=ffs_amd.ALGO_DISPERSION_EXTENDED if kind.startswith("extended") else ffs_amd.ALGO_DISPERSION)
        if kind.endswith("_gain"):
            c.set_gain(GAIN)
        if kind.endswith("_gain_map"):
            c.set_gain_map(gmap)
        ctxs[kind] = (c, c.stream())
    c0 = next(iter(ctxs.values()))[0]
    pitch, fstride = c0.device_layout()

    def resident(src):
        host = np.zeros((B, H, pitch // np.dtype(dt).itemsize), dt)
        for i in range(B):
            host[i, :, :W] = src[i % len(src)]
        return torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()

    d_photons, d_adu = resident(frames), resident(adu_frames)

    def in_adu(key):
        return key.endswith("_gain") or key.endswith("_gain_map")

    times = {key: [] for key in ctxs}
    rest = {key: [] for key in ctxs}
    for _ in range(args.rounds):                 # alternating: every row once per round
        for key, (c, st) in ctxs.items():
            d = d_adu if in_adu(key) else d_photons
            a, b = st.bench_threshold(d.data_ptr(), pitch, fstride, B, args.iters)
            times[key].append(a)
            rest[key].append(b)
    alg = float(W) * H * np.dtype(dt).itemsize * B
    for key, (c, st) in ctxs.items():
        ms = statistics.median(times[key])
        match = None
        if in_adu(key) and args.check > 0:
            match = oracle_match(W, H, dt, adu_frames, mask, args.check, key.startswith("extended"), gmap if key.endswith("_gain_map") else None)
        src = adu_frames if in_adu(key) else frames
        strong = float(np.mean([r.num_strong_pixels for r in st.process(np.ascontiguousarray(src[:2]))]))   # (what the row's frames hold)
        print(json.dumps({"workload": workload, "kernel": key, "gain": GAIN if key.endswith("_gain") else "map" if key.endswith("_gain_map") else 0, "batch": B, "unique_frames": len(frames),
                          "strong_pixels_per_frame": strong,
                          "launches_per_round": args.iters, "label": args.label, "ms_per_launch": round(ms, 4),
                          "ms_rounds": [round(t, 4) for t in times[key]], "ms_rest": round(statistics.median(rest[key]), 4),
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
    ap.add_argument("--frames", type=int, default=8, help="unique synthetic frames (bench.py's: seeds from 2000)")
    ap.add_argument("--check", type=int, default=1, help="frames of the gain rows' batch held to tests/gain_oracle.py (0: none)")
    ap.add_argument("--label", default="", help="copied into every line (which checkout this is, which round)")
    ap.add_argument("--no-j9", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (before libffs_hip.so: one HIP runtime in the process)
    run_workload("eiger16m", args)
    if not args.no_j9:
        run_workload("jungfrau9m", args)


if __name__ == "__main__":
    main()
