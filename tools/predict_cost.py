#!/usr/bin/env python3
"""What scan prediction (ffs_ctx_predict) costs, on an Eiger-16M geometry: 4148 x 4362 pixels of 0.075 mm at 200 mm, 0.98 A, a cell of
78 x 78 x 37 A in an orientation from a fixed seed, dmin 1.5, images of 0.1 degrees, delta_b = 3 x 0.02 and delta_m = 3 x 0.05 degrees;
case "100" has 100 images, case "3600" a full turn.  One process, one JSON line per case, appended to --out (profiles/NAME.jsonl) and
printed.  Per case:

  kernel_ms      the sum of the three launches' times (count pass, scan, write pass) from HIP events on their dispatches, median and
                 extremes of --reps calls after --warmup-calls
  call_ms        the wall time of the whole call (validation, the scan-point settings on the host, their copy, the launches, the records' copy)
  hosttool_s     `ffs_hosttool predict` for the same geometry on one core of the same machine (the same header on the CPU), once; its
                 records must be the library's, byte for byte
  float64 ops    what the launches execute in their walks: a lane that walks (its index is present and inside the resolution sphere)
                 spends 28 float64 operations a scan point -- A_k h is 9 multiplications and 6 additions, its squared norm 5, its side of
                 the sphere 3 additions, 5 and a comparison that is not counted -- and the launches walk three times (the count pass once,
                 the write pass twice: once for a lane's position, once to write).  Crossings add a few hundred operations each and are
                 not counted.  The rate is set beside the machine's vector float64 rate without contraction, 256 CUs x 64 lanes x 2.4 GHz =
                 39.3e12 operations/s, and beside the bytes the launches move.

  python3 tools/predict_cost.py --out profiles/NAME.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-feedback-service_amd", "python"))
import numpy as np  # noqa: E402

W, H = 4148, 4362
PIXEL_MM, DISTANCE_MM, WAVELENGTH, OSC_WIDTH = 0.075, 200.0, 0.98, 0.1
CELL, SEED, DMIN = (78.0, 78.0, 37.0), 2024, 1.5
SIGMA_B, SIGMA_M, N_SIGMA = 0.02, 0.05, 3.0
VECTOR_F64_OPS = 256 * 64 * 2.4e9
HOSTTOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")


def geometry():
    bx, by = W / 2.0, H / 2.0
    return dict(d_matrix=[1.0, 0.0, -bx * PIXEL_MM, 0.0, -1.0, by * PIXEL_MM, 0.0, 0.0, -DISTANCE_MM], pixel_size_mm=[PIXEL_MM, PIXEL_MM], wavelength=WAVELENGTH,
                s0=[0.0, 0.0, -1.0 / WAVELENGTH], rot_axis=[1.0, 0.0, 0.0], osc_start_deg=0.0, osc_width_deg=OSC_WIDTH)


def a_matrix():
    q, r = np.linalg.qr(np.random.default_rng(SEED).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return (q @ np.diag([1.0 / CELL[0], 1.0 / CELL[1], 1.0 / CELL[2]])).reshape(9)


def walkers(A):
    """(candidates, lanes that walk) by the rule's own box and leave test, in NumPy"""
    real = np.linalg.inv(A.reshape(3, 3))
    hm = [int(np.floor(np.linalg.norm(real[i]) / DMIN)) + 1 for i in range(3)]
    h, k, l = np.meshgrid(*[np.arange(-m, m + 1, dtype=np.float64) for m in hm], indexing="ij")
    r = np.stack([h.ravel(), k.ravel(), l.ravel()], 1) @ A.reshape(3, 3).T
    rr = np.sum(r * r, 1)
    return int(rr.size), int(np.count_nonzero(rr <= (1.0 / DMIN ** 2) * 1.000001)) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="the file the lines are appended to (profiles/NAME.jsonl)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--cases", default="100,3600", help="image counts, comma separated")
    ap.add_argument("--label", default="", help="copied into every line (which build of the library this is)")
    args = ap.parse_args()
    import ffs_amd

    g, A = geometry(), a_matrix()
    delta_b, delta_m = N_SIGMA * np.deg2rad(SIGMA_B), N_SIGMA * np.deg2rad(SIGMA_M)
    n_cand, n_walk = walkers(A)
    c = ffs_amd.Context(W, H, np.uint16, max_batch=1)
    for n_images in [int(v) for v in args.cases.split(",")]:
        kernel, wall, rec = [], [], None
        for i in range(args.warmup_calls + args.reps):
            t0 = time.perf_counter()
            rec, ms = c.predict(g, A, n_images, DMIN, delta_b, delta_m, want_ms=True)
            t1 = time.perf_counter()
            if i >= args.warmup_calls:
                kernel.append(ms)
                wall.append((t1 - t0) * 1e3)
        # the wall time above holds two calls of the library (the size, then the records); one call with room for the records:
        single = []
        for i in range(args.reps):
            t0 = time.perf_counter()
            c.predict(g, A, n_images, DMIN, delta_b, delta_m, cap=len(rec))
            single.append((time.perf_counter() - t0) * 1e3)
        host_s, same = None, None
        if os.path.exists(HOSTTOOL):
            with tempfile.TemporaryDirectory() as d:
                np.asarray(A, "<f8").tofile(os.path.join(d, "crystal.bin"))
                t0 = time.perf_counter()
                subprocess.run([HOSTTOOL, "predict", f"distance={DISTANCE_MM!r}", f"beam_x={W / 2.0!r}", f"beam_y={H / 2.0!r}", f"pixel_x={PIXEL_MM!r}", f"pixel_y={PIXEL_MM!r}",
                                f"wavelength={WAVELENGTH!r}", "osc_start=0", f"osc_width={OSC_WIDTH!r}", f"width={W}", f"height={H}", "crystal=crystal.bin",
                                f"n_images={n_images}", f"dmin={DMIN!r}", f"sigma_b={SIGMA_B!r}", f"sigma_m={SIGMA_M!r}", f"n_sigma={N_SIGMA!r}", "out=p.bin"],
                               cwd=d, check=True, capture_output=True)
                host_s = time.perf_counter() - t0
                same = open(os.path.join(d, "p.bin"), "rb").read() == rec.tobytes()
        ops = 3 * n_walk * (n_images + 1) * 28
        med = statistics.median(kernel)
        moved = 3 * (n_images + 1) * 72 + len(rec) * 96 + 3 * ((n_cand + 255) // 256) * 12
        line = dict(mode="predict", label=args.label, geometry="Eiger-16M 4148x4362, 0.075 mm, 200 mm, 0.98 A", cell=CELL, seed=SEED, dmin=DMIN, n_images=n_images,
                    osc_width_deg=OSC_WIDTH, candidates=n_cand, walking_lanes=n_walk, predictions=int(len(rec)),
                    flagged=int(np.count_nonzero(rec["flags"] & ~np.uint32(1))), on_panel=bool(np.all((rec["x_px"] >= 0) & (rec["x_px"] < W) & (rec["y_px"] >= 0) & (rec["y_px"] < H))),
                    reps=args.reps, kernel_ms_median=round(med, 4), kernel_ms_min=round(min(kernel), 4), kernel_ms_max=round(max(kernel), 4),
                    size_query_plus_call_ms_median=round(statistics.median(wall), 4), call_ms_median=round(statistics.median(single), 4),
                    call_ms_min=round(min(single), 4), call_ms_max=round(max(single), 4), hosttool_one_core_s=None if host_s is None else round(host_s, 3),
                    hosttool_same_bytes=same, float64_ops=ops, float64_ops_per_s=round(ops / (med * 1e-3), 0),
                    share_of_vector_float64_rate=round(ops / (med * 1e-3) / VECTOR_F64_OPS, 4), vector_float64_rate_ops_per_s=VECTOR_F64_OPS,
                    bytes_moved_by_the_launches=moved, bound="float64 arithmetic (the launches move kilobytes to megabytes; the walk is registers and scalar loads)",
                    lane_steps_on_candidates_that_never_cross=round(1.0 - len(np.unique(rec[["h", "k", "l"]])) / max(n_walk, 1), 4))
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
