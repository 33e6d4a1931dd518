#!/usr/bin/env python3
"""What summation integration (ffs_stream_shoebox_fold) costs, on 32 resident Eiger-16M frames of bench.py's sweep workload (the first 32
images of its 100-image sweep, 800 reflections with a rocking curve).  The shoeboxes are the 3D reflections the sweep finds over those
images, their bounding boxes padded by 2 pixels and 1 image, centred on their centres of mass, under the flat geometry the driver builds
for a synthetic source (0.075 mm pixels, 300 mm, 0.976 A, 0.1 degrees an image) with --sigma-b / --sigma-m degrees and 3 sigma.  One
process, one JSON line per measurement, appended to --out (profiles/NAME.jsonl) and printed.

  fold      one batch of 32 frames is submitted and waited for once; then the fold alone, --reps times after --warmup-calls (every fold adds
            the images again: the accumulators' values play no part in the time): the kernel's time from its HIP events and the wall time
            of the whole call (index query, the list's copy, the launch, the event wait), medians and extremes; what the launch walks --
            boxes, corners (each one float64 chain of two sqrt and seven divisions, once per box), pixel visits (pixels x images) -- and the
            first fold's census (foreground and background pixels, flagged boxes).
  pipeline  --streams streams of one context, every one with a batch in flight (submit_device / wait in a Python loop, the oldest batch
            first), --steps steps after --warmup, WITHOUT and WITH the fold after every wait, alternating in this one process --rounds
            times: frames/s and ms per step of either, and the ratio.

  python3 tools/shoebox_cost.py --out profiles/NAME.jsonl
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

W, H, NZ, B = 4148, 4362, 100, 32
PIXEL_MM, DISTANCE_MM, WAVELENGTH, OSC_WIDTH = 0.075, 300.0, 0.976, 0.1


def emit(args, record):
    line = json.dumps(record)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def geometry():
    bx, by = W / 2.0, H / 2.0
    return dict(d_matrix=[1.0, 0.0, -bx * PIXEL_MM, 0.0, -1.0, by * PIXEL_MM, 0.0, 0.0, -DISTANCE_MM], pixel_size_mm=[PIXEL_MM, PIXEL_MM], wavelength=WAVELENGTH,
                s0=[0.0, 0.0, -1.0 / WAVELENGTH], rot_axis=[1.0, 0.0, 0.0], osc_start_deg=0.0, osc_width_deg=OSC_WIDTH)


def shoeboxes(ffs_amd, refl, pad_xy=2, pad_z=1):
    """The sweep's 3D reflections as a shoebox table: s1 through the centre of mass, phi at its image, the box padded."""
    t = np.zeros(len(refl), ffs_amd.SHOEBOX_DT)
    x, y = refl["com_x"].astype(np.float64), refl["com_y"].astype(np.float64)
    lab = np.stack([(x - W / 2.0) * PIXEL_MM, (H / 2.0 - y) * PIXEL_MM, np.full(len(refl), -DISTANCE_MM)], axis=1)
    t["s1"] = lab / np.linalg.norm(lab, axis=1)[:, None] / WAVELENGTH
    t["phi"] = np.deg2rad(refl["com_z"].astype(np.float64) * OSC_WIDTH)
    t["x_min"], t["x_max"] = refl["x_min"].astype(np.int64) - pad_xy, refl["x_max"].astype(np.int64) + 1 + pad_xy
    t["y_min"], t["y_max"] = refl["y_min"].astype(np.int64) - pad_xy, refl["y_max"].astype(np.int64) + 1 + pad_xy
    t["z_min"], t["z_max"] = refl["z_min"].astype(np.int64) - pad_z, refl["z_max"].astype(np.int64) + 1 + pad_z
    off_axis = np.hypot(lab[:, 0], lab[:, 1]) > 1e-9      # (a reflection exactly at the beam centre has no Kabsch frame: the library refuses it)
    return t[off_axis]


def pipeline(streams, d, pitch, fstride, steps, fold):
    inflight = []
    t0 = time.perf_counter()
    for step in range(steps + len(streams)):
        if len(inflight) == len(streams) or step >= steps:
            st = inflight.pop(0)
            st.wait_counts()
            if fold:
                st.shoebox_fold(0)
        else:
            st = streams[step % len(streams)]
        if step < steps:
            st.submit_device(d.data_ptr(), pitch, fstride, B, 0)
            inflight.append(st)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="the file the lines are appended to (profiles/NAME.jsonl)")
    ap.add_argument("--sigma-b", type=float, default=0.01, help="degrees")
    ap.add_argument("--sigma-m", type=float, default=0.04, help="degrees")
    ap.add_argument("--algorithm", default="ellipsoid", choices=["ellipsoid", "dials"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="", help="copied into every line (which build of the library this is)")
    args = ap.parse_args()
    import torch  # (before libffs_hip.so: one HIP runtime in the process)
    import ffs_amd
    from ffs_amd import synth

    p = synth.sweep_params(seed=5000, n_frames=NZ, n_spots=800)
    c = ffs_amd.Context(W, H, np.uint16, max_batch=B)
    c.set_mask(synth.mask_eiger16m())
    c.set_params(want_reflections=0, min_spot_size=3, min_spot_size_3d=15)
    pitch, fstride = c.device_layout()
    host = np.zeros((B, H, pitch // 2), np.uint16)
    host[:, :, :W] = synth.frames(p, range(B), threads=min(16, os.cpu_count() or 1))
    d = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
    del host
    streams = [c.stream() for _ in range(args.streams)]
    st = streams[0]

    # the 3D reflections of the 32 images
    stack = ffs_amd.Stack3D(c)
    st.submit_device(d.data_ptr(), pitch, fstride, B, 0)
    st.wait_counts()
    stack.add_batch(st)
    refl = stack.finish()[0]
    stack.close()
    table = shoeboxes(ffs_amd, refl)
    w, h, depth = (table["x_max"] - table["x_min"]).astype(np.int64), (table["y_max"] - table["y_min"]).astype(np.int64), np.minimum(table["z_max"], B) - np.maximum(table["z_min"], 0)
    delta_b, delta_m = 3.0 * np.deg2rad(args.sigma_b), 3.0 * np.deg2rad(args.sigma_m)
    common = {"workload": "sweep16m, images 0..31", "batch": B, "algorithm": args.algorithm, "sigma_b_deg": args.sigma_b, "sigma_m_deg": args.sigma_m, "n_sigma": 3.0,
              "label": args.label}
    c.shoebox_begin(geometry(), table, args.algorithm, delta_b=delta_b, delta_m=delta_m)

    st.submit_device(d.data_ptr(), pitch, fstride, B, 0)
    st.wait_counts()
    kernel, wall = [], []
    census = None
    for i in range(args.warmup_calls + args.reps):
        t0 = time.perf_counter()
        ms = st.shoebox_fold(0, want_ms=True)
        t1 = time.perf_counter()
        if census is None:
            s = c.shoebox_sums("tukey")
            census = dict(foreground_pixels=int(s["fg_count"].sum()), background_pixels=int(s["n_background"].sum()), boxes_with_foreground=int((s["fg_count"] > 0).sum()),
                          boxes_flagged=int((s["flags"] != 0).sum()), background_failures=int(((s["fg_count"] > 0) & (s["bg_status"] != 0)).sum()))
        if i >= args.warmup_calls:
            kernel.append(ms)
            wall.append((t1 - t0) * 1e3)
    visits = int((w * h * depth).sum())
    emit(args, dict(common, mode="fold", reps=args.reps, reflections_3d=int(len(refl)), shoeboxes=int(len(table)), box_width_median=float(np.median(w)),
                    box_height_median=float(np.median(h)), box_depth_median=float(np.median(depth)), corners=int(((w + 1) * (h + 1)).sum()), pixel_visits=visits,
                    kernel_ms_median=round(statistics.median(kernel), 4), kernel_ms_min=round(min(kernel), 4), kernel_ms_max=round(max(kernel), 4),
                    call_wall_ms_median=round(statistics.median(wall), 4), call_wall_ms_min=round(min(wall), 4), call_wall_ms_max=round(max(wall), 4),
                    pixel_visits_per_us=round(visits / (statistics.median(kernel) * 1e3), 2), **census))

    pipeline(streams, d, pitch, fstride, args.warmup, False)
    pipeline(streams, d, pitch, fstride, args.warmup, True)
    rates = {"without": [], "with": []}
    for r in range(args.rounds):
        for variant, fold in (("without", False), ("with", True)):
            secs = pipeline(streams, d, pitch, fstride, args.steps, fold)
            rates[variant].append(B * args.steps / secs)
            emit(args, dict(common, mode="pipeline", variant=variant, round=r, streams=args.streams, steps=args.steps, warmup=args.warmup,
                            frames_per_s=round(B * args.steps / secs, 1), ms_per_step=round(secs / args.steps * 1e3, 4)))
    mean = {k: statistics.mean(v) for k, v in rates.items()}
    emit(args, dict(common, mode="pipeline_ab", rounds=args.rounds, streams=args.streams, steps=args.steps, frames_per_s_mean={k: round(v, 1) for k, v in mean.items()},
                    ms_per_step_mean={k: round(B / v * 1e3, 4) for k, v in mean.items()}, ratio_with_to_without=round(mean["with"] / mean["without"], 4)))
    c.shoebox_end()
    for s in streams:
        s.close()
    c.close()


if __name__ == "__main__":
    main()
