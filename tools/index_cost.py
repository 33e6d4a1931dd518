#!/usr/bin/env python3
"""What the indexer's basis-vector search (ffs_ctx_index_grid, ffs_ctx_index_peaks) costs at n_points 256, on a Pilatus-6M geometry (2463 x
2527 pixels of 0.172 mm at 150 mm, 1.0 A, images of 0.25 degrees over 90 degrees): case "small", a triclinic cell of 23 x 31 x 37 A to
2.0 A (a few thousand spots), and case "large", 78 x 78 x 37 A to 1.6 A (about 100 000).  One process, one JSON line per case, appended
to --out (profiles/NAME.jsonl) and printed.  Per case, medians of --reps calls after --warmup-calls:

  grid_kernel_ms   the launches of ffs_ctx_index_grid from HIP events around them: zero fill, scatter, the three FFT passes (the last writes
                   the power grid and the line sums), the two small trees
  peaks_kernel_ms  the launches of ffs_ctx_index_peaks: the second statistic, selection (count, scan, write), union, flatten, per-root
                   sums, compaction
  grid_call_ms, peaks_call_ms   the wall time of the whole calls (the map on the host, copies, launches, the host's waits)
  chain_call_ms    Context.index_basis: spots in, candidate vectors out
  hosttool_s       `ffs_hosttool indexbasis` on one core of the same machine for the same centres (the same header on the CPU), run ONCE per
                   case: the whole process on the clock, reading the centres and writing its three files included; its peaks and vectors
                   must be the library's, byte for byte
  stages           ffs_ctx_index_launch_ms: HIP events recorded between the stages in the calls' stream, median per stage over the same
                   calls: fill + scatter, the three FFT passes, the sums' trees; the second statistic, selection, union + flatten,
                   per-root sums + compaction
  bytes            what each stage of the grid must move at 256: the fill writes 16 N^3, the passes along axes 0 and 1 read and write
                   16 N^3 each, the last pass reads 16 N^3 and writes 8 N^3 (104 N^3 = 1.74 GB in all); the second statistic reads 8 N^3,
                   the selection reads 8 N^3 twice.  Each is set over the read/write ceiling ffs_bench_hbm measures in the same process
                   (the second statistic and the selection over its read-only ceiling).  No counter pass is taken.

  python3 tools/index_cost.py --out profiles/NAME.jsonl
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

PANEL = (2463, 2527)
PIXEL_MM, DISTANCE_MM, WAVELENGTH, OSC_WIDTH, N_IMAGES = 0.172, 150.0, 1.0, 0.25, 360
BEAM = (1231.4, 1263.7)
CASES = {"small": dict(cell=(23.0, 31.0, 37.0, 82.0, 97.0, 105.0), seed=5, dmin=2.0, max_cell=45.0),
         "large": dict(cell=(78.0, 78.0, 37.0, 90.0, 90.0, 90.0), seed=2024, dmin=1.6, max_cell=94.0)}
HOSTTOOL = os.path.join(ROOT, "fast-feedback-service_amd", "bin", "ffs_hosttool")
N = 256


def geometry():
    return dict(d_matrix=[1.0, 0.0, -BEAM[0] * PIXEL_MM, 0.0, -1.0, BEAM[1] * PIXEL_MM, 0.0, 0.0, -DISTANCE_MM], pixel_size_mm=[PIXEL_MM, PIXEL_MM], wavelength=WAVELENGTH,
                s0=[0.0, 0.0, -1.0 / WAVELENGTH], rot_axis=[1.0, 0.0, 0.0], osc_start_deg=0.0, osc_width_deg=OSC_WIDTH)


def real_axes(cell, seed):
    a, b, c, al, be, ga = cell
    al, be, ga = np.radians([al, be, ga])
    cx, cy = np.cos(be), (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    rows = np.array([[a, 0, 0], [b * np.cos(ga), b * np.sin(ga), 0], [c * cx, c * cy, c * np.sqrt(1 - cx * cx - cy * cy)]])
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return rows @ q.T


def lattice_spots(g, axes, dmin, seed):
    """(x_px, y_px, z) of the lattice points within 1/dmin that cross the Ewald sphere inside the scan and meet the panel, with centroid noise"""
    A = np.linalg.inv(axes)
    hmax = [int(np.linalg.norm(axes[i]) / dmin) + 1 for i in range(3)]
    h = np.stack(np.meshgrid(*[np.arange(-m, m + 1) for m in hmax], indexing="ij"), -1).reshape(-1, 3)
    r0 = h[np.any(h != 0, axis=1)] @ A.T
    r0 = r0[np.einsum("ij,ij->i", r0, r0) <= 1.0 / dmin ** 2]
    u, s0 = np.array(g["rot_axis"]), np.array(g["s0"])
    ur, su = r0 @ u, s0 @ u
    a, b = r0 @ s0 - su * ur, np.cross(u, r0) @ s0
    c = -0.5 * np.einsum("ij,ij->i", r0, r0) - su * ur
    rad = np.hypot(a, b)
    ok = np.abs(c) <= rad
    Dinv = np.linalg.inv(np.array(g["d_matrix"]).reshape(3, 3))
    out = []
    for sign in (1.0, -1.0):
        z = np.mod(np.degrees(np.arctan2(b[ok], a[ok]) + sign * np.arccos(c[ok] / rad[ok])), 360.0) / OSC_WIDTH
        p = np.radians(z * OSC_WIDTH)
        r = r0[ok]
        v = (r * np.cos(p)[:, None] + np.outer((r @ u) * (1 - np.cos(p)), u) + np.cross(u, r) * np.sin(p)[:, None] + s0) @ Dinv.T
        x, y = v[:, 0] / v[:, 2] / PIXEL_MM, v[:, 1] / v[:, 2] / PIXEL_MM
        out.append(np.stack([x, y, z], 1)[(v[:, 2] > 0) & (z < N_IMAGES) & (x >= 0) & (x < PANEL[0]) & (y >= 0) & (y < PANEL[1])])
    xyz = np.concatenate(out)
    return np.ascontiguousarray(xyz + np.random.default_rng(seed).normal(size=xyz.shape) * [0.3, 0.3, 0.1])


def timed(call, warmup, reps):
    wall, out = [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        out = call()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="the file the lines are appended to (profiles/NAME.jsonl)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--cases", default="small,large")
    ap.add_argument("--label", default="", help="copied into every line (which build of the library this is)")
    args = ap.parse_args()
    import ffs_amd

    g = geometry()
    ctx = ffs_amd.Context(PANEL[0], PANEL[1], np.uint16, max_batch=1)
    hbm_read, hbm_rw = ctx.stream().bench_hbm(5)
    for name in args.cases.split(","):
        case = CASES[name]
        xyz = lattice_spots(g, real_axes(case["cell"], case["seed"]), case["dmin"], case["seed"])
        rlp, _, _ = ffs_amd.index_rlp(g, xyz)
        dmin, b_iso = ffs_amd.index_defaults(rlp, case["max_cell"], N)
        grid_ms, peaks_ms, grid_stages, peaks_stages = [], [], [], []

        def grid():
            used, ms = ctx.index_grid(rlp, dmin, b_iso, N, want_ms=True)
            grid_ms.append(ms)
            grid_stages.append(ctx.index_launch_ms())
            return used

        grid_wall, used = timed(grid, args.warmup_calls, args.reps)
        n_peaks = len(ctx.index_peaks()[0])

        def peaks():
            pk, st, ms = ctx.index_peaks(cap=n_peaks, want_ms=True)
            peaks_ms.append(ms)
            peaks_stages.append(ctx.index_launch_ms())
            return pk, st

        peaks_wall, (pk, st) = timed(peaks, args.warmup_calls, args.reps)
        chain_wall, vectors = timed(lambda: ctx.index_basis(xyz, g, case["max_cell"], n_points=N), 1, max(args.reps // 4, 3))
        host_s, same = None, None
        if os.path.exists(HOSTTOOL):
            with tempfile.TemporaryDirectory() as d:
                xyz.astype("<f8").tofile(os.path.join(d, "c.centres"))
                t0 = time.perf_counter()
                subprocess.run([HOSTTOOL, "indexbasis", "centres=c.centres", f"distance={DISTANCE_MM!r}", f"beam_x={BEAM[0]!r}", f"beam_y={BEAM[1]!r}", f"pixel_x={PIXEL_MM!r}",
                                f"pixel_y={PIXEL_MM!r}", f"wavelength={WAVELENGTH!r}", "osc_start=0", f"osc_width={OSC_WIDTH!r}", f"max-cell={case['max_cell']!r}", f"npoints={N}",
                                "out=twin"], cwd=d, check=True, capture_output=True)
                host_s = time.perf_counter() - t0
                same = (open(os.path.join(d, "twin.peaks"), "rb").read() == pk.tobytes()
                        and open(os.path.join(d, "twin.basis_vectors"), "rb").read() == vectors.tobytes())
        gk, pkm = statistics.median(grid_ms[args.warmup_calls:]), statistics.median(peaks_ms[args.warmup_calls:])
        moved = 104 * N ** 3
        names = ffs_amd.INDEX_LAUNCH_SPANS
        stage_ms = {k: round(statistics.median(d[k] for d in (grid_stages if i < 5 else peaks_stages)[args.warmup_calls:]), 4) for i, k in enumerate(names)}
        stage_bytes = dict(fill_scatter=16 * N ** 3, fft_axis0=32 * N ** 3, fft_axis1=32 * N ** 3, fft_axis2_power=24 * N ** 3, second_statistic=8 * N ** 3, selection=16 * N ** 3)
        stage_gbps = {k: round(b / (stage_ms[k] * 1e-3) / 1e9, 1) for k, b in stage_bytes.items()}
        stage_share = {k: round(v / (hbm_read if k in ("second_statistic", "selection") else hbm_rw), 3) for k, v in stage_gbps.items()}
        line = dict(mode="index", label=args.label, geometry="Pilatus-6M 2463x2527, 0.172 mm, 150 mm, 1.0 A, 360 images of 0.25 deg", case=name, cell=case["cell"],
                    n_points=N, spots=int(len(xyz)), used=int(used.sum()), dmin=round(dmin, 5), b_iso=round(b_iso, 3), n_selected=int(st["n_selected"]), peaks=int(len(pk)),
                    vectors=int(len(vectors)), reps=args.reps, grid_kernel_ms_median=round(gk, 4), grid_kernel_ms_min=round(min(grid_ms[args.warmup_calls:]), 4),
                    grid_kernel_ms_max=round(max(grid_ms[args.warmup_calls:]), 4), peaks_kernel_ms_median=round(pkm, 4), peaks_kernel_ms_min=round(min(peaks_ms[args.warmup_calls:]), 4),
                    peaks_kernel_ms_max=round(max(peaks_ms[args.warmup_calls:]), 4), grid_call_ms_median=round(statistics.median(grid_wall), 4),
                    peaks_call_ms_median=round(statistics.median(peaks_wall), 4), chain_call_ms_median=round(statistics.median(chain_wall), 4),
                    hosttool_one_core_s=None if host_s is None else round(host_s, 3), hosttool_same_bytes=same, grid_bytes_moved=moved,
                    grid_GBps=round(moved / (gk * 1e-3) / 1e9, 1), hbm_read_GBps=round(hbm_read, 1), hbm_read_write_GBps=round(hbm_rw, 1),
                    grid_share_of_read_write_ceiling=round(moved / (gk * 1e-3) / 1e9 / hbm_rw, 3),
                    stage_ms_median=stage_ms, stage_bytes_moved=stage_bytes, stage_GBps=stage_gbps, stage_share_of_ceiling=stage_share,
                    hosttool_runs=1, hosttool_time_includes="process start, reading the centres, writing the three files",
                    launches_timed="HIP events between the stages in the calls' stream; no counter pass taken")
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
