#!/usr/bin/env python3
"""What index assignment for many settings (ffs_ctx_index_assign) costs: 2^17 spots of a lattice (78 x 78 x 37 A on a Pilatus-6M geometry, the
"large" case of tools/index_cost.py at a higher resolution, cut to 131072 spots) under 1000 settings: the triples of the sweep's own basis
vectors as ffs_index_settings gives them, filled up to 1000 with the true cell in random orientations, the true setting last.  One process,
one JSON line, appended to --out (profiles/NAME.jsonl) and printed.  Medians of --reps calls after --warmup-calls, with min and max:

  stages          ffs_ctx_index_assign_launch_ms: HIP events around the three stages in the call's stream, summed over the call's passes:
                  assign (with the key table), duplicates (place, fill, resolve), reduce
  call_ms         the wall time of the whole call (the inverses and the planes on the host, allocation, copies, launches, the host's waits)
  step_ms         the whole step of `spotfinder --index-assign` on the GPU, restated here: every round's pending settings in one call until no
                  absence is detected, then the best setting once more with hkl
  hosttool_s      `ffs_hosttool indexassign` on one core of the same machine for the same centres and settings (the same headers on the CPU),
                  run ONCE: the whole process on the clock, reading its inputs, the same rounds and writing its three files included; its
                  records must be the step's, byte for byte
No counter pass is taken.

  python3 tools/assign_cost.py --out profiles/NAME.jsonl
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import index_cost as IC  # noqa: E402

CELL, SEED, DMIN, MAX_CELL = (78.0, 78.0, 37.0, 90.0, 90.0, 90.0), 2024, 1.5, 94.0
N_SPOTS, N_SETTINGS = 1 << 17, 1000
HOSTTOOL = IC.HOSTTOOL


def the_step(ffs, ctx, rlp, phi, A):
    """host/index_assign.hpp on the GPU: (records after correction, the best setting, its hkl)"""
    A = A.copy()
    recs = np.zeros(len(A), ffs.INDEX_ASSIGNMENT_DT)
    pending, rounds = list(range(len(A))), 0
    while pending:
        got = ctx.index_assign(rlp, phi, A[pending])
        nxt = []
        for p, k in enumerate(pending):
            recs[k] = got[p]
            t = ffs.index_absence_detect(got[p])
            if t >= 0 and rounds < 16:
                A[k] = ffs.index_reindex(A[k], t)
                nxt.append(k)
        pending, rounds = nxt, rounds + 1
    volume = [1.0 / abs(np.linalg.det(a.reshape(3, 3))) if recs[k]["status"] == 0 else 0.0 for k, a in enumerate(A)]
    best = min(range(len(A)), key=lambda k: (-int(recs[k]["n_indexed"]), volume[k], k))
    return recs, best, ctx.index_assign(rlp, phi, A[best], want_hkl=True)[1][0]


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="the file the line is appended to (profiles/NAME.jsonl)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-calls", type=int, default=3)
    ap.add_argument("--label", default="", help="copied into the line (which build of the library this is)")
    args = ap.parse_args()
    import ffs_amd as ffs

    g = IC.geometry()
    axes = IC.real_axes(CELL, SEED)
    xyz = IC.lattice_spots(g, axes, DMIN, SEED)
    assert len(xyz) >= N_SPOTS, len(xyz)
    xyz = np.ascontiguousarray(xyz[np.sort(np.random.default_rng(SEED).permutation(len(xyz))[:N_SPOTS])])
    rlp, _, mm = ffs.index_rlp(g, xyz)
    phi = np.ascontiguousarray(mm[:, 2])
    ctx = ffs.Context(IC.PANEL[0], IC.PANEL[1], np.uint16, max_batch=1)
    vectors = ctx.index_basis(xyz, g, MAX_CELL, n_points=256)
    own = ffs.index_settings(vectors)["A"].reshape(-1, 9)[:N_SETTINGS - 1]
    rng = np.random.default_rng(SEED + 1)
    turned = [np.linalg.inv(axes @ np.linalg.qr(rng.normal(size=(3, 3)))[0]).reshape(9) for _ in range(N_SETTINGS - 1 - len(own))]
    A = np.ascontiguousarray(np.concatenate([own, np.array(turned).reshape(-1, 9), np.linalg.inv(axes).reshape(1, 9)]))
    assert A.shape == (N_SETTINGS, 9)
    stages, recs = [], None

    def call():
        out, ms = ctx.index_assign(rlp, phi, A, want_ms=True)
        stages.append(ms)
        return out

    wall, recs = IC.timed(call, args.warmup_calls, args.reps)
    stages = stages[args.warmup_calls:]
    step_wall, (step_recs, best, hkl) = IC.timed(lambda: the_step(ffs, ctx, rlp, phi, A), 1, 3)
    host_s, same = None, None
    if os.path.exists(HOSTTOOL):
        with tempfile.TemporaryDirectory() as d:
            xyz.astype("<f8").tofile(os.path.join(d, "c.centres"))
            A.astype("<f8").tofile(os.path.join(d, "a.settings"))
            t0 = time.perf_counter()
            subprocess.run(["taskset", "-c", "0", HOSTTOOL, "indexassign", "centres=c.centres", f"distance={IC.DISTANCE_MM!r}", f"beam_x={IC.BEAM[0]!r}", f"beam_y={IC.BEAM[1]!r}",
                            f"pixel_x={IC.PIXEL_MM!r}", f"pixel_y={IC.PIXEL_MM!r}", f"wavelength={IC.WAVELENGTH!r}", "osc_start=0", f"osc_width={IC.OSC_WIDTH!r}", "settings=a.settings",
                            "out=twin"], cwd=d, check=True, capture_output=True)
            host_s = time.perf_counter() - t0
            same = (open(os.path.join(d, "twin.assignments"), "rb").read() == step_recs.tobytes() and open(os.path.join(d, "twin.hkl"), "rb").read() == hkl.tobytes())
    total = [sum(s.values()) for s in stages]
    line = dict(mode="index_assign", label=args.label, geometry="Pilatus-6M 2463x2527, 0.172 mm, 150 mm, 1.0 A, 360 images of 0.25 deg", cell=CELL, spots=int(len(rlp)),
                settings=int(len(A)), settings_from_own_vectors=int(len(own)), reps=args.reps, true_setting_indexed=int(recs[-1]["n_indexed"]),
                true_setting_accepted=int(recs[-1]["n_accepted"]), accepted_all_settings=int(recs["n_accepted"].astype(np.int64).sum()),
                indexed_all_settings=int(recs["n_indexed"].astype(np.int64).sum()), best_setting=int(best),
                stage_ms={k: spread([s[k] for s in stages]) for k in ffs.INDEX_ASSIGN_LAUNCH_SPANS}, launches_ms=spread(total), call_ms=spread(wall),
                step_ms=spread(step_wall), pairs_per_s_launches=round(len(rlp) * len(A) / (statistics.median(total) * 1e-3), 0),
                hosttool_one_core_s=None if host_s is None else round(host_s, 3), hosttool_same_bytes=same, hosttool_runs=1,
                hosttool_time_includes="process start, reading the centres and settings, the rounds of the correction, writing the three files",
                launches_timed="HIP events around the stages in the call's stream, summed over the passes; no counter pass taken")
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
