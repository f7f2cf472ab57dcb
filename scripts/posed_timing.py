"""Cost of tracing posed models at 3840 x 2160 over §13's terrain with caves (seed 7, 1024^3): 64 placements of a 128^3 model
captured from the middle of the terrain, in an 8 x 8 grid above it, traced four ways:
    instances       lattice instances through trace_primary_instanced_device: the yardstick, code unchanged
    identity        the same placements as poses (blok_pose_from_instance): the general transform and the second pass on identical pixels
    yaw30           each turned 30 degrees about its centre: what the rotation costs in divergence
    yaw30_scale2    turned and doubled
One step per invocation, so that each runs under a time limit of its own:

    call      host clock around each synchronised call, the four alternated in one loop, median of --reps after --warmup, with the spread
    trace     the same calls, --reps times each in turn, nothing timed: to be run under `rocprofv3 --kernel-trace --stats`
    kernels   reads that run's kernel trace (--trace-csv): the dispatches of the instance and posed kernels in order, --reps per case

    python scripts/posed_timing.py --step call [--size 1024] [--reps 7] [--warmup 2] [--out profiles/posed_timing.txt]

Every invocation but `trace` appends one JSON line to --out.
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

STEPS = ("call", "trace", "kernels")
SEED, EDGE, GRID, PITCH = 7, 128, 8, 160
WIDTH, HEIGHT = 3840, 2160
CASES = ("instances", "identity", "yaw30", "yaw30_scale2")


def kernel_rows(path, name):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if name in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [ms for _, ms in sorted(rows)]


def stats(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4), "reps": len(ms)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-csv", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "posed_timing.txt"))
    args = ap.parse_args()
    n = args.size
    rec = {"step": args.step, "volume": n, "model_edge": EDGE, "placements": GRID * GRID, "frame": [WIDTH, HEIGHT]}
    if args.step == "kernels":
        reps = args.reps
        ibins, ipass = kernel_rows(args.trace_csv, "instance_bins_kernel"), kernel_rows(args.trace_csv, "instance_pass_kernel")
        pbins, ppass = kernel_rows(args.trace_csv, "posed_bins_kernel"), kernel_rows(args.trace_csv, "posed_pass_kernel")
        assert len(ibins) == len(ipass) == reps and len(pbins) == len(ppass) == reps * (len(CASES) - 1), (len(ibins), len(ipass), len(pbins), len(ppass))
        rec["instances"] = {"bins": stats(ibins), "pass": stats(ipass)}
        for k, name in enumerate(CASES[1:]):
            rec[name] = {"bins": stats(pbins[k * reps:(k + 1) * reps]), "pass": stats(ppass[k * reps:(k + 1) * reps])}
        rec["identity_pass_over_instance_pass"] = round(rec["identity"]["pass"]["ms_median"] / rec["instances"]["pass"]["ms_median"], 2)
        rec["yaw30_pass_over_identity_pass"] = round(rec["yaw30"]["pass"]["ms_median"] / rec["identity"]["pass"]["ms_median"], 2)
    else:
        import torch
        from blok_amd import pose as P
        from blok_amd import stamp as ST
        from blok_amd import terrain as T
        from blok_amd import world as W
        from blok_amd._ffi import INSTANCE, POSE, POSE_ID
        from blok_amd.tracer import HipTracer
        t = HipTracer(WIDTH, HEIGHT).init()
        t.volume_create((0, 0, 0), (n, n, n))
        p = T.default_params(n, SEED)
        rec["terrain_voxels"] = t.volume_generate_terrain(p)
        ground = int(T.height(p, [(n // 2, n // 2)])[0])
        lo = (n // 2 - EDGE // 2, max(0, min(n - EDGE, ground - EDGE // 2)), n // 2 - EDGE // 2)
        model = t.volume_capture_model(lo, tuple(c + EDGE for c in lo))
        rec["model_voxels"] = t.last_capture_voxels
        t.volume_rebuild()
        first = n // 2 - GRID * PITCH // 2
        offsets = [(first + PITCH * i, n + 40, first + PITCH * j) for j in range(GRID) for i in range(GRID)]           # above the terrain's box
        table = np.concatenate([ST.placement(o, model=model) for o in offsets]).astype(INSTANCE)
        half = (EDGE / 2.0,) * 3
        poses = {"identity": np.concatenate([P.from_instance(r) for r in table])}
        for name, scale in (("yaw30", 1.0), ("yaw30_scale2", 2.0)):
            poses[name] = np.concatenate([P.rotation(model, yaw=math.radians(30.0), scale=scale, pivot_local=half, position=tuple(c + EDGE / 2.0 for c in o))
                                          for o in offsets]).astype(POSE)
        t.check_instances(table)
        for v in poses.values():
            t.check_poses(v)
        cam = W.camera_look_at((n / 2.0, n + 900.0, -700.0), (n / 2.0, n + 100.0, n / 2.0), 60.0, WIDTH, HEIGHT)
        dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        d_table = dev(table)
        d_poses = {k: dev(v) for k, v in poses.items()}
        hits = torch.zeros(WIDTH * HEIGHT * 16, dtype=torch.uint8, device="cuda")
        rgba = torch.zeros(WIDTH * HEIGHT, dtype=torch.int32, device="cuda")
        ids = torch.zeros(WIDTH * HEIGHT, dtype=torch.int32, device="cuda")

        def call(name):
            if name == "instances":
                t.trace_primary_instanced_device(cam, d_table.data_ptr(), len(table), hits.data_ptr(), rgba.data_ptr(), ids.data_ptr())
            else:
                t.trace_primary_posed_device(cam, 0, 0, d_poses[name].data_ptr(), len(table), hits.data_ptr(), rgba.data_ptr(), ids.data_ptr())
            torch.cuda.synchronize()

        if args.step == "trace":
            for name in CASES:
                for _ in range(args.reps):
                    call(name)
            t.shutdown()
            return 0
        ms = {name: [] for name in CASES}
        for i in range(args.warmup + args.reps):
            for name in CASES:                                   # alternated: drift of the clocks falls on all four alike
                t0 = time.perf_counter()
                call(name)
                if i >= args.warmup:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        for name in CASES:
            rec[name] = stats(ms[name])
            call(name)
            got = ids.cpu().numpy().view(np.uint32)
            rec[name]["pixels_won"] = int(((got != 0xFFFFFFFF) & ((got & POSE_ID) != 0)).sum()) if name != "instances" else int((got != 0xFFFFFFFF).sum())
        assert rec["identity"]["pixels_won"] == rec["instances"]["pixels_won"] > 0
        rec["identity_over_instances"] = round(rec["identity"]["ms_median"] / rec["instances"]["ms_median"], 2)
        rec["yaw30_over_identity"] = round(rec["yaw30"]["ms_median"] / rec["identity"]["ms_median"], 2)
        t.shutdown()
    line = json.dumps(rec)
    print(line, flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
