"""Cost of blok_hip_volume_stamp_affine on a keyed volume with §13's terrain with caves (seed 7): a 128^3 model captured from
the middle of the terrain, written back (SET) where it was taken at
    yaw 0, scale 1      the cells blok_hip_volume_stamp_models writes: the ratio to it is the price of pulling instead of pushing
    yaw 30, scale 1     yaw 30, scale 2     yaw 30, scale 0.5
with blok_hip_volume_stamp_models of the same model at the same place, measured in the same run, as the yardstick.  One step per invocation, so
that each runs under a time limit of its own:

    call      host clock around each blocking call, median of --reps after --warmup, with the spread; the cells written; and a
              device-to-device copy of 256 MiB as the yardstick of the written bytes (8 bytes a cell) per second
    trace     the same calls, --reps times each, nothing timed: to be run under `rocprofv3 --kernel-trace`
    kernels   reads that run's kernel trace (--trace-csv): the dispatches of affine_kernel and stamp_kernel in order, --reps per case, as
              the kernels' own times, with the written bytes per second

    python scripts/affine_timing.py --step call [--size 1024] [--reps 7] [--warmup 2] [--out profiles/affine_timing.txt]

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
SEED, EDGE = 7, 128
CASES = (("yaw0_scale1", 0.0, 1.0), ("yaw30_scale1", 30.0, 1.0), ("yaw30_scale2", 30.0, 2.0), ("yaw30_scale0.5", 30.0, 0.5))


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def kernel_rows(path, name):
    """(duration in ms) of the dispatches whose kernel name contains `name`, in start order."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if name in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [ms for _, ms in sorted(rows)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-csv", default="")
    ap.add_argument("--written", default="", help="kernels: the cells written per case, comma separated, yardstick first (from the call step's line)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "affine_timing.txt"))
    args = ap.parse_args()
    n = args.size
    rec = {"step": args.step, "volume": n, "model_edge": EDGE}
    if args.step == "kernels":
        written = [int(v) for v in args.written.split(",")] if args.written else []
        per_case = args.reps
        stamp = kernel_rows(args.trace_csv, "stamp_kernel")
        pull = kernel_rows(args.trace_csv, "affine_kernel")
        assert len(stamp) == per_case and len(pull) == per_case * len(CASES), (len(stamp), len(pull))
        groups = [("stamp_models", stamp)] + [(name, pull[k * per_case:(k + 1) * per_case]) for k, (name, _, _) in enumerate(CASES)]
        for k, (name, ms) in enumerate(groups):
            rec[name] = {"kernel_ms_median": round(float(np.median(ms)), 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4), "reps": len(ms)}
            if k < len(written):
                rec[name]["written_GB_per_s"] = round(written[k] * 8 / (float(np.median(ms)) * 1e-3) / 1e9, 1)
        rec["yaw0_kernel_over_stamp_kernel"] = round(rec["yaw0_scale1"]["kernel_ms_median"] / rec["stamp_models"]["kernel_ms_median"], 2)
    else:
        from blok_amd import affine as AF
        from blok_amd import stamp as ST
        from blok_amd import terrain as T
        from blok_amd.tracer import HipTracer
        t = HipTracer(64, 64).init()
        t.volume_create((0, 0, 0), (n, n, n))
        p = T.default_params(n, SEED)
        rec["terrain_voxels"] = t.volume_generate_terrain(p)
        rec["keyed"] = t.volume_refresh_counts()[2] == 0
        ground = int(T.height(p, [(n // 2, n // 2)])[0])
        lo = (n // 2 - EDGE // 2, max(0, min(n - EDGE, ground - EDGE // 2)), n // 2 - EDGE // 2)
        hi = tuple(c + EDGE for c in lo)
        model = t.volume_capture_model(lo, hi)
        rec["model_voxels"] = t.last_capture_voxels
        place = ST.placement(lo, model=model)
        centre = tuple(c + EDGE / 2.0 for c in lo)
        records = {"yaw0_scale1": AF.from_instance(place)}
        for name, yaw, scale in CASES[1:]:
            records[name] = AF.rotation(yaw=math.radians(yaw), scale=scale, pivot=(EDGE / 2.0,) * 3, position=centre, model=model)
        calls = [("stamp_models", lambda: t.volume_stamp_models(place, ST.STAMP_SET, 1.0))]
        calls += [(name, (lambda r: lambda: t.volume_stamp_affine(r, None, None, ST.STAMP_SET, 1.0))(records[name])) for name, _, _ in CASES]
        if args.step == "trace":
            for _, fn in calls:
                for _ in range(args.reps):
                    fn()
            t.shutdown()
            return 0
        import torch
        for name, fn in calls:
            rec[name] = times_ms(fn, args.reps, args.warmup)
            rec[name]["written"] = fn()
        assert rec["yaw0_scale1"]["written"] == rec["stamp_models"]["written"] == rec["model_voxels"]
        rec["yaw0_call_over_stamp_models_call"] = round(rec["yaw0_scale1"]["ms_median"] / rec["stamp_models"]["ms_median"], 2)
        src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()
        rec["d2d_copy_256MiB"] = times_ms(copy, args.reps, args.warmup)
        rec["d2d_copy_GB_per_s"] = round((256 << 20) / (rec["d2d_copy_256MiB"]["ms_median"] * 1e-3) / 1e9, 1)
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
