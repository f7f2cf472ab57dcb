"""Cost of the column field and of scatter on a keyed volume with §13's terrain with caves: host clock around each blocking
call, median of --reps after --warmup, with the spread.  One step per invocation, so that each runs under a time limit of its own:

    field      blok_hip_volume_column_field over the whole box along each axis, in both directions
    scatter    blok_hip_volume_scatter_models over the whole box's field along +y, cell_log2 2, 4 and 6 with radius 0 and 4
    baseline   what both replace: blok_hip_volume_download plus the host builds blok_column_field and blok_scatter, on a 256^3 volume of
               its own with the same terrain, beside the device's calls on the same volume, equal byte for byte

    python scripts/columns_timing.py --step field [--size 1024] [--reps 10] [--warmup 2] [--out profiles/columns_timing.txt]

Every invocation appends one JSON line to --out.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from blok_amd import columns as K              # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("field", "scatter", "baseline")


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def scatter_params(p, c, radius):
    return K.scatter_params(seed=1, flags=K.ROTATE | K.MIRROR, cell_log2=c, probability=40000, surface_material=p.surface_material, radius=radius, max_rise=1,
                            max_drop=1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "columns_timing.txt"))
    args = ap.parse_args()
    n = 256 if args.step == "baseline" else args.size
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))
    p = T.default_params(n, 0xB10C0001)
    filled = t.volume_generate_terrain(p)
    rec = {"step": args.step, "volume": n, "terrain_voxels": filled, "keyed": t.volume_refresh_counts()[2] == 0, "mask_bytes": 8 * ((n + 3) // 4) ** 3}
    entries = K.scatter_entries([(0, 3, (1, 0, 1), 0), (1, 1, (2, 0, 1), 1)])
    if args.step == "field":
        rec["fields"] = []
        for axis in range(3):
            for flags in (0, K.FROM_LOW):
                info = t.volume_column_field(None, None, axis, flags)
                rec["fields"].append({"axis": axis, "flags": flags, **{k: int(info[k][0]) for k in ("n_columns", "n_hit", "min_top", "max_top")},
                                      "field": times_ms(lambda: t.volume_column_field(None, None, axis, flags), args.reps, args.warmup)})
    elif args.step == "scatter":
        t.volume_column_field()
        rec["scatters"] = []
        for c in (2, 4, 6):
            for radius in (0, 4):
                sp = scatter_params(p, c, radius)
                info = t.volume_scatter_models(sp, entries)
                rec["scatters"].append({"cell_log2": c, "radius": radius, "n_cells": int(info["n_cells"][0]), "n_placed": int(info["n_placed"][0]),
                                        "n_rejected": [int(v) for v in info["n_rejected"][0]],
                                        "scatter": times_ms(lambda: t.volume_scatter_models(sp, entries), args.reps, args.warmup)})
    else:
        sp = scatter_params(p, 4, 4)
        held = {}

        def host():
            d, m = t.volume_download()
            held["field"] = K.column_field_host(d, m, (0, 0, 0), None, None, 1, 0)
            held["table"] = K.scatter_host(*held["field"], sp, entries)
        rec["download_and_host_builds"] = times_ms(host, args.reps, args.warmup)

        def device():
            t.volume_column_field()
            t.volume_scatter_models(sp, entries)
        rec["device_field_and_scatter"] = times_ms(device, args.reps, args.warmup)
        same = (t.volume_columns_download(0).tobytes() == held["field"][0].tobytes() and t.volume_columns_download(1).tobytes() == held["field"][1].tobytes() and
                t.volume_columns_info().tobytes() == held["field"][2].tobytes() and t.volume_scatter_download().tobytes() == held["table"][0].tobytes() and
                t.volume_scatter_info().tobytes() == held["table"][1].tobytes())
        rec["n_placed"] = int(held["table"][1]["n_placed"][0])
        rec["device_equals_host"] = bool(same)
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
