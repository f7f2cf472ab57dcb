"""Cost of the distance field on a keyed volume with §13's terrain with caves: host clock around each blocking call, median
of --reps after --warmup, with the spread, beside the bytes each pass has to move.  One step per invocation, so that each runs under a
time limit of its own:

    field      blok_hip_volume_distance_field over the whole box at R = 1, 4, 8 and 16, to the filled and to the empty cells
    brush      the same over a 64^3 region around a brush at R = 8
    edits      GROW, SHRINK and HOLLOW over the whole box (each from a fresh field at R = 2, the volume restored in between)
    baseline   what the field replaces: blok_hip_volume_download plus the host build's blok_distance_field.  The download entry has no
               region — it fetches the whole box, 8 GiB at 1024^3 — so the 64^3 and the 256^3 case are volumes of their own with the same
               terrain, each fetched whole and given to the host build whole, beside the device's field of the same volume

    python scripts/distance_timing.py --step field [--size 1024] [--reps 10] [--warmup 2] [--out profiles/distance_timing.txt]

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

from blok_amd import _ffi                      # noqa: E402
from blok_amd import distance as D             # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("field", "brush", "edits", "baseline")


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def pass_bytes(lo, hi, box, radius):
    """What the three passes have to move, from shapes alone: the mask words of the bricks the x pass reads (8 bytes each; its halo along x
    not counted), and 2 bytes per cell written and read of the two intermediates and of the snapshot."""
    ext = [h - l for l, h in zip(lo, hi)]
    wy = min(box[1], hi[1] + radius) - max(0, lo[1] - radius)
    wz = min(box[2], hi[2] + radius) - max(0, lo[2] - radius)
    masks = 8 * ((ext[0] + 3) // 4) * ((wy + 3) // 4) * ((wz + 3) // 4)
    gx, gy, out = 2 * ext[0] * wy * wz, 2 * ext[0] * ext[1] * wz, 2 * ext[0] * ext[1] * ext[2]
    return {"x": masks + gx, "y": gx + gy, "z": gy + out, "total": masks + 2 * gx + 2 * gy + out}


def field_record(t, lo, hi, box, radius, to_empty, reps, warmup):
    info = t.volume_distance_field(lo, hi, radius, to_empty)
    rec = {"R": radius, "to_empty": to_empty, **{k: int(info[k][0]) for k in ("n_zero", "n_near", "n_far")}}
    rec["bytes"] = pass_bytes(lo or (0, 0, 0), hi or box, box, radius)
    rec["field"] = times_ms(lambda: t.volume_distance_field(lo, hi, radius, to_empty), reps, warmup)
    # the whole call — three passes, the scratch it allocates each time and its wait — against the bytes the passes move
    rec["TB_per_s"] = round(rec["bytes"]["total"] / (rec["field"]["ms_median"] * 1e-3) / 1e12, 3)
    return rec


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "distance_timing.txt"))
    args = ap.parse_args()
    n = args.size
    t = HipTracer(64, 64).init()
    rec = {"step": args.step}

    def terrain(size):
        t.volume_create((0, 0, 0), (size, size, size))
        p = T.default_params(size, 0xB10C0001)
        return p, t.volume_generate_terrain(p)

    if args.step == "baseline":
        rec["cases"] = []
        for size in (64, 256):
            _, filled = terrain(size)
            held = {}

            def host():
                held["d"] = t.volume_download()[0]
                held["f"] = D.distance_field_host(held["d"], (0, 0, 0), None, None, 8, 0)
            case = {"volume": size, "terrain_voxels": filled, "R": 8, "download_and_host_field": times_ms(host, args.reps, args.warmup)}
            case["device_field"] = times_ms(lambda: t.volume_distance_field(None, None, 8), args.reps, args.warmup)
            same = t.volume_distance_download().tobytes() == held["f"][0].tobytes() and t.volume_distance_info().tobytes() == held["f"][1].tobytes()
            case["device_equals_host"] = bool(same)
            rec["cases"].append(case)
    else:
        p, filled = terrain(n)
        box = (n, n, n)
        rec.update(volume=n, terrain_voxels=filled, keyed=t.volume_refresh_counts()[2] == 0, hbm_rate_of_classify_TB_per_s=5.0)
        if args.step == "field":
            rec["fields"] = [field_record(t, None, None, box, radius, to_empty, args.reps, args.warmup) for radius in (1, 4, 8, 16) for to_empty in (False, True)]
        elif args.step == "brush":
            c = n // 2
            ground = int(T.height(p, np.array([[c, c]], dtype=np.int32))[0])
            lo = (c - 32, max(0, min(ground - 32, n - 64)), c - 32)
            hi = tuple(v + 64 for v in lo)
            rec.update(region=[lo, hi], fields=[field_record(t, lo, hi, box, 8, to_empty, args.reps, args.warmup) for to_empty in (False, True)])
        else:
            t.volume_encode_bricks()                              # the volume as it is, to put it back between the edits (§18)
            rec["edits"] = {}
            for name, op, to_empty in (("grow", _ffi.DISTANCE_GROW, False), ("shrink", _ffi.DISTANCE_SHRINK, True), ("hollow", _ffi.DISTANCE_HOLLOW, True)):
                ms, written = [], 0
                for i in range(args.warmup + args.reps):
                    t.volume_distance_field(None, None, 2, to_empty)
                    t0 = time.perf_counter()
                    written = t.volume_edit_by_distance(op, 3, 1.0, 5)
                    if i >= args.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                    t.volume_restore_bricks()
                # an edit reads the snapshot and the densities and writes two words per written cell, then refreshes the region
                rec["edits"][name] = {"d2": 3, "voxels_written": written, "bytes_read": 6 * n ** 3, "ms_median": round(float(np.median(ms)), 3),
                                      "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": args.reps}
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
