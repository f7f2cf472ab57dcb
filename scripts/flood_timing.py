"""Cost of the flood from seeds on a keyed volume with §13's terrain with caves: host clock around each blocking call, median
of --reps after --warmup, with the spread, beside the rounds run and the bricks visited (a diagnostic counter, blok_hip_debug.h).  One
step per invocation, so that each runs under a time limit of its own:

    air        blok_hip_volume_flood_field over the whole box through the empty cells from the six faces, K = 65534
    bucket     the paint bucket from one surface seed, K = 64 and K = 65534: through the surface material alone, and through everything filled
    region     the air flood over a 64^3 region around the surface at the box's centre
    edits      FILL, FILL_UNREACHED, PAINT and CLEAR over the whole box (each from a fresh field, the volume restored in between)
    baseline   what the flood replaces: blok_hip_volume_download plus the host build's blok_flood_field, on 64^3 and 256^3 volumes of
               their own with the same terrain, beside the device's flood of the same volume, equal byte for byte

    python scripts/flood_timing.py --step air [--size 1024] [--reps 10] [--warmup 2] [--out profiles/flood_timing.txt]

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
from blok_amd import flood as F                # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("air", "bucket", "region", "edits", "baseline")


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def flood_record(t, lo, hi, seeds, K, flags, material, reps, warmup):
    info = t.volume_flood_field(lo, hi, seeds, K, flags, material)
    rounds, visits = t.volume_flood_counters()
    ext = [int(e) for e in info["ext"][0]]
    bricks = int(np.prod([(e + 3) // 4 + 1 for e in ext])) if lo is not None else int(np.prod([(e + 3) // 4 for e in ext]))
    rec = {"K": K, "flags": flags, **{k: int(info[k][0]) for k in ("farthest", "n_seed", "n_reached", "n_unreached")}, "rounds": rounds, "bricks_visited": visits,
           "cover_bricks_at_most": bricks}
    rec["flood"] = times_ms(lambda: t.volume_flood_field(lo, hi, seeds, K, flags, material), reps, warmup)
    rec["us_per_round"] = round(rec["flood"]["ms_median"] * 1e3 / max(rounds, 1), 2)
    return rec


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "flood_timing.txt"))
    args = ap.parse_args()
    n = args.size
    t = HipTracer(64, 64).init()
    rec = {"step": args.step}

    def terrain(size):
        t.volume_create((0, 0, 0), (size, size, size))
        p = T.default_params(size, 0xB10C0001)
        return p, t.volume_generate_terrain(p)

    def surface(p, size):
        c = size // 2
        return c, int(T.height(p, np.array([[c, c]], dtype=np.int32))[0])

    if args.step == "baseline":
        rec["cases"] = []
        for size in (64, 256):
            _, filled = terrain(size)
            held = {}

            def host():
                d, m = t.volume_download()
                held["f"] = F.flood_field_host(d, m, (0, 0, 0), None, None, None, F.MAX_STEPS, F.ALL_FACES)
            case = {"volume": size, "terrain_voxels": filled, "download_and_host_flood": times_ms(host, args.reps, args.warmup)}
            case["device_flood"] = times_ms(lambda: t.volume_flood_field(None, None, None, F.MAX_STEPS, F.ALL_FACES), args.reps, args.warmup)
            case["rounds"], case["bricks_visited"] = t.volume_flood_counters()
            same = t.volume_flood_download().tobytes() == held["f"][0].tobytes() and t.volume_flood_info().tobytes() == held["f"][1].tobytes()
            case["device_equals_host"] = bool(same)
            rec["cases"].append(case)
    else:
        p, filled = terrain(n)
        rec.update(volume=n, terrain_voxels=filled, keyed=t.volume_refresh_counts()[2] == 0)
        c, ground = surface(p, n)
        if args.step == "air":
            rec["floods"] = [flood_record(t, None, None, None, F.MAX_STEPS, F.ALL_FACES, 0, args.reps, args.warmup)]
        elif args.step == "bucket":
            seed = [(c, ground, c)]
            same = F.THROUGH_FILLED | F.SAME_MATERIAL
            rec.update(seed=seed[0], floods=[flood_record(t, None, None, seed, K, flags, p.surface_material, args.reps, args.warmup)
                                             for flags in (same, F.THROUGH_FILLED) for K in (64, F.MAX_STEPS)])
        elif args.step == "region":
            lo = (c - 32, max(0, min(ground - 32, n - 64)), c - 32)
            hi = tuple(v + 64 for v in lo)
            rec.update(region=[lo, hi], floods=[flood_record(t, lo, hi, None, F.MAX_STEPS, F.ALL_FACES, 0, args.reps, args.warmup)])
        else:
            t.volume_encode_bricks()                              # the volume as it is, to put it back between the edits (§18)
            rec["edits"] = {}
            seed = [(c, ground, c)]
            for name, op, flags, seeds in (("fill", F.FILL, F.ALL_FACES, None), ("fill_unreached", F.FILL_UNREACHED, F.ALL_FACES, None),
                                           ("paint", F.PAINT, F.THROUGH_FILLED, seed), ("clear", F.CLEAR, F.THROUGH_FILLED, seed)):
                ms, written = [], 0
                for i in range(args.warmup + args.reps):
                    t.volume_flood_field(None, None, seeds, 64, flags)
                    t0 = time.perf_counter()
                    written = t.volume_edit_by_flood(op, 8, 1.0, 5)
                    if i >= args.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                    t.volume_restore_bricks()
                # an edit reads the snapshot and the densities and writes up to two words per written cell, then refreshes the region
                rec["edits"][name] = {"K": 64, "d": 8, "voxels_written": written, "bytes_read": 6 * n ** 3, "ms_median": round(float(np.median(ms)), 3),
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
