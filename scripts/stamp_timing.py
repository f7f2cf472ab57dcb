"""Cost of blok_hip_volume_stamp_models and blok_hip_volume_capture_model: host clock around each blocking call, median of
--reps after --warmup, against the routes they replace, which use only entries that existed before them (the host maps the voxel list
and calls volume_set_voxels; volume_download + numpy selection + model_create).  One JSON line per case.

    python scripts/stamp_timing.py [--size 1024] [--reps 20] [--warmup 3] [--baseline-reps 5] [--only stamp|capture]
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
from blok_amd import stamp as ST               # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def world_voxels(xyz, offset, axis, flip):
    """The placement's mapping (blok_hip.h), vectorised: what a caller without the stamp entry has to do on the host."""
    w = np.empty_like(xyz)
    for k in range(3):
        a = axis[k]
        w[:, a] = (offset[a] - 1 - xyz[:, k]) if (flip >> k) & 1 else (offset[a] + xyz[:, k])
    return w


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-reps", type=int, default=5)
    ap.add_argument("--only", choices=["stamp", "capture"], default=None)
    ap.add_argument("--no-baseline", action="store_true", help="the new entries alone (a profiler pass)")
    args = ap.parse_args()
    n = args.size
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))
    p = T.default_params(n, 0xB10C0001)
    filled = t.volume_generate_terrain(p)
    print(json.dumps({"case": "setup", "volume": n, "terrain_voxels": filled, "keyed": t.volume_refresh_counts()[2] == 0}), flush=True)
    c = n // 2

    if args.only in (None, "stamp"):
        g = np.arange(128, dtype=np.int32)
        x, y, z = (v.ravel() for v in np.meshgrid(g, g, g, indexing="ij"))
        ball = (x - 63.5) ** 2 + (y - 63.5) ** 2 + (z - 63.5) ** 2 <= 64.0 ** 2
        solid = np.stack([x[ball], y[ball], z[ball]], axis=1).astype(np.int32)
        rng = np.random.default_rng(1)
        sparse = np.unique(rng.integers(0, 128, size=(52000, 3)).astype(np.int32), axis=0)
        for name, xyz in (("solid ball in 128^3", solid), ("sparse in 128^3", sparse)):
            mats = (np.arange(len(xyz)) % 250 + 1).astype(np.uint32)
            model = t.model_create(xyz, mats)
            for place_name, (axis, flip) in (("identity", ((0, 1, 2), 0)), ("rotated", ((2, 0, 1), 5))):
                offset = (c - 60, c - 40, c - 70)
                place = ST.placement(offset, axis, flip, model)
                written = t.volume_stamp_models(place, _ffi.STAMP_SET, 1.0)
                rec = {"case": "stamp SET", "model": name, "placement": place_name, "model_voxels": len(xyz), "written": written}
                rec["stamp"] = times_ms(lambda: t.volume_stamp_models(place, _ffi.STAMP_SET, 1.0), args.reps, args.warmup)
                rec["stamp_keep"] = times_ms(lambda: t.volume_stamp_models(place, _ffi.STAMP_KEEP, 1.0), args.reps, args.warmup)
                rec["stamp_erase"] = times_ms(lambda: t.volume_stamp_models(place, _ffi.STAMP_ERASE), args.reps, args.warmup)
                if not args.no_baseline:
                    ones = np.ones(len(xyz), dtype=np.float32)

                    def replaced():
                        t.volume_set_voxels(world_voxels(xyz, offset, axis, flip), mats, ones)
                    rec["replaced_route_host_map_and_set_voxels"] = times_ms(replaced, args.baseline_reps, 1)
                    rec["speedup"] = round(rec["replaced_route_host_map_and_set_voxels"]["ms_median"] / rec["stamp"]["ms_median"], 1)
                print(json.dumps(rec), flush=True)
            t.model_destroy(model)

    if args.only in (None, "capture"):
        h = int(T.height(p, np.array([[c, c]], dtype=np.int32))[0])
        lo = (c - 128, max(0, min(n - 256, h - 128)), c - 128)
        hi = tuple(v + 256 for v in lo)
        model = t.volume_capture_model(lo, hi)
        voxels = t.last_capture_voxels
        info = t.model_download(model)[2]
        t.model_destroy(model)
        made = []

        def capture():
            made.append(t.volume_capture_model(lo, hi))
        rec = {"case": "capture 256^3 of the terrain", "region_lo": lo, "voxels": voxels, "levels": info["levels"], "capture": times_ms(capture, args.reps, args.warmup)}
        for m in made:
            t.model_destroy(m)
        # what the capture reads: the region's densities for the bounds, the tight box's densities for the brick masks, one id per voxel
        box = np.prod(np.array(info["hi"]) - np.array(info["lo"]))
        rec["bytes_read"] = int(4 * 256 ** 3 + 4 * box + 4 * voxels)
        rec["region_bytes_at_8_per_voxel"] = 8 * 256 ** 3
        rec["read_GBps_over_the_whole_call"] = round(rec["bytes_read"] / (rec["capture"]["ms_median"] * 1e-3) / 1e9, 1)
        if not args.no_baseline:
            def replaced():
                d, m = t.volume_download()
                sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
                zz, yy, xx = np.nonzero(d[sl] > 0)
                made.append(t.model_create(np.stack([xx, yy, zz], axis=1).astype(np.int32), m[sl][zz, yy, xx]))
            rec["replaced_route_download_select_model_create"] = times_ms(replaced, max(2, args.baseline_reps // 2), 1)
            rec["speedup"] = round(rec["replaced_route_download_select_model_create"]["ms_median"] / rec["capture"]["ms_median"], 1)
        print(json.dumps(rec), flush=True)
    t.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
