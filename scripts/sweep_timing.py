"""Cost of blok_hip_volume_sweep_models: host clock around each blocking call, median of --reps after --warmup, on a keyed
volume with §13's terrain.  (a) one solid 128^3 ball swept down from 300 voxels above the ground; (b) 1 000 placements of models of
8 - 200 voxels, in one call and as 1 000 single calls; (c) the same answers by the route the entry replaces, volume_download plus
blok_sweep_voxels on the host.  One JSON line per case.

    python scripts/sweep_timing.py [--size 1024] [--reps 20] [--warmup 3] [--baseline-reps 2] [--no-baseline]
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
from blok_amd import sweep as SW               # noqa: E402
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true", help="the new entry alone (a profiler pass)")
    args = ap.parse_args()
    n = args.size
    down = 3                                   # -Y
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))
    p = T.default_params(n, 0xB10C0001)
    filled = t.volume_generate_terrain(p)
    print(json.dumps({"case": "setup", "volume": n, "terrain_voxels": filled, "keyed": t.volume_refresh_counts()[2] == 0}), flush=True)
    c = n // 2
    ground = int(T.height(p, np.array([[c, c]], dtype=np.int32))[0])

    # (a) the ball
    g = np.arange(128, dtype=np.int32)
    x, y, z = (v.ravel() for v in np.meshgrid(g, g, g, indexing="ij"))
    inside = (x - 63.5) ** 2 + (y - 63.5) ** 2 + (z - 63.5) ** 2 <= 64.0 ** 2
    ball_xyz = np.stack([x[inside], y[inside], z[inside]], axis=1).astype(np.int32)
    ball = t.model_create(ball_xyz, np.ones(len(ball_xyz), dtype=np.uint32))
    ball_offset = (c - 64, min(ground + 300, n - 130), c - 64)
    ball_place = ST.placement(ball_offset, model=ball)
    got = t.volume_sweep_models(ball_place, down, n, _ffi.SWEEP_BOX_IS_SOLID)[0]
    rec_a = {"case": "a: solid 128^3 ball swept down", "model_voxels": len(ball_xyz), "offset": ball_offset,
             "result": [int(got["n_overlap"]), int(got["travel"]), int(got["blocked"])]}
    rec_a["sweep"] = times_ms(lambda: t.volume_sweep_models(ball_place, down, n, _ffi.SWEEP_BOX_IS_SOLID), args.reps, args.warmup)
    print(json.dumps(rec_a), flush=True)

    # (b) debris: ten blobs of 8 - 200 voxels, 1 000 placements in the air over the terrain
    rng = np.random.default_rng(7)
    blobs, blob_ids = [], []
    for k in range(10):
        count = int(rng.integers(8, 201))
        xyz = np.unique(np.clip(np.rint(rng.normal(0.0, 1.0 + count ** (1.0 / 3.0) / 1.5, size=(4 * count, 3))), -8, 8).astype(np.int32), axis=0)[:count]
        blobs.append(xyz)
        blob_ids.append(t.model_create(xyz, np.full(len(xyz), k + 1, dtype=np.uint32)))
    which = rng.integers(0, 10, size=1000)
    orient = rng.integers(0, 48, size=1000)
    from itertools import permutations
    orientations = [(axis, flip) for axis in permutations((0, 1, 2)) for flip in range(8)]
    offsets = np.stack([rng.integers(32, n - 32, size=1000), rng.integers(n // 2, n - 32, size=1000), rng.integers(32, n - 32, size=1000)], axis=1)
    table = np.concatenate([ST.placement(tuple(offsets[i]), *orientations[orient[i]], blob_ids[which[i]]) for i in range(1000)])
    results = t.volume_sweep_models(table, down, n, _ffi.SWEEP_BOX_IS_SOLID)
    rec_b = {"case": "b: 1000 placements of 8-200 voxels", "model_voxels": [len(b) for b in blobs], "blocked": int(results["blocked"].sum()),
             "travel_median": float(np.median(results["travel"]))}
    rec_b["table"] = times_ms(lambda: t.volume_sweep_models(table, down, n, _ffi.SWEEP_BOX_IS_SOLID), args.reps, args.warmup)

    def singles():
        for i in range(1000):
            t.volume_sweep_models(table[i:i + 1], down, n, _ffi.SWEEP_BOX_IS_SOLID)
    rec_b["singles"] = times_ms(singles, args.reps, args.warmup)
    rec_b["table_over_singles"] = round(rec_b["table"]["ms_median"] / rec_b["singles"]["ms_median"], 4)
    print(json.dumps(rec_b), flush=True)

    # (c) the route replaced: the volume to the host, every voxel walked there
    if not args.no_baseline:
        held = {}

        def download():
            held["d"] = t.volume_download()[0]
        rec_c = {"case": "c: volume_download + blok_sweep_voxels", "download": times_ms(download, args.baseline_reps, 0)}
        d = held["d"]
        host = {}

        def host_ball():
            host["a"] = SW.sweep_voxels_host(d, (0, 0, 0), ball_xyz, ball_place, down, n, _ffi.SWEEP_BOX_IS_SOLID)
        rec_c["host_ball"] = times_ms(host_ball, args.baseline_reps, 0)

        def host_table():
            host["b"] = [SW.sweep_voxels_host(d, (0, 0, 0), blobs[which[i]], table[i:i + 1], down, n, _ffi.SWEEP_BOX_IS_SOLID) for i in range(1000)]
        rec_c["host_table"] = times_ms(host_table, args.baseline_reps, 0)
        rec_c["same_answers"] = bool(host["a"].tobytes() == got.tobytes() and all(host["b"][i].tobytes() == results[i].tobytes() for i in range(1000)))
        rec_c["ball_speedup"] = round((rec_c["download"]["ms_median"] + rec_c["host_ball"]["ms_median"]) / rec_a["sweep"]["ms_median"], 1)
        rec_c["table_speedup"] = round((rec_c["download"]["ms_median"] + rec_c["host_table"]["ms_median"]) / rec_b["table"]["ms_median"], 1)
        print(json.dumps(rec_c), flush=True)
    t.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
