"""Cost of blok_hip_volume_apply_shapes on a keyed volume with §13's terrain with caves: host clock around each blocking call,
median of --reps after --warmup, with the spread.  One step per invocation, so that each runs under a time limit of its own:

    stroke     (a) a stroke of 256 capsules of radius 8 as one table, against the only equivalents without it: 256 blok_hip_volume_apply_brush
               calls along the same path (then one wait), and one blok_hip_volume_set_voxels of the same cells
    kernel     (b) three such strokes and nothing else timed: for a run under a kernel trace, which takes the bin and apply kernels alone;
               prints what the apply kernel moves by construction (the tiles with a list, 8 bytes per cell read, 4 per changed value
               written) against the stroke's touched cells x 16 B
    box        (c) one BOX SET over the whole box (8 bytes written per cell, nothing that was there survives) against a memset of the same bytes
    spheres    (d) 4096 spheres of radius 4 scattered over the box: as many commit groups as shapes, the worst case for step 4

    python scripts/shapes_timing.py --step stroke [--size 1024] [--reps 7] [--warmup 2] [--out profiles/shapes_timing.txt]

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

from blok_amd import shapes as SH              # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("stroke", "kernel", "box", "spheres")
N_CAPSULES, RADIUS = 256, 8


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def stroke_points(n):
    """257 points of a helix along x through the middle of the box, on voxel centres: about 3 voxels apart, 40 voxels from the axis."""
    u = np.linspace(0.0, 1.0, N_CAPSULES + 1)
    x = np.floor(0.1 * n + 0.8 * n * u)
    y = np.floor(n / 2 + 40 * np.sin(9 * np.pi * u))
    z = np.floor(n / 2 + 40 * np.cos(9 * np.pi * u))
    return [(float(a) + 0.5, float(b) + 0.5, float(c) + 0.5) for a, b, c in zip(x, y, z)]


def touched(points, n):
    """(world voxels the stroke touches as an (n, 3) int32 array, tiles of 64 x 4 x 4 cells that hold one) from the host build over the
    stroke's bounding box."""
    p = np.array(points)
    lo = np.maximum(np.floor(p.min(axis=0)).astype(int) - RADIUS - 1, 0)
    hi = np.minimum(np.floor(p.max(axis=0)).astype(int) + RADIUS + 2, n)
    ext = hi - lo
    d = np.zeros((ext[2], ext[1], ext[0]), np.float32)
    m = np.zeros(d.shape, np.uint32)
    SH.apply_host(d, m, tuple(int(c) for c in lo), SH.stroke(points, RADIUS, SH.SET, 1, 1.0))
    z, y, x = np.nonzero(d)
    xyz = np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=1).astype(np.int32)
    tiles = np.unique(np.stack([xyz[:, 0] // 64, xyz[:, 1] // 4, xyz[:, 2] // 4], axis=1), axis=0)
    return xyz, len(tiles)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shapes_timing.txt"))
    args = ap.parse_args()
    n = args.size
    rec = {"step": args.step, "volume": n}
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))
    p = T.default_params(n, 0xB10C0001)
    rec["terrain_voxels"] = t.volume_generate_terrain(p)
    rec["keyed"] = t.volume_refresh_counts()[2] == 0
    points = stroke_points(n)
    if args.step in ("stroke", "kernel"):
        xyz, tiles = touched(points, n)
        table = SH.stroke(points, RADIUS, SH.ADD, value=1.0)
        rec["capsules"], rec["radius"], rec["touched_cells"], rec["touched_tiles"] = len(table), RADIUS, len(xyz), tiles
        if args.step == "stroke":
            rec["written"] = t.volume_apply_shapes(table)
            rec["apply_shapes"] = times_ms(lambda: t.volume_apply_shapes(table), args.reps, args.warmup)

            import torch

            def brushes():
                for c in points[:-1]:
                    t.volume_apply_brush(c, float(RADIUS), 1.0, 0)
                torch.cuda.synchronize()                              # (the brush only enqueues; the other two calls block)
            rec["apply_brush_x256"] = times_ms(brushes, args.reps, args.warmup)
            ids, ones = np.ones(len(xyz), np.uint32), np.ones(len(xyz), np.float32)
            rec["set_voxels_same_cells"] = times_ms(lambda: t.volume_set_voxels(xyz, ids, ones), args.reps, args.warmup)
            rec["brush_chain_over_apply_shapes"] = round(rec["apply_brush_x256"]["ms_median"] / rec["apply_shapes"]["ms_median"], 2)
            rec["set_voxels_over_apply_shapes"] = round(rec["set_voxels_same_cells"]["ms_median"] / rec["apply_shapes"]["ms_median"], 2)
        else:
            for _ in range(3):
                t.volume_apply_shapes(table)
            # by construction: every tile with a list is read whole, both arrays; ADD of 1.0 over a terrain changes densities only
            rec["apply_bytes_read"] = tiles * 1024 * 8
            rec["touched_cells_x_16"] = len(xyz) * 16
            rec["read_over_touched_x_16"] = round(rec["apply_bytes_read"] / rec["touched_cells_x_16"], 2)
    elif args.step == "box":
        import torch
        whole = SH.box((0, 0, 0), (n, n, n), SH.SET, 3, 1.0)
        rec["written"] = t.volume_apply_shapes(whole)
        rec["box_set"] = times_ms(lambda: t.volume_apply_shapes(whole), args.reps, args.warmup)
        buf = torch.empty(8 * n ** 3, dtype=torch.uint8, device="cuda")

        def memset():
            buf.zero_()
            torch.cuda.synchronize()
        rec["memset_same_bytes"] = times_ms(memset, args.reps, args.warmup)
        rec["bytes_written"] = 8 * n ** 3
        rec["box_set_over_memset"] = round(rec["box_set"]["ms_median"] / rec["memset_same_bytes"]["ms_median"], 2)
    else:
        rng = np.random.default_rng(1)
        centres = rng.integers(8, n - 8, size=(4096, 3))
        table = np.concatenate([SH.sphere(tuple(float(v) + 0.5 for v in c), 4, SH.ADD, value=1.0) for c in centres])
        rec["spheres"], rec["written"] = len(table), t.volume_apply_shapes(table)
        before = t.volume_refresh_counts()
        rec["apply_shapes"] = times_ms(lambda: t.volume_apply_shapes(table), args.reps, args.warmup)
        rec["commits_per_call"] = (sum(t.volume_refresh_counts()) - sum(before)) // (args.reps + args.warmup)
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
