"""Cost of the light grid's build on a 1024^3 terrain with caves whose ore material glows.  One JSON line per part:
  table: the light table the grid is built over (blok_hip_volume_extract_quads over the whole box, blok_hip_lights_from_quads);
  grid:  blok_hip_build_light_grid at each of --cells x --reach (host clock around the blocking call, median of --reps): cells, cells
         with a list, items, the longest list, bytes, ms;
  frame: blok_hip_trace_paths_device at 3840x2160, 8 spp, 2 bounces with the table alone (path_kernel_lit) and with a grid of c = 5,
         reach 1, share 192 installed (path_kernel_lit_grid), alternated (device events, median);
  cave:  a camera four voxels in front of the table's largest light, looking along its plane: 16 frames of each loop at 640x360, 8 spp,
         2 bounces; the mean over the pixels of the per-pixel variance of the luminance across the frames, and the mean colour.

    python scripts/light_grid_timing.py [--n 1024] [--reps 7] [--cells 4,5,6] [--reach 1,2] [--skip-frame]
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="4,5,6")
    ap.add_argument("--reach", default="1,2")
    ap.add_argument("--skip-frame", action="store_true")
    args = ap.parse_args()
    import torch
    from blok_amd import lights as LT
    from blok_amd import terrain as T
    from blok_amd import world as W
    from blok_amd._ffi import BlokError
    from blok_amd.tracer import HipTracer

    n, w, h = args.n, args.width, args.height
    tr = HipTracer(w, h).init()
    p = T.default_params(n, 7)
    mats = W.scene_materials().copy()
    mats["emission"][p.ore_material] = (4.0, 2.2, 0.4)
    tr.volume_create((0, 0, 0), (n, n, n))
    filled = tr.volume_generate_terrain(p)
    tr.volume_rebuild(mats)
    tr._check(tr._lib.blok_hip_volume_extract_quads(tr._ctx, None, None, 0, None, None))
    info = LT.from_quads(tr)
    print(json.dumps({"part": "table", "n": n, "filled_voxels": filled, "lights": int(info["n"][0]), "light_faces": int(info["n_faces"][0])}), flush=True)

    for c in [int(v) for v in args.cells.split(",")]:
        for reach in [int(v) for v in args.reach.split(",")]:
            ms, g = [], None
            try:
                for i in range(1 + args.reps):
                    t0 = time.perf_counter()
                    g = LT.build_grid(tr, c, reach, 192)
                    if i >= 1:
                        ms.append((time.perf_counter() - t0) * 1e3)
            except BlokError as e:
                print(json.dumps({"part": "grid", "cell_log2": c, "reach": reach, "refused": str(e)}), flush=True)
                continue
            print(json.dumps({"part": "grid", "cell_log2": c, "reach": reach, "dim": [int(d) for d in g["dim"][0]], "cells": int(g["n_cells"][0]),
                              "cells_with_a_list": int(g["n_nonempty"][0]), "items": int(g["n_items"][0]), "longest_list": int(g["max_items"][0]),
                              "bytes": int(g["bytes"][0]), "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3),
                              "max_ms": round(float(np.max(ms)), 3)}), flush=True)
    if args.skip_frame:
        tr.shutdown()
        return 0

    top = float(p.base_height + p.amplitude)
    cam = W.camera_look_at((0.12 * n, top + 0.08 * n, 0.10 * n), (n / 2.0, float(p.base_height) + 0.15 * n, n / 2.0), 60.0, w, h)
    color = torch.empty(w * h * 4, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def once():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        tr.trace_paths_device(cam, color.data_ptr(), args.spp, args.bounces, frame_index=1, stream=s)
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    ways = ["table alone", "table and grid"]
    times, sums = {k: [] for k in ways}, {}
    for rep in range(args.warmup + args.reps):            # alternating
        for k in ways:
            if k == "table and grid":
                LT.build_grid(tr, 5, 1, 192)
            else:
                LT.clear_grid(tr)
            t = once()
            if rep >= args.warmup:
                times[k].append(t)
            sums[k] = float(color.double().sum().item())
    out = {"part": "frame", "size": f"{w}x{h}", "spp": args.spp, "bounces": args.bounces, "frames": args.reps, "mean_colour": {k: sums[k] / (w * h * 4) for k in ways}}
    for k in ways:
        t = times[k]
        out[k] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3)}
    print(json.dumps(out), flush=True)

    # the cave: beside the largest light of the table
    table = LT.download(tr)
    L = table[int(np.argmax(table["du"].astype(np.int64) * table["dv"]))]
    a = int(L["face"]) >> 1
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    centre = L["lo"].astype(np.float64)
    centre[u] += 0.5 * float(L["du"]); centre[v] += 0.5 * float(L["dv"])
    normal = np.zeros(3); normal[a] = -1.0 if int(L["face"]) & 1 else 1.0
    along = np.zeros(3); along[u] = 1.0
    eye = centre + 4.0 * normal
    cw, ch = 640, 360
    cave = W.camera_look_at(tuple(eye), tuple(eye + 8.0 * along - 2.0 * normal), 70.0, cw, ch)
    small = HipTracer(cw, ch)
    tr.shutdown()
    tr = small.init()
    tr.volume_create((0, 0, 0), (n, n, n))
    tr.volume_generate_terrain(p)
    tr.volume_rebuild(mats)
    tr._check(tr._lib.blok_hip_volume_extract_quads(tr._ctx, None, None, 0, None, None))
    LT.from_quads(tr)
    lum = np.array([0.2126, 0.7152, 0.0722])
    res = {"part": "cave", "size": f"{cw}x{ch}", "spp": args.spp, "bounces": args.bounces, "frames": 16, "light": {"lo": [int(x) for x in L["lo"]], "du": int(L["du"]), "dv": int(L["dv"]), "face": int(L["face"])}}
    for k in ways:
        if k == "table and grid":
            LT.build_grid(tr, 5, 1, 192)
        frames = np.stack([tr.trace_paths(cave, args.spp, args.bounces, frame_index=f)["color"][..., :3].astype(np.float64) @ lum for f in range(16)])
        res[k] = {"mean_luminance": float(frames.mean()), "mean_per_pixel_variance": float(frames.var(axis=0, ddof=1).mean())}
    res["variance global / grid"] = res[ways[0]]["mean_per_pixel_variance"] / max(res[ways[1]]["mean_per_pixel_variance"], 1e-300)
    print(json.dumps(res), flush=True)
    tr.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
