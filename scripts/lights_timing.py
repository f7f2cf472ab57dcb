"""Cost of emissive voxels as lights on a 1024^3 terrain with caves whose ore material glows, 3840x2160, 8 spp, 2 bounces.
One JSON line per part:
  table:  blok_hip_volume_extract_quads over the whole box, and blok_hip_lights_from_quads alone (host clock around the blocking calls,
          median of --reps), with the quads, the lights, their faces and the owned materials;
  frame_before_any_table: blok_hip_trace_paths_device back to back before the process has built any table (what a caller without lights runs);
  frame:  the same entry with the table installed, with it cleared, and with a table of one light that no surface point can face (below the
          world, looking down: never a shadow ray, so the lit kernel's body and its three draws alone), alternated in one process (device
          events, median);
          with a library that has no light table (BLOK_HIP_LIB = a build of the parent commit) only the second, so that a job which
          alternates this script under both libraries sets the lit frame, the cleared frame and the parent's frame side by side.

    python scripts/lights_timing.py [--n 1024] [--reps 7] [--warmup 2] [--skip-table]
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
    ap.add_argument("--skip-table", action="store_true", help="do not time the table's build (the frame part only)")
    args = ap.parse_args()
    import torch
    from blok_amd import _ffi
    from blok_amd import terrain as T
    from blok_amd import world as W
    from blok_amd.tracer import HipTracer

    n, w, h = args.n, args.width, args.height
    tr = HipTracer(w, h).init()
    has_lights = hasattr(tr._lib, "blok_hip_lights_from_quads") and getattr(tr._lib.blok_hip_lights_from_quads, "argtypes", None) is not None
    p = T.default_params(n, 7)
    assert p.cave_octaves > 0
    mats = W.scene_materials().copy()
    mats["emission"][p.ore_material] = (4.0, 2.2, 0.4)
    tr.volume_create((0, 0, 0), (n, n, n))
    filled = tr.volume_generate_terrain(p)
    tr.volume_rebuild(mats)
    top = float(p.base_height + p.amplitude)
    cam = W.camera_look_at((0.12 * n, top + 0.08 * n, 0.10 * n), (n / 2.0, float(p.base_height) + 0.15 * n, n / 2.0), 60.0, w, h)
    out = {"part": "world", "n": n, "filled_voxels": filled, "library": "with light table" if has_lights else "without light table"}
    print(json.dumps(out), flush=True)

    def host_ms(fn, reps, warmup=1):
        ms = []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3)}

    color = torch.empty(w * h * 4, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def frame():
        tr.trace_paths_device(cam, color.data_ptr(), args.spp, args.bounces, frame_index=1, stream=s)

    def once():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        frame()
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    t = [once() for _ in range(args.warmup + 2 * args.reps)][args.warmup:]
    print(json.dumps({"part": "frame_before_any_table", "size": f"{w}x{h}", "spp": args.spp, "bounces": args.bounces, "frames": len(t), "median_ms": round(float(np.median(t)), 3),
                      "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3)}), flush=True)

    info = None
    if has_lights:
        from blok_amd import lights as LT
        counts = tr.volume_extract_quads(count_only=True)
        lib, ctx = tr._lib, tr._ctx

        def extract():
            tr._check(lib.blok_hip_volume_extract_quads(ctx, None, None, 0, None, None))

        if not args.skip_table:
            t_extract = host_ms(extract, 3)
            t_lights = host_ms(lambda: LT.from_quads(tr), args.reps)
            t_both = host_ms(lambda: (extract(), LT.from_quads(tr)), 3)
        else:
            extract()
            t_extract = t_lights = t_both = None
        info = LT.from_quads(tr)
        print(json.dumps({"part": "table", "quads": counts[0], "exposed_faces": counts[1], "lights": int(info["n"][0]), "light_faces": int(info["n_faces"][0]),
                          "owned_materials": int(info["n_owned"][0]), "table_bytes": int(info["bytes"][0]), "extract_quads": t_extract, "lights_from_quads": t_lights,
                          "extract_then_lights": t_both}), flush=True)

    ways = ["cleared", "lit", "one light never faced"] if has_lights and info is not None and int(info["n"][0]) else ["cleared"]
    far = None
    if has_lights:
        far = np.zeros(1, dtype=_ffi.LIGHT)
        far["lo"], far["du"], far["dv"], far["material"], far["face"] = (0, -2000, 0), 1, 1, p.ore_material, 3
    times = {k: [] for k in ways}
    means = {}
    for rep in range(args.warmup + args.reps):            # alternating
        for k in ways:
            if has_lights:
                from blok_amd import lights as LT
                if k == "lit":
                    LT.from_quads(tr)
                elif k == "cleared":
                    LT.clear(tr)
                else:
                    LT.set(tr, far)
            t = once()
            if rep >= args.warmup:
                times[k].append(t)
            means[k] = float(color.view(-1, 4)[:, :3].mean().item())
    out = {"part": "frame", "size": f"{w}x{h}", "spp": args.spp, "bounces": args.bounces, "frames": args.reps}
    for k in ways:
        t = times[k]
        out[k] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3), "mean_colour": round(means[k], 6)}
    if "lit" in out:
        out["lit/cleared"] = round(out["lit"]["median_ms"] / out["cleared"]["median_ms"], 3)
        out["one light never faced/cleared"] = round(out["one light never faced"]["median_ms"] / out["cleared"]["median_ms"], 3)
    print(json.dumps(out), flush=True)
    tr.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
