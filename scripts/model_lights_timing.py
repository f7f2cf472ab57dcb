"""Cost of emissive models as lights.  One JSON line per part:
  table:  blok_hip_model_lights for a 32^3 and a 128^3 model (a third of the cells filled, a tenth of those glowing), host clock around the
          blocking call, median of --reps, with the model's bricks' voxels and the faces found;
  prefix: blok_hip_instance_lights_info over 16, 256 and 4096 instances (host clock around the blocking probe: the staging of the table,
          the one-workgroup kernel and the download of the n + 1 words);
  frame:  3840x2160, 8 spp, 2 bounces over the --n^3 terrain with caves whose ore glows, alternated in one process (device events, median):
          the world's table only (blok_hip_trace_paths_device); 256 lantern instances over the terrain without a model table
          (path_kernel_lit through the instanced entry); the same with the model table (path_kernel_lit_placed).

    python scripts/model_lights_timing.py [--n 1024] [--reps 7] [--warmup 2]
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
    args = ap.parse_args()
    import torch
    from blok_amd import lights as LT
    from blok_amd import terrain as T
    from blok_amd import world as W
    from blok_amd._ffi import INSTANCE
    from blok_amd.tracer import HipTracer

    n, w, h = args.n, args.width, args.height
    tr = HipTracer(w, h).init()
    p = T.default_params(n, 7)
    mats = W.scene_materials().copy()
    mats["emission"][p.ore_material] = (4.0, 2.2, 0.4)
    glow = int(p.ore_material)
    tr.volume_create((0, 0, 0), (n, n, n))
    tr.volume_generate_terrain(p)
    tr.volume_rebuild(mats)

    def host_ms(fn, reps, warmup=1):
        ms = []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3)}

    rng = np.random.default_rng(11)
    for edge in (32, 128):
        cells = np.argwhere(rng.random((edge, edge, edge)) < 1.0 / 3.0).astype(np.int32)
        ids = np.where(rng.random(len(cells)) < 0.1, glow, 1).astype(np.uint32)
        model = tr.model_create(cells, ids)
        t = host_ms(lambda: LT.model_lights(tr, model), args.reps)
        print(json.dumps({"part": "table", "model": f"{edge}^3", "voxels": len(cells), "faces": int(LT.model_lights_info(tr, model)["n"][0]), "model_lights": t}), flush=True)
        LT.model_lights_clear(tr, model)

    cube = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    lantern = tr.model_create(cube, np.full(27, glow, dtype=np.uint32))
    LT.model_lights(tr, lantern)
    top = int(p.base_height + p.amplitude)

    def table_of(count):
        t = np.zeros(count, dtype=INSTANCE)
        t["model"], t["axis"] = lantern, (0, 1, 2)
        t["offset"][:, 0] = rng.integers(8, n - 8, count)
        t["offset"][:, 2] = rng.integers(8, n - 8, count)
        t["offset"][:, 1] = min(top + 4, n - 4)
        return t

    for count in (16, 256, 4096):
        table = table_of(count)
        t = host_ms(lambda: LT.instance_lights_info(tr, table), args.reps)
        header, _ = LT.instance_lights_info(tr, table)
        print(json.dumps({"part": "prefix", "instances": count, "a_inst": int(header["a_inst"][0]), "n_lit": int(header["n_lit"][0]), "instance_lights_info": t}), flush=True)

    tr.volume_extract_quads()
    world = LT.from_quads(tr)
    cam = W.camera_look_at((0.12 * n, float(top) + 0.08 * n, 0.10 * n), (n / 2.0, float(p.base_height) + 0.15 * n, n / 2.0), 60.0, w, h)
    color = torch.empty(w * h * 4, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    inst = torch.from_numpy(table_of(256).view(np.uint8)).cuda()

    def once(instanced):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        if instanced:
            tr.trace_paths_instanced_device(cam, inst.data_ptr(), 256, color.data_ptr(), spp=args.spp, max_bounces=args.bounces, frame_index=1, stream=s)
        else:
            tr.trace_paths_device(cam, color.data_ptr(), args.spp, args.bounces, frame_index=1, stream=s)
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    ways = ["world table only", "256 lanterns, no model table", "256 lanterns, model table"]
    times = {k: [] for k in ways}
    means = {}
    for rep in range(args.warmup + args.reps):            # alternating
        for k in ways:
            if k == ways[2]:
                LT.model_lights(tr, lantern)
            else:
                LT.model_lights_clear(tr, lantern)
            t = once(k != ways[0])
            if rep >= args.warmup:
                times[k].append(t)
            means[k] = float(color.view(-1, 4)[:, :3].mean().item())
    out = {"part": "frame", "size": f"{w}x{h}", "spp": args.spp, "bounces": args.bounces, "frames": args.reps, "world_light_faces": int(world["n_faces"][0])}
    for k in ways:
        t = times[k]
        out[k] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3), "mean_colour": round(means[k], 6)}
    print(json.dumps(out), flush=True)
    tr.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
