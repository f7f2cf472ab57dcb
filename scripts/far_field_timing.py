"""Cost of the far field ("Scaled models and the far field"): §13's terrain with caves (seed 7) in a --size^3 resident volume as the
world, and the eight boxes around it in x and z as level-K copies — one scaled model each, placed as an instance.  Per K of --levels:

    ring_build   host clock around the eight x (volume_create at the neighbour's place + generate_terrain + reduce + lod_model + model_set_scale)
    primary      the plain first-hit frame (blok_hip_trace_primary_device) against the instanced one, device events, median of --reps
    paths        the same for --spp path-traced frames (color plane only)

at --width x --height from pose A of the box (blok_amd.world.scene_camera, pose 0: bench.py's).  Kernel medians of the
binning and instance-pass kernels come from a run of its own under  rocprofv3 --kernel-trace --stats -- python scripts/far_field_timing.py ...

    python scripts/far_field_timing.py [--size 1024] [--levels 2,3] [--reps 20] [--spp 8] [--out profiles/far_field_timing.txt]

Every invocation appends one JSON line per K to --out.
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

from blok_amd import lod as L                  # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd import world as W                # noqa: E402
from blok_amd._ffi import INSTANCE, INSTANCE_NONE          # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

SEED = 7


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--levels", default="2,3")
    ap.add_argument("--min-count", type=int, default=1)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "far_field_timing.txt"))
    args = ap.parse_args()
    import torch
    n, w, h = args.size, args.width, args.height
    p = T.default_params(n, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    cam = W.scene_camera(n, 0, w, h)                     # pose A
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.reps):
            start.record()
            fn()
            end.record()
            end.synchronize()
            ms.append(start.elapsed_time(end))
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4)}

    for K in (int(k) for k in args.levels.split(",")):
        rec = {"volume": n, "level": K, "min_count": args.min_count, "frame": [w, h], "reps": args.reps}
        t = HipTracer(w, h).init()
        table, voxels = [], []
        t0 = time.perf_counter()
        for dz in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dz == 0:
                    continue
                t.volume_create((dx * n, 0, dz * n), (n, n, n))
                t.volume_generate_terrain(p)
                info = t.volume_reduce(None, None, K, L.VOTE_EXPOSED)
                model = t.volume_lod_model(K, args.min_count)
                t.model_set_scale(model, K)
                voxels.append(t.last_capture_voxels)
                rec_i = np.zeros(1, dtype=INSTANCE)
                rec_i["model"], rec_i["axis"] = model, (0, 1, 2)
                rec_i["offset"] = [int(c) << K for c in info["level"][0][K - 1]["clo"]]
                table.append(rec_i[0])
        rec["ring_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["ring_voxels"] = voxels
        t.volume_create((0, 0, 0), (n, n, n))
        rec["terrain_voxels"] = t.volume_generate_terrain(p)
        t.volume_rebuild(W.scene_materials(SEED))
        table = np.array(table, dtype=INSTANCE)
        t.check_instances(table)
        dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        hits = torch.empty((w * h, 4), dtype=torch.int32, device="cuda")
        rgba = torch.empty(w * h, dtype=torch.int32, device="cuda")
        ids = torch.empty(w * h, dtype=torch.int32, device="cuda")
        color = torch.empty((w * h, 4), dtype=torch.float32, device="cuda")
        rec["primary_plain"] = timed(lambda: t.draw_frame_device(cam, hits.data_ptr(), rgba.data_ptr(), stream=stream))
        rec["primary_instanced"] = timed(lambda: t.trace_primary_instanced_device(cam, dev.data_ptr(), len(table), hits.data_ptr(), rgba.data_ptr(),
                                                                                  ids.data_ptr(), stream=stream))
        torch.cuda.synchronize()
        rec["pixels_won"] = int((ids.cpu().numpy().view(np.uint32) != INSTANCE_NONE).sum())
        rec["paths_plain"] = timed(lambda: t.trace_paths_device(cam, color.data_ptr(), spp=args.spp, stream=stream))
        rec["paths_instanced"] = timed(lambda: t.trace_paths_instanced_device(cam, dev.data_ptr(), len(table), color_ptr=color.data_ptr(), spp=args.spp,
                                                                              stream=stream))
        torch.cuda.synchronize()
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
