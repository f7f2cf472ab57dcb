"""Cost of posed models in the path-traced frame: 3840x2160, pose A, the 1024^3 world, 8 spp, 2 bounces, the placements of
scripts/instance_timing.py.  Per case four ways, alternated in one process:
  (a) blok_hip_trace_paths_instanced_device over the placements as lattice instances: the yardstick;
  (b) blok_hip_trace_paths_posed_device over the same placements as identity poses (blok_pose_from_instance): the same pixels;
  (c) the same models turned by 30 degrees about +y around their boxes' centres;
  (d) ... and scaled by 2.
Prints the median frame time of each with min..max and the pixels whose first hit is a placed model.  Kernel times: run it under
rocprofv3 --kernel-trace --stats -- python scripts/posed_paths_timing.py."""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=2)
    ap.add_argument("--cases", default="32:16,32:256,128:16", help="model edge:placements, comma separated")
    args = ap.parse_args()
    import torch
    from blok_amd import pose as P
    from blok_amd import world as W
    from blok_amd.tracer import HipTracer
    from blok_amd._ffi import INSTANCE_NONE
    from instance_timing import ball, placements
    import bench

    w, h = args.width, args.height
    t0 = time.time()
    packed = bench.build_world(args.n, 0xB10C0001)
    print(f"world built in {time.time() - t0:.1f} s", flush=True)
    tr = HipTracer(w, h).init()
    tr.add_world(packed)
    cam = W.scene_camera(args.n, 0, w, h, 0xB10C0001)
    world_hits = tr.draw_frame(cam)
    n = w * h
    color = torch.empty(n * 4, dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def once(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    def on_device(records):
        return torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).cuda()

    models = {}
    for case in args.cases.split(","):
        edge, count = (int(v) for v in case.split(":"))
        if edge not in models:
            models[edge] = tr.model_create(*ball(edge, edge))
        table = placements(count, world_hits, cam, w, h, edge, seed=count + edge)
        table["model"] = models[edge]
        centre = (edge / 2.0,) * 3
        at = [tuple(float(o) + edge / 2.0 for o in inst["offset"]) for inst in table]      # the centre of each placement's box (a cube: any orientation)
        tables = {"a instances": on_device(table),
                  "b identity poses": on_device(np.concatenate([P.from_instance(inst, 1.0) for inst in table])),
                  "c yaw 30": on_device(np.concatenate([P.rotation(models[edge], math.radians(30.0), 0.0, 0.0, 1.0, centre, p) for p in at])),
                  "d yaw 30, scale 2": on_device(np.concatenate([P.rotation(models[edge], math.radians(30.0), 0.0, 0.0, 2.0, centre, p) for p in at]))}

        def launch(name):
            common = dict(color_ptr=color.data_ptr(), ids_ptr=ids.data_ptr(), spp=args.spp, max_bounces=args.bounces, frame_index=1, stream=s)
            if name.startswith("a"):
                return lambda: tr.trace_paths_instanced_device(cam, tables[name].data_ptr(), count, **common)
            return lambda: tr.trace_paths_posed_device(cam, 0, 0, tables[name].data_ptr(), count, **common)

        ways = {name: launch(name) for name in tables}
        for _ in range(args.warmup):
            for fn in ways.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in ways}
        for _ in range(args.reps):                 # alternating
            for name, fn in ways.items():
                times[name].append(once(fn))
        out = {"model_edge": edge, "placements": count, "spp": args.spp, "bounces": args.bounces, "frames": args.reps}
        for name, fn in ways.items():
            fn()
            torch.cuda.synchronize()
            won = int((ids.cpu().numpy().view(np.uint32) != INSTANCE_NONE).sum())
            t = times[name]
            out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3),
                         "pixels_won": won, "screen_fraction": round(won / n, 4)}
        out["b/a"] = round(out["b identity poses"]["median_ms"] / out["a instances"]["median_ms"], 3)
        out["c/b"] = round(out["c yaw 30"]["median_ms"] / out["b identity poses"]["median_ms"], 3)
        print(json.dumps(out), flush=True)
    tr.shutdown()


if __name__ == "__main__":
    main()
