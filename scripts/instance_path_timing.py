"""Cost of instances in the path-traced frame: 3840x2160, pose A, the 1024^3 world, 8 spp, 2 bounces (draw_frame_rt's defaults), the
placements of scripts/instance_timing.py.  Per case: the median frame time of the plain entry (blok_hip_trace_paths_device) and of the
instanced one (blok_hip_trace_paths_instanced_device), taken alternately in the same process, and the pixels whose first hit is an instance.
Kernel times (the instance BVH build among them): run it under  rocprofv3 --kernel-trace --stats -- python scripts/instance_path_timing.py."""
from __future__ import annotations

import argparse
import json
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=2)
    ap.add_argument("--cases", default="32:0,32:16,32:256,32:1024,128:16", help="model edge:instances, comma separated")
    ap.add_argument("--build-only", default="", help="instance counts whose BVH build alone is launched --reps times (for rocprofv3)")
    args = ap.parse_args()
    import torch
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

    models = {}
    for case in args.cases.split(","):
        edge, count = (int(v) for v in case.split(":"))
        if edge not in models:
            models[edge] = tr.model_create(*ball(edge, edge))
        table = placements(max(count, 1), world_hits, cam, w, h, edge, seed=count + edge)[:count]
        table["model"] = models[edge]
        dev = torch.from_numpy(table.view(np.uint8).copy()).cuda() if count else None
        ptr = dev.data_ptr() if count else 0
        plain = lambda: tr.trace_paths_device(cam, color.data_ptr(), args.spp, args.bounces, frame_index=1, stream=s)
        inst = lambda: tr.trace_paths_instanced_device(cam, ptr, count, color_ptr=color.data_ptr(), ids_ptr=ids.data_ptr(), spp=args.spp,
                                                       max_bounces=args.bounces, frame_index=1, stream=s)
        for _ in range(3):
            plain()
            inst()
        torch.cuda.synchronize()
        tp, ti = [], []
        for _ in range(args.reps):                 # alternating
            tp.append(once(plain))
            ti.append(once(inst))
        won = int((ids.cpu().numpy().view(np.uint32) != INSTANCE_NONE).sum())
        print(json.dumps({"model_edge": edge, "instances": count, "plain_ms": round(float(np.median(tp)), 3),
                          "plain_spread_ms": round(float(np.max(tp) - np.min(tp)), 3), "instanced_ms": round(float(np.median(ti)), 3),
                          "instanced_spread_ms": round(float(np.max(ti) - np.min(ti)), 3), "pixels_won": won,
                          "screen_fraction": round(won / n, 4)}), flush=True)
    for count in (int(c) for c in args.build_only.split(",") if c):
        table = placements(count, world_hits, cam, w, h, 32, seed=count)
        table["model"] = models.get(32, 0)
        dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        for _ in range(args.reps):
            tr.debug_build_tlas(dev.data_ptr(), count)
        print(json.dumps({"build_only": count}), flush=True)
    tr.shutdown()


if __name__ == "__main__":
    main()
