"""Cost of object motion for poses in the ray-traced frame: 3840x2160, pose A, the 1024^3 world, 256 placements of a 32^3 model (those of
scripts/instance_timing.py, given as poses about their boxes' centres) that every frame turn by one degree about +y, spp 1 and 2 bounces
by default.  Prints the median frame time of blok_hip_draw_frame_rt_posed and of blok_hip_draw_frame_rt_posed_motion, each on its own
context (their post states must not mix) and called alternately in the same process, how many pixels are pose pixels and the mean history
length on them.  --posed-only: only blok_hip_draw_frame_rt_posed, the same frames (for a library of another revision through BLOK_HIP_LIB,
which has no motion entry).
Kernel times (pose_motion_prepare_kernel, posed_motion_kernel, the temporal kernels): run it under  rocprofv3 --kernel-trace --stats -- python
scripts/pose_motion_timing.py  (profiles/)."""
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
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--edge", type=int, default=32)
    ap.add_argument("--frames", type=int, default=12, help="measured frames per entry")
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--bounces", type=int, default=2)
    ap.add_argument("--degrees", type=float, default=1.0, help="every pose's turn about +y per frame")
    ap.add_argument("--posed-only", action="store_true")
    args = ap.parse_args()
    from blok_amd import pose as P
    from blok_amd import world as W
    from blok_amd.tracer import HipTracer
    from blok_amd._ffi import INSTANCE_NONE, POSE_ID
    from instance_timing import ball, placements
    import bench

    w, h = args.width, args.height
    t0 = time.time()
    packed = bench.build_world(args.n, 0xB10C0001)
    print(f"world built in {time.time() - t0:.1f} s", flush=True)
    tracers = [HipTracer(w, h).init()] + ([] if args.posed_only else [HipTracer(w, h).init()])
    cam = W.scene_camera(args.n, 0, w, h, 0xB10C0001)
    for tr in tracers:
        tr.add_world(packed)
        model = tr.model_create(*ball(args.edge, args.edge))
    plain = tracers[0]
    world_hits = plain.draw_frame(cam)
    base = placements(args.poses, world_hits, cam, w, h, args.edge, seed=args.poses + args.edge)
    centres = base["offset"].astype(np.float64) + args.edge / 2.0
    half = (args.edge / 2.0,) * 3

    def table(k):
        return np.concatenate([P.rotation(model, yaw=math.radians(args.degrees * k + 7.0 * i), pivot_local=half, position=tuple(c))
                               for i, c in enumerate(centres)])

    tables = [table(k) for k in range(3 + args.frames)]
    _, ids, _ = plain.trace_primary_posed(cam, None, tables[-1])
    posed = (ids != INSTANCE_NONE) & ((ids & POSE_ID) != 0)
    covered = int(posed.sum())
    for k in range(3):                                               # warm-up (and previous tables for the motion entry)
        plain.draw_frame_rt_posed(cam, None, tables[k], args.spp, args.bounces)
        if not args.posed_only:
            tracers[1].draw_frame_rt_posed_motion(cam, None, tables[k], args.spp, args.bounces)
    tp, tm = [], []
    for k in range(3, 3 + args.frames):                              # alternating; each call ends with its frame's host copy
        s = time.perf_counter(); plain.draw_frame_rt_posed(cam, None, tables[k], args.spp, args.bounces); tp.append(time.perf_counter() - s)
        if not args.posed_only:
            s = time.perf_counter(); tracers[1].draw_frame_rt_posed_motion(cam, None, tables[k], args.spp, args.bounces); tm.append(time.perf_counter() - s)
    out = {"poses": args.poses, "model_edge": args.edge, "spp": args.spp, "bounces": args.bounces, "degrees_per_frame": args.degrees,
           "pose_pixels": covered, "screen_fraction": round(covered / (w * h), 4),
           "rt_posed_ms": round(1e3 * float(np.median(tp)), 3), "rt_posed_spread_ms": round(1e3 * float(np.ptp(tp)), 3),
           "mean_history_on_poses": {"posed": round(float(plain.denoise_state()[2][posed].mean()), 3)}}
    if not args.posed_only:
        out |= {"rt_posed_motion_ms": round(1e3 * float(np.median(tm)), 3), "rt_posed_motion_spread_ms": round(1e3 * float(np.ptp(tm)), 3)}
        out["mean_history_on_poses"]["posed_motion"] = round(float(tracers[1].denoise_state()[2][posed].mean()), 3)
    print(json.dumps(out), flush=True)
    for tr in tracers:
        tr.shutdown()


if __name__ == "__main__":
    main()
