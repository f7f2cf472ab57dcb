"""Cost of object motion in the ray-traced frame: 3840x2160, pose A, the 1024^3 world, 256 instances of a 32^3 model (the placements of
scripts/instance_timing.py) that move by one voxel along x every frame (back and forth), spp 1 and 2 bounces by default.
Prints the median frame time of blok_hip_draw_frame_rt_instanced and of blok_hip_draw_frame_rt_instanced_motion, each on its own context
(their post states must not mix) and called alternately in the same process, and how many pixels are tracked instance pixels.
Kernel times (instance_motion_kernel, the two temporal kernels): run it under  rocprofv3 --kernel-trace --stats -- python
scripts/instance_motion_timing.py  (profiles/)."""
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
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--edge", type=int, default=32)
    ap.add_argument("--frames", type=int, default=12, help="measured frames per entry")
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--bounces", type=int, default=2)
    args = ap.parse_args()
    from blok_amd import world as W
    from blok_amd.tracer import HipTracer
    from blok_amd._ffi import INSTANCE_NONE
    from instance_timing import ball, placements
    import bench

    w, h = args.width, args.height
    t0 = time.time()
    packed = bench.build_world(args.n, 0xB10C0001)
    print(f"world built in {time.time() - t0:.1f} s", flush=True)
    plain, motion = HipTracer(w, h).init(), HipTracer(w, h).init()
    cam = W.scene_camera(args.n, 0, w, h, 0xB10C0001)
    for tr in (plain, motion):
        tr.add_world(packed)
        model = tr.model_create(*ball(args.edge, args.edge))
    world_hits = plain.draw_frame(cam)
    base = placements(args.instances, world_hits, cam, w, h, args.edge, seed=args.instances + args.edge)
    base["model"] = model

    def table(k):
        t = base.copy()
        t["offset"][:, 0] += k % 2                                  # one voxel along x, back and forth
        return t

    _, ids, _ = plain.trace_primary_instanced(cam, table(0))
    covered = int((ids != INSTANCE_NONE).sum())
    for k in range(3):                                               # warm-up (and a previous table for the motion entry)
        plain.draw_frame_rt_instanced(cam, table(k), args.spp, args.bounces)
        motion.draw_frame_rt_instanced_motion(cam, table(k), args.spp, args.bounces)
    tp, tm = [], []
    for k in range(3, 3 + args.frames):                              # alternating; each call ends with its frame's host copy
        t = table(k)
        s = time.perf_counter(); plain.draw_frame_rt_instanced(cam, t, args.spp, args.bounces); tp.append(time.perf_counter() - s)
        s = time.perf_counter(); motion.draw_frame_rt_instanced_motion(cam, t, args.spp, args.bounces); tm.append(time.perf_counter() - s)
    hist_p, hist_m = plain.denoise_state()[2], motion.denoise_state()[2]
    inst = ids != INSTANCE_NONE
    print(json.dumps({"instances": args.instances, "model_edge": args.edge, "spp": args.spp, "bounces": args.bounces,
                      "instance_pixels": covered, "screen_fraction": round(covered / (w * h), 4),
                      "rt_instanced_ms": round(1e3 * float(np.median(tp)), 3), "rt_instanced_spread_ms": round(1e3 * float(np.ptp(tp)), 3),
                      "rt_instanced_motion_ms": round(1e3 * float(np.median(tm)), 3),
                      "rt_instanced_motion_spread_ms": round(1e3 * float(np.ptp(tm)), 3),
                      "mean_history_on_instances": {"instanced": round(float(hist_p[inst].mean()), 3),
                                                    "instanced_motion": round(float(hist_m[inst].mean()), 3)}}), flush=True)
    plain.shutdown(); motion.shutdown()


if __name__ == "__main__":
    main()
