"""Cost of instanced voxel models on the benchmark frame: 3840x2160, pose A, the 1024^3 world, with N = 0, 16, 256, 1024 seeded
instances of a 32^3 and of a 128^3 model placed in view (in front of the terrain the pixel they stand on sees).  Prints, per case, the
frame time of the plain entry (blok_hip_trace_primary_device) and of the instanced one, and how many pixels the instances win.
Kernel times: run it under  rocprofv3 --kernel-trace --stats -- python scripts/instance_timing.py  (profiles/)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def ball(edge: int, seed: int):
    rng = np.random.default_rng(seed)
    r = edge / 2
    g = np.stack(np.meshgrid(*[np.arange(edge)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = np.linalg.norm(g + 0.5 - r, axis=1)
    xyz = g[(d <= r) & ((g[:, 0] < r) | (g[:, 1] < r) | (d > 0.6 * r))]      # a ball with a cut-out wedge: orientation shows
    return xyz.astype(np.int32), rng.integers(1, 200, size=len(xyz)).astype(np.uint32)


def placements(n, hits, cam, w, h, edge, seed):
    """n instances whose boxes are centred at 0.6 of the way to the world surface along random live pixels' rays."""
    from blok_amd import world as W                                       # noqa: F401
    from blok_amd._ffi import INSTANCE
    rng = np.random.default_rng(seed)
    flat = hits.reshape(-1)
    live = np.flatnonzero(flat["hit"] == 1)
    pick = rng.choice(live, size=n, replace=True)
    px, py = pick % w, pick // w
    c = cam[0]
    u = ((2 * (px + 0.5) / w - 1) * c["tan_half_fov"] * c["aspect"])[:, None]
    v = ((1 - 2 * (py + 0.5) / h) * c["tan_half_fov"])[:, None]
    d = c["fwd"][None] + c["right"][None] * u + c["up"][None] * v
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = c["pos"][None] + d * (0.6 * flat["t"][pick])[:, None]
    table = np.zeros(n, dtype=INSTANCE)
    perms = [(a, b, cc) for a in range(3) for b in range(3) for cc in range(3) if len({a, b, cc}) == 3]
    for i in range(n):
        table[i]["model"] = 0
        table[i]["offset"] = np.round(p[i] - edge / 2).astype(np.int32)
        table[i]["axis"] = perms[rng.integers(6)]
        table[i]["flip"] = rng.integers(8)
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--counts", default="0,16,256,1024")
    ap.add_argument("--edges", default="32,128")
    args = ap.parse_args()
    import torch
    from blok_amd import world as W
    from blok_amd.tracer import HipTracer
    from blok_amd._ffi import INSTANCE_NONE
    import bench

    w, h = args.width, args.height
    t0 = time.time()
    packed = bench.build_world(args.n, 0xB10C0001)
    print(f"world built in {time.time() - t0:.1f} s", flush=True)
    tr = HipTracer(w, h).init()
    tr.add_world(packed)
    cam = W.scene_camera(args.n, 0, w, h, 0xB10C0001)
    world_hits = tr.draw_frame(cam)
    hits = torch.empty((w * h, 4), dtype=torch.int32, device="cuda")
    rgba = torch.empty(w * h, dtype=torch.int32, device="cuda")
    ids = torch.empty(w * h, dtype=torch.int32, device="cuda")

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(args.reps):
            start.record()
            fn()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end))
        return float(np.median(times))

    plain = timed(lambda: tr.draw_frame_device(cam, hits.data_ptr(), rgba.data_ptr(), stream=torch.cuda.current_stream().cuda_stream))
    print(json.dumps({"entry": "plain", "frame_ms": round(plain, 4)}), flush=True)
    for edge in (int(e) for e in args.edges.split(",")):
        model = tr.model_create(*ball(edge, edge))
        for count in (int(c) for c in args.counts.split(",")):
            table = placements(count, world_hits, cam, w, h, edge, seed=count + edge) if count else placements(1, world_hits, cam, w, h, edge, 1)[:0]
            table["model"] = model
            dev = torch.from_numpy(table.view(np.uint8).copy()).cuda() if count else None
            ptr = dev.data_ptr() if count else 0
            s = torch.cuda.current_stream().cuda_stream
            ms = timed(lambda: tr.trace_primary_instanced_device(cam, ptr, count, hits.data_ptr(), rgba.data_ptr(), ids.data_ptr(), stream=s))
            torch.cuda.synchronize()
            won = int((ids.cpu().numpy().view(np.uint32) != INSTANCE_NONE).sum())
            print(json.dumps({"entry": "instanced", "model_edge": edge, "instances": count, "frame_ms": round(ms, 4),
                              "added_ms": round(ms - plain, 4), "pixels_won": won, "screen_fraction": round(won / (w * h), 4)}), flush=True)
        tr.model_destroy(model)
    tr.shutdown()


if __name__ == "__main__":
    main()
