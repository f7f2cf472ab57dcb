"""How often each block of the walk loop (trace_core.h: walk_loop) runs and with how many lanes, from the host harness's per-ray event logs — to
price a change of the loop before building it (the cycle weights per block are in profiles/r06_walk_isa.txt).

The benchmark frame (4K over the 1024^3 world), poses A, B, C.  Sampled 32x32-pixel beam tiles; every ray of a tile starts 2 voxels before the
tile's nearest hit (what the beam pre-pass provides); the 8x8 wave tiles of a beam tile are walked as waves of 64 lanes in lockstep: trip i of a
wave is trip i of each of its lanes, and a block runs in a trip when at least one lane wants it.  Per pose:
  trips per walking wave, live lanes per trip; how often the descend block and the step block run and with how many lanes, how often both;
  ascents per step; descents and steps per lane; the lengths of descent cascades (descents in a row).
The harness walks every ray from the root (the kernel's shared prefix of descents, walk_enter_wave, is not modelled): descents per lane are an
upper bound by the shared ones (2-4 of them, scripts/r04/common_prefix_estimate.py).  A lane's last trip (a report, or the walk's end) logs no event
and is counted as a trip of the top and the exit test alone.
usage: walk_blocks.py [--n 1024] [--stride-x 11] [--stride-y 9]      (output: profiles/r06_walk_blocks.txt)"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from blok_amd import world as W                     # noqa: E402
from tests import harness_ffi as H, oracle_ffi as O   # noqa: E402

CAP = 192          # event bytes kept per ray (longer walks are truncated: counted and reported)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--stride-x", type=int, default=11, help="every stride-th beam tile in x")
    ap.add_argument("--stride-y", type=int, default=9)
    a = ap.parse_args()
    n, Wd, Ht = a.n, a.width, a.height
    cm = W.ChunkManager(128, 1.0); cm.generate_scene(n); cm.rebuild_dirty_chunks()
    pw = cm.pack_chunks_to_gpu_svo(W.scene_materials())
    hk = H.HostKernel(pw.nodes, pw.sub_chunks); L = H.lib()
    L.hh_trace_rect_stats.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 6 + [C.c_void_p] * 3
    L.hh_trace_rect_events.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 6 + [C.c_void_p, C.c_uint32, C.c_void_p]
    print(f"{n}^3 world, {Wd}x{Ht}, every ({a.stride_x}, {a.stride_y})-th 32x32 beam tile, waves of 8x8 pixels, walks from the root")
    for pose in (0, 1, 2):
        cam = W.scene_camera(n, pose, Wd, Ht)
        waves = trips = live = d_trips = d_lanes = s_trips = s_lanes = both = asc = 0
        lane_desc, lane_step, cascades, truncated = [], [], [], 0
        for by in range(2, Ht // 32, a.stride_y):
            for bx in range(3, Wd // 32, a.stride_x):
                x0, y0 = bx * 32, by * 32
                out = np.zeros(32 * 32, dtype=O.HIT); it = np.zeros(32 * 32, dtype=np.uint32)
                L.hh_trace_rect_stats(hk.h, C.c_void_p(cam.ctypes.data), Wd, Ht, x0, y0, 32, 32, None, C.c_void_p(out.ctypes.data), C.c_void_p(it.ctypes.data))
                t = np.where(out["hit"] == 1, out["t"], np.inf)
                if not np.isfinite(t.min()):
                    continue                                     # a sky tile: its waves do not walk
                ts = np.full(32 * 32, max(float(t.min()) - 2.0, 0.001), dtype=np.float32)
                ev = np.zeros((32, 32, CAP), dtype=np.uint8)
                L.hh_trace_rect_events(hk.h, C.c_void_p(cam.ctypes.data), Wd, Ht, x0, y0, 32, 32, C.c_void_p(ts.ctypes.data), CAP, C.c_void_p(ev.ctypes.data))
                for wy in range(4):
                    for wx in range(4):
                        lanes = ev[wy * 8:wy * 8 + 8, wx * 8:wx * 8 + 8].reshape(64, CAP)
                        kind = lanes & 3                         # 1 descend, 2 step; 0: the walk's start marker (first byte) and the padding
                        count = (kind != 0).sum(axis=1)
                        truncated += int((lanes[:, -1] != 0).sum())
                        seqs = [lanes[k][(kind[k] != 0)] for k in range(64)]
                        T = int(count.max()) + 1
                        waves += 1; trips += T
                        for k in range(64):
                            q = seqs[k]; kd = q & 3; lv = (q >> 2) & 7
                            lane_desc.append(int((kd == 1).sum())); lane_step.append(int((kd == 2).sum()))
                            run = 0
                            for j in range(len(q)):
                                if kd[j] == 1:
                                    run += 1
                                else:
                                    if run:
                                        cascades.append(run)
                                    run = 0
                                    asc += int(j + 1 < len(q) and lv[j + 1] > lv[j])
                            if run:
                                cascades.append(run)
                        for i in range(T):
                            alive = int((count + 1 > i).sum())
                            nd = sum(1 for q in seqs if i < len(q) and (q[i] & 3) == 1)
                            ns = sum(1 for q in seqs if i < len(q) and (q[i] & 3) == 2)
                            live += alive
                            d_trips += nd > 0; d_lanes += nd; s_trips += ns > 0; s_lanes += ns; both += nd > 0 and ns > 0
        ld, ls, cs = np.array(lane_desc), np.array(lane_step), np.array(cascades)
        print(f"pose {'ABC'[pose]}: {waves} walking waves; {trips / waves:.1f} trips per wave, {live / trips:.1f} of 64 lanes live per trip")
        print(f"  descend block: in {d_trips / trips:.2f} of trips with {d_lanes / max(d_trips, 1):.1f} lanes; step block: in {s_trips / trips:.2f} of trips with "
              f"{s_lanes / max(s_trips, 1):.1f} lanes; both in {both / trips:.2f}; an ascent in {asc / max(int(ls.sum()), 1):.2f} of steps")
        print(f"  per lane: {ld.mean():.1f} descents, {ls.mean():.1f} steps; descent cascades: mean length {cs.mean():.2f}, "
              + ", ".join(f"{k}: {np.mean(cs == k):.2f}" for k in range(1, 6)) + f"; logs cut at {CAP} events: {truncated} lanes")


if __name__ == "__main__":
    main()
