"""Estimate of what a listed ray of a resting view still repeats once it restarts at its own hit (the node words of a
packed list): how much of the descent from the root to the hit's brick a wave's scalar chain (trace_core.h: walk_enter_wave) already shares.
scripts/own_start_estimate.py's bands — 64 rows of the 4K frame over the 1024^3 scene, here every 432 rows — traced through the host
harness; the hit pixels of each 32 x 32 area in the list's order (wave tile by wave tile, row by row inside one), 64 consecutive per group.
m is the lowest level at which all the hit voxels of a group share a cell (0: one voxel; `levels`: they part at the root); the chain shares
the descents above that cell, so a group makes max(m - 1, 0) per-lane descents of its levels - 1.  Also the distinct bricks (4^3 cells) a
group's hits lie in.  CPU counts from the records — not GPU measurements.

    python scripts/brick_restart_estimate.py [pose ...]
"""
import sys, ctypes as C
sys.path.insert(0, '.')
import numpy as np
from blok_amd import world as W
from tests import harness_ffi as H, oracle_ffi as O
n = 1024; poses = [int(a) for a in sys.argv[1:]] or [0, 1, 2]
cm = W.ChunkManager(128, 1.0); cm.generate_scene(n); cm.rebuild_dirty_chunks(); pw = cm.pack_chunks_to_gpu_svo()
hk = H.HostKernel(pw.nodes, pw.sub_chunks)
L = H.lib()
L.hh_trace_rect_stats2.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 6 + [C.c_void_p] * 4
L.hh_tree_nodes.restype = C.c_void_p
L.hh_tree_nodes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
origin, count = np.zeros(3, dtype=np.int32), C.c_size_t(0)
L.hh_tree_nodes(hk.h, C.byref(count), C.c_void_p(origin.ctypes.data))      # a voxel's digits are those of its tree coordinate
Wd, Ht, B, STEP, AREA = 3840, 2160, 64, 432, 32
levels = hk.levels

print(f"| Pose | Groups | Groups by m = 0..{levels} | Per-lane descents per group (of {levels - 1}) | Distinct bricks per group |")
print("|---|---|---|---|---|")
for pose in poses:
    cam = W.scene_camera(n, pose, Wd, Ht)
    by_m = np.zeros(levels + 1, dtype=np.int64); bricks = 0
    for y0 in range(0, Ht - B + 1, STEP):
        out = np.zeros(Wd * B, dtype=O.HIT); it = np.zeros(Wd * B, dtype=np.uint32)
        L.hh_trace_rect_stats2(hk.h, C.c_void_p(cam.ctypes.data), Wd, Ht, 0, y0, Wd, B, None, None, C.c_void_p(out.ctypes.data), C.c_void_p(it.ctypes.data))
        out = out.reshape(B, Wd)
        hit = out['hit'] == 1
        vox = out['voxel'].astype(np.int64) - origin
        for ay in range(0, B, AREA):
            for ax in range(0, Wd, AREA):
                ys, xs = np.mgrid[ay:ay + AREA, ax:ax + AREA]
                ys, xs = ys.reshape(-1), xs.reshape(-1)
                order = np.lexsort((xs, ys, xs // 8, ys // 8))      # wave tile by wave tile, row by row inside one
                ys, xs = ys[order], xs[order]
                keep = hit[ys, xs]
                v = vox[ys[keep], xs[keep]]
                for g in range(0, len(v), 64):
                    q = v[g:g + 64]
                    diff = int(np.bitwise_or.reduce((q ^ q[0]).reshape(-1)))
                    m = 0 if diff == 0 else min((diff.bit_length() - 1) // 2 + 1, levels)
                    by_m[m] += 1
                    bricks += len(np.unique(q >> 2, axis=0))
    groups = int(by_m.sum())
    per_lane = sum(int(c) * max(m - 1, 0) for m, c in enumerate(by_m)) / max(groups, 1)
    print(f"| {'ABC'[pose] if pose < 3 else pose} | {groups} | {', '.join(str(int(c)) for c in by_m)} | {per_lane:.2f} | {bricks / max(groups, 1):.1f} |", flush=True)
