"""Estimate of what restarting every listed ray of a resting view where its own walk ended would save (the starts of a
packed list): scripts/packed_walk_estimate.py's recipe — bands of 64 rows every 216 rows of the 4K frame, every ray behind the ideal bound of
its 8x8 tile grown by one pixel, areas of 32 pixels regrouped by descending trip count, 64 consecutive rays per wave — with a start
parameter per ray: a hit ray starts at its own hit t (the records are asserted byte-equal), and in the last two columns a miss ray of a
live tile is given `levels` trips as well (the host harness does not report a miss's last cell; `levels` is its upper bound).  CPU trip
counts from the root through the host harness — not GPU measurements.

    python scripts/own_start_estimate.py [pose ...]
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
Wd, Ht, B, FIXED, AREA = 3840, 2160, 64, 4, 32


def packed_trips(it, walked):
    """Wave trips and waves of the counts regrouped inside areas of AREA pixels by descending count, 64 to a wave."""
    trips = waves = 0
    h, w = it.shape
    for ay in range(0, h, AREA):
        for ax in range(0, w, AREA):
            c = np.sort(it[ay:ay + AREA, ax:ax + AREA][walked[ay:ay + AREA, ax:ax + AREA]])[::-1]
            if c.size:
                trips += int(c[::64].sum()); waves += (c.size + 63) // 64
    return trips, waves


print("| Pose | Trips per listed ray, today | Hits restarted | Packed wave trips vs today (hits restarted) | The same, 4 fixed trips per group | Misses also `levels` trips | The same, 4 fixed trips per group |")
print("|---|---|---|---|---|---|---|")
for pose in poses:
    cam = W.scene_camera(n, pose, Wd, Ht)
    today = [0, 0]; hits_only = [0, 0]; misses_too = [0, 0]; rays = 0; lane_today = 0; lane_own = 0
    for y0 in range(0, Ht - B + 1, 216):
        w, h = Wd, B
        def run(ts):
            out = np.zeros(w * h, dtype=O.HIT); it = np.zeros(w * h, dtype=np.uint32)
            L.hh_trace_rect_stats2(hk.h, C.c_void_p(cam.ctypes.data), Wd, Ht, 0, y0, w, h, None if ts is None else C.c_void_p(ts.ctypes.data), None,
                                   C.c_void_p(out.ctypes.data), C.c_void_p(it.ctypes.data))
            return out, it.reshape(h, w)
        out, _ = run(None)
        hit = (out['hit'] == 1).reshape(h, w)
        t = np.where(hit, out['t'].reshape(h, w), np.inf).astype(np.float32)
        pad = np.pad(t, 1, constant_values=np.inf)
        near = np.full((h // 8, w // 8), np.inf, dtype=np.float32)
        for dy in range(10):
            for dx in range(10):
                near = np.minimum(near, pad[dy:dy + h:8, dx:dx + w:8])
        live = np.isfinite(near)
        ts = np.where(live, np.maximum(near - 2, 0), 9999.0).astype(np.float32).repeat(8, axis=0).repeat(8, axis=1)
        out1, it = run(np.ascontiguousarray(ts))
        assert np.array_equal(out.view(np.uint8), out1.view(np.uint8))
        walked = live.repeat(8, axis=0).repeat(8, axis=1)
        out2, it_own = run(np.ascontiguousarray(np.where(hit, t, ts).astype(np.float32)))
        assert np.array_equal(out.view(np.uint8), out2.view(np.uint8)), "a walk from a hit's own t reports another record"
        assert (it_own[hit] == hk.levels).all()
        it_all = np.where(hit, it_own, np.minimum(it_own, hk.levels))
        for acc, counts in ((today, it), (hits_only, it_own), (misses_too, it_all)):
            a, b = packed_trips(counts, walked); acc[0] += a; acc[1] += b
        rays += int(walked.sum()); lane_today += int(it[walked].sum()); lane_own += int(it_own[walked].sum())
    r = lambda x: (x[0] / today[0], (x[0] + FIXED * x[1]) / (today[0] + FIXED * today[1]))
    print(f"| {'ABC'[pose] if pose < 3 else pose} | {lane_today / rays:.1f} | {lane_own / rays:.1f} | {r(hits_only)[0]:.2f} | {r(hits_only)[1]:.2f} | {r(misses_too)[0]:.2f} | {r(misses_too)[1]:.2f} |", flush=True)
