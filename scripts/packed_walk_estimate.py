"""Estimate of what walking a resting view's rays packed by measured length would save (the packed walk): wave trips of
walk_loop per 8x8 wave as today, against the same rays regrouped inside areas of 16, 32 and 64 pixels by descending trip count, 64
consecutive rays per wave.  Bands of 64 rows every 216 rows of the 4K frame; every ray starts behind the ideal bound of its 8x8 tile grown
by one pixel (the nearest visible hit there, less two voxels), and a tile without a hit in its grown footprint is not walked.  CPU trip
counts from the root through the host harness — not GPU measurements.

    python scripts/packed_walk_estimate.py [pose]
"""
import sys, ctypes as C
sys.path.insert(0, '.')
import numpy as np
from blok_amd import world as W
from tests import harness_ffi as H, oracle_ffi as O
n = 1024; pose = int(sys.argv[1]) if len(sys.argv) > 1 else 0
cm = W.ChunkManager(128, 1.0); cm.generate_scene(n); cm.rebuild_dirty_chunks(); pw = cm.pack_chunks_to_gpu_svo()
hk = H.HostKernel(pw.nodes, pw.sub_chunks)
L = H.lib()
L.hh_trace_rect_stats2.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 6 + [C.c_void_p] * 4
Wd, Ht, B, FIXED = 3840, 2160, 64, 4
cam = W.scene_camera(n, pose, Wd, Ht)
today = 0; lane_trips = 0; waves = 0; heavy = []
packed = {16: 0, 32: 0, 64: 0}; groups = {16: 0, 32: 0, 64: 0}
for y0 in range(0, Ht - B + 1, 216):
    w, h = Wd, B
    def run(ts):
        out = np.zeros(w * h, dtype=O.HIT); it = np.zeros(w * h, dtype=np.uint32)
        L.hh_trace_rect_stats2(hk.h, C.c_void_p(cam.ctypes.data), Wd, Ht, 0, y0, w, h, None if ts is None else C.c_void_p(ts.ctypes.data), None,
                               C.c_void_p(out.ctypes.data), C.c_void_p(it.ctypes.data))
        return out, it.reshape(h, w)
    out, _ = run(None)
    t = np.where(out['hit'] == 1, out['t'], np.inf).reshape(h, w).astype(np.float32)
    # nearest hit of every 8x8 tile grown by one pixel (inside the band)
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
    per_wave = it.reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3))[live]
    today += int(per_wave.sum()); waves += per_wave.size; lane_trips += int(it[walked].sum()); heavy.append(per_wave)
    for area in packed:
        for ay in range(0, h, area):
            for ax in range(0, w, area):
                sel = walked[ay:ay + area, ax:ax + area]
                c = np.sort(it[ay:ay + area, ax:ax + area][sel])[::-1]
                if c.size:
                    packed[area] += int(c[::64].sum()); groups[area] += (c.size + 63) // 64
heavy = np.sort(np.concatenate(heavy))[::-1]
print(f"pose {pose}: {waves} walking waves, trips per wave {today / waves:.2f}, lane utilisation {lane_trips / (64 * today):.2f}, "
      f"share of all trips held by the heaviest 10 % of waves {heavy[:len(heavy) // 10].sum() / heavy.sum():.2f}")
for area in packed:
    print(f"    regrouped inside {area} x {area} pixels: {packed[area] / today:.3f} of today's wave trips ({groups[area]} waves); "
          f"with {FIXED} trips of fixed cost per wave on both sides {(packed[area] + FIXED * groups[area]) / (today + FIXED * waves):.3f}")
