"""Cost of blok_hip_volume_extract_quads: host clock around each blocking call, median of --reps after --warmup; the
quads, faces and result bytes; the download of the result; the route it replaces (volume_download of the box, and blok_quads_extract on
one host thread where --host-extract allows the size); and a floor: a device copy of arrays of the mask array's and the id array's sizes.
One JSON line per case.

    python scripts/quads_timing.py [--sizes 256,1024] [--reps 20] [--warmup 3] [--host-extract 256]
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

from blok_amd import mesh as M                 # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402
from tests import voxelize_meshes as VM        # noqa: E402


def median_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3), round(float(np.max(ms)), 3)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-extract", type=int, default=256, help="largest size at which the host extraction of the replaced route is timed")
    ap.add_argument("--no-download", action="store_true", help="skip volume_download (the replaced route)")
    args = ap.parse_args()
    import torch
    for n in [int(s) for s in args.sizes.split(",")]:
        t = HipTracer(64, 64).init()
        t.volume_create((0, 0, 0), (n, n, n))
        cells = n ** 3
        # the floor: one device copy each of arrays of the masks' (8 B per 64 voxels) and the ids' (4 B per voxel) sizes: read + write
        a, b = torch.empty(cells // 64, dtype=torch.int64, device="cuda"), torch.empty(cells, dtype=torch.int32, device="cuda")
        a2, b2 = torch.empty_like(a), torch.empty_like(b)

        def copy():
            a2.copy_(a); b2.copy_(b)
            torch.cuda.synchronize()
        med, lo, hi = median_ms(copy, args.reps, args.warmup)
        print(json.dumps({"case": "floor: device copy of mask-sized and id-sized arrays", "volume": n, "ms_median": med, "ms_min": lo, "ms_max": hi,
                          "bytes_read": cells // 8 + 4 * cells}), flush=True)
        del a, b, a2, b2

        def bumpy(v):
            return 0.04 * np.sin(9.0 * v[:, 0]) * np.cos(7.0 * v[:, 1]) + 0.03 * np.sin(11.0 * v[:, 2])
        c = n / 2 + 0.37

        def terrain(caves):
            p = T.default_params(n, 0xB10C0001)
            if not caves:
                p.cave_octaves = 0
            t.volume_generate_terrain(p)

        def sphere():
            t.volume_upload()
            pos, tri = VM.icosphere([c, c - 0.21, c + 0.13], 0.44 * n, 8 if n >= 1024 else 6, bumpy)
            t.volume_voxelize_mesh(pos, tri, material=2, solid=True)

        def checkerboard():
            # over the terrain: the sub-region [0, 256)^3 becomes a checkerboard, written by set_voxels slab by slab
            z, y, x = np.indices((32, 256, 256), dtype=np.int32)
            for z0 in range(0, 256, 32):
                xyz = np.stack([x, y, z + z0], axis=-1).reshape(-1, 3)
                t.volume_set_voxels(xyz, np.ones(len(xyz), np.uint32), ((xyz.sum(axis=1) % 2) == 0).astype(np.float32))
        cases = [("terrain, caves", lambda: terrain(True), None), ("terrain, no caves", lambda: terrain(False), None),
                 ("solid displaced icosphere", sphere, None), ("checkerboard in [0, 256)^3 over the terrain", checkerboard, ((0, 0, 0), (256, 256, 256)))]
        for name, make, region in cases:
            make()
            lo_, hi_ = region if region else (None, None)
            for ignore in (False, True):
                n_quads, n_faces = t.volume_extract_quads(lo_, hi_, ignore, count_only=True)
                def extract():              # the entry alone: the snapshot stays on the device
                    if t._lib.blok_hip_volume_extract_quads(t._ctx, *_region(lo_, hi_), 1 if ignore else 0, None, None) != 0:
                        raise RuntimeError("blok_hip_volume_extract_quads failed")
                call = median_ms(extract, args.reps, args.warmup)
                count = median_ms(lambda: t.volume_extract_quads(lo_, hi_, ignore, count_only=True), args.reps, args.warmup)
                down = median_ms(lambda: t.volume_quads_download(0, n_quads), max(3, args.reps // 4), 1)
                print(json.dumps({"case": name, "volume": n, "ignore_material": ignore, "quads": n_quads, "faces": n_faces, "result_bytes": 32 * n_quads,
                                  "extract_ms_median": call[0], "extract_ms_min": call[1], "extract_ms_max": call[2], "count_only_ms_median": count[0],
                                  "download_ms_median": down[0], "download_ms_min": down[1], "download_ms_max": down[2]}), flush=True)
            if name == "terrain, caves" and not args.no_download:
                # the route it replaces: the whole volume across the bus, then the same extraction on one host thread
                try:
                    t0 = time.perf_counter()
                    d, m = t.volume_download()
                    first = (time.perf_counter() - t0) * 1e3
                    t0 = time.perf_counter()
                    d, m = t.volume_download()
                    second = (time.perf_counter() - t0) * 1e3
                    rec = {"case": "replaced route: volume_download (includes allocating the host arrays)", "volume": n, "bytes": 8 * cells,
                           "download_ms_first": round(first, 1), "download_ms_second": round(second, 1)}
                    if n <= args.host_extract:
                        t0 = time.perf_counter()
                        counts = M.extract_quads_host(d, m, count_only=True)
                        rec.update({"host_extract_s_one_thread": round(time.perf_counter() - t0, 2), "host_quads": counts[0], "host_faces": counts[1]})
                    else:
                        rec["host_extract_s_one_thread"] = "not run at this size"
                    print(json.dumps(rec), flush=True)
                    del d, m
                except MemoryError:
                    print(json.dumps({"case": "replaced route: volume_download", "volume": n, "error": "host arrays do not fit"}), flush=True)
        t.shutdown()
    return 0


def _region(lo, hi):
    import ctypes as C
    return (None if lo is None else (C.c_int32 * 3)(*lo), None if hi is None else (C.c_int32 * 3)(*hi))


if __name__ == "__main__":
    sys.exit(main())
