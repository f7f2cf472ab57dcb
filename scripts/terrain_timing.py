"""Cost of blok_hip_volume_generate_terrain: host clock around each blocking call, median of --reps after --warmup, the
rebuild that follows, the fill floor (two hipMemsetAsync over the density and id ranges, timed the same way) and the route it replaces
(host evaluation + volume_upload of the same box).  One JSON line per case.

    python scripts/terrain_timing.py [--sizes 256,1024] [--reps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402


def median_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--upload", action="store_true", help="also time the replaced route: host evaluation + volume_upload")
    args = ap.parse_args()
    import torch
    for n in [int(s) for s in args.sizes.split(",")]:
        t = HipTracer(64, 64).init()
        t.volume_create((0, 0, 0), (n, n, n))
        cells = n ** 3
        # the floor: the runtime's own fill, two hipMemsetAsync over arrays of the density's and the ids' sizes
        a, b = torch.empty(cells, dtype=torch.float32, device="cuda"), torch.empty(cells, dtype=torch.int32, device="cuda")
        hip = C.CDLL([line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line][0])
        hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]

        def fill():
            for buf in (a, b):
                if hip.hipMemsetAsync(buf.data_ptr(), 0, 4 * cells, None) != 0:
                    raise RuntimeError("hipMemsetAsync failed")
            if hip.hipDeviceSynchronize() != 0:
                raise RuntimeError("hipDeviceSynchronize failed")
        med, lo, hi = median_ms(fill, args.reps, args.warmup)
        print(json.dumps({"case": "floor: two hipMemsetAsync", "volume": n, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                          "bytes_per_s": round(8 * cells / (med * 1e-3))}), flush=True)
        del a, b
        for caves in (True, False):
            for name, flags in (("replace", 0), ("shell", T.SHELL | T.CLOSE_SIDES), ("add", T.ADD)):
                p = T.default_params(n, 0xB10C0001)
                p.flags = flags
                if not caves:
                    p.cave_octaves = 0
                gen, reb, written = [], [], 0
                for i in range(args.warmup + args.reps):
                    if flags & T.ADD:
                        t.volume_upload()                         # ADD starts from an empty box each time
                        t.volume_rebuild()
                    t0 = time.perf_counter()
                    written = t.volume_generate_terrain(p)
                    t1 = time.perf_counter()
                    t.volume_rebuild()
                    t2 = time.perf_counter()
                    if i >= args.warmup:
                        gen.append((t1 - t0) * 1e3); reb.append((t2 - t1) * 1e3)
                med = float(np.median(gen))
                stored = cells if not flags & T.ADD else written
                print(json.dumps({"case": f"{name} {'caves' if caves else 'no caves'}", "volume": n, "generate_ms_median": round(med, 3),
                                  "generate_ms_min": round(float(np.min(gen)), 3), "generate_ms_max": round(float(np.max(gen)), 3),
                                  "rebuild_ms_median": round(float(np.median(reb)), 3), "filled_voxels": int(written),
                                  "voxels_evaluated_per_s": round(cells / (med * 1e-3)), "voxels_stored_per_s": round(stored / (med * 1e-3)), "bytes_written_per_s": round(8 * stored / (med * 1e-3))}), flush=True)
        if args.upload:
            p = T.default_params(n, 0xB10C0001)
            t0 = time.perf_counter()
            slabs = [T.eval_box(p, (0, 0, z), (n, n, min(z + 32, n))) for z in range(0, n, 32)]
            host_s = time.perf_counter() - t0
            d = np.concatenate([s[0] for s in slabs]); m = np.concatenate([s[1] for s in slabs])
            del slabs
            med, lo, hi = median_ms(lambda: t.volume_upload(d, m), max(3, args.reps // 4), 1)
            print(json.dumps({"case": "replaced route: volume_upload of host arrays", "volume": n, "upload_ms_median": round(med, 3), "upload_ms_min": round(lo, 3),
                              "upload_ms_max": round(hi, 3), "host_eval_s_one_thread": round(host_s, 2)}), flush=True)
        t.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
