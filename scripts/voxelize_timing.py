"""Cost of blok_hip_volume_voxelize_mesh on a 1024^3 volume: host clock around each blocking call, median of --reps after
--warmup, and the rebuild that follows.  One JSON line per case.

    python scripts/voxelize_timing.py [--reps 20] [--warmup 3] [--subdiv 8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from blok_amd.tracer import HipTracer          # noqa: E402
from tests import voxelize_meshes as M         # noqa: E402


def work_lists(t, pos, tri, mats, solid) -> dict:
    """One more call with BLOK_VOXELIZE_STATS set: the sizes of its work lists (pairs, launches, touched bricks, columns), from stderr."""
    t.volume_upload()
    os.environ["BLOK_VOXELIZE_STATS"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            t.volume_voxelize_mesh(pos, tri, materials=mats, solid=solid)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["BLOK_VOXELIZE_STATS"]
        f.seek(0)
        line = [l for l in f.read().decode().splitlines() if l.startswith("[voxelize]")][-1].split()[1:]
    return {k: int(v) for k, v in zip(line[0::2], line[1::2]) if k != "triangles"}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--subdiv", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    n = args.size
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))

    def bumpy(v):
        return 0.04 * np.sin(9.0 * v[:, 0]) * np.cos(7.0 * v[:, 1]) + 0.03 * np.sin(11.0 * v[:, 2])
    c = n / 2 + 0.37
    sphere = M.icosphere([c, c - 0.21, c + 0.13], 0.44 * n, args.subdiv, bumpy)
    cube = M.box([0.02 * n + 0.3, 0.02 * n + 0.6, 0.02 * n + 0.1], [0.98 * n - 0.4, 0.98 * n - 0.2, 0.98 * n - 0.7])
    mats256 = (np.arange(len(sphere[1])) % 256).astype(np.uint32)
    cases = [("icosphere surface", sphere, None, False), ("icosphere solid", sphere, None, True),
             ("icosphere surface 256 materials", sphere, mats256, False), ("icosphere solid 256 materials", sphere, mats256, True),
             ("box12 surface", cube, None, False), ("box12 solid", cube, None, True)]
    for name, (pos, tri), mats, solid in cases:
        vox_ms, reb_ms, written = [], [], 0
        for i in range(args.warmup + args.reps):
            t.volume_upload()                                  # an empty box each time
            t.volume_rebuild()
            t0 = time.perf_counter()
            written = t.volume_voxelize_mesh(pos, tri, materials=mats, solid=solid)
            t1 = time.perf_counter()
            t.volume_rebuild()
            t2 = time.perf_counter()
            if i >= args.warmup:
                vox_ms.append((t1 - t0) * 1e3)
                reb_ms.append((t2 - t1) * 1e3)
        stats = work_lists(t, pos, tri, mats, solid)
        med = float(np.median(vox_ms))
        print(json.dumps({"case": name, "volume": n, "triangles": int(len(tri)), "voxelize_ms_median": round(med, 3),
                          "voxelize_ms_min": round(float(np.min(vox_ms)), 3), "voxelize_ms_max": round(float(np.max(vox_ms)), 3),
                          "rebuild_ms_median": round(float(np.median(reb_ms)), 3), "voxels_written": int(written),
                          "triangles_per_s": round(len(tri) / (med * 1e-3)), **stats}), flush=True)
    t.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
