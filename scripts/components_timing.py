"""Cost of blok_hip_volume_label_components and blok_hip_volume_capture_component: host clock around each blocking call,
median of --reps after --warmup, on a keyed volume, against the route they replace (volume_download, then blok_components_label on the
host, and scipy.ndimage.label where it imports) at the sizes the host can hold.  One JSON line per case.

    python scripts/components_timing.py [--size 1024] [--reps 20] [--warmup 3] [--baseline-max 512] [--only terrain|random|solid] [--no-baseline]
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

from blok_amd import _ffi                                      # noqa: E402
from blok_amd import terrain as T                              # noqa: E402
from blok_amd.components import label_components_host          # noqa: E402
from blok_amd.tracer import HipTracer                          # noqa: E402


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def measure(t, name, n, args, baseline):
    """Labels the whole box of the volume as it stands; the capture of the largest component that does not touch the floor."""
    count, voxels = t.volume_label_components()
    rec = {"case": name, "volume": n, "components": count, "voxels": voxels,
           "snapshot_bytes": 4 * n ** 3 + 40 * count + 16 * ((n ** 3 + 63) // 64 + 1)}
    rec["label"] = times_ms(lambda: t.volume_label_components(), args.reps, args.warmup)
    rec["mask_bytes_read"] = 8 * ((n + 3) // 4) ** 3
    # the largest floating component: the table is fetched in pages, only the columns that decide are kept
    best = None
    page = 1 << 20
    for at in range(0, count, page):
        r = t.volume_components_download(at, min(page, count - at))
        r = r[r["touches"] & 8 == 0]
        if len(r):
            top = r[np.argmax(r["n_voxels"])]
            if best is None or top["n_voxels"] > best["n_voxels"]:
                best = top.copy()
    if best is None:
        rec["capture_largest_floating"] = None
    else:
        made = []

        def capture():
            made.append(t.volume_capture_component(int(best["label"]))[0])
        rec["capture_largest_floating"] = {"voxels": int(best["n_voxels"]), "box": (best["hi"] - best["lo"]).tolist(), **times_ms(capture, args.reps, args.warmup)}
        for m in made:
            t.model_destroy(m)
    if baseline:
        got = {}

        def download():
            got["d"] = t.volume_download()[0]
        rec["replaced_route_download"] = times_ms(download, 2, 1)
        if n <= args.baseline_max:
            rec["replaced_route_host_label"] = times_ms(lambda: label_components_host(got["d"], label_capacity=0, component_capacity=0), 2, 0)
            rec["speedup_over_download_and_host_label"] = round((rec["replaced_route_download"]["ms_median"] + rec["replaced_route_host_label"]["ms_median"]) /
                                                                rec["label"]["ms_median"], 1)
            try:
                from scipy import ndimage
                rec["scipy_ndimage_label"] = times_ms(lambda: ndimage.label(got["d"] > 0), 2, 0)
            except ImportError:
                pass
        got.clear()
    print(json.dumps(rec), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-max", type=int, default=512, help="largest box the host labels")
    ap.add_argument("--only", choices=["terrain", "random", "solid"], default=None)
    ap.add_argument("--no-baseline", action="store_true", help="the new entries alone (a profiler pass)")
    args = ap.parse_args()
    t = HipTracer(64, 64).init()
    rng = np.random.default_rng(1)

    if args.only in (None, "terrain"):
        n = args.size
        t.volume_create((0, 0, 0), (n, n, n))
        p = T.default_params(n, 0xB10C0001)
        filled = t.volume_generate_terrain(p)
        print(json.dumps({"case": "setup", "volume": n, "terrain_voxels": filled, "keyed": t.volume_refresh_counts()[2] == 0}), flush=True)
        measure(t, "(a) terrain with caves", n, args, not args.no_baseline)
        heights = T.height(p, rng.integers(16, n - 16, size=(100, 2)).astype(np.int32))
        for k in range(100):                                   # 100 brushes of radius 8 at and below the surface
            xz = rng.integers(16, n - 16, size=2)
            y = int(np.clip(heights[k] - rng.integers(0, 24), 16, n - 16))
            t.volume_apply_brush((float(xz[0]) + 0.5, y + 0.5, float(xz[1]) + 0.5), 8.0, 0.0, 1)
        measure(t, "(b) the same after 100 SUBTRACT brushes of radius 8", n, args, False)
        t.volume_destroy()

    if args.only in (None, "random"):
        for n in (256, 512):
            d = (rng.random((n, n, n), dtype=np.float32) < 0.3116).astype(np.float32)
            t.volume_create((0, 0, 0), (n, n, n))
            t.volume_upload(d, np.ones((n, n, n), dtype=np.uint32))
            del d
            measure(t, "(c) random fill p = 0.3116", n, args, not args.no_baseline)
            t.volume_destroy()

    if args.only in (None, "solid"):
        n = 512
        t.volume_create((0, 0, 0), (n, n, n))
        t.volume_upload(np.ones((n, n, n), dtype=np.float32), np.ones((n, n, n), dtype=np.uint32))
        measure(t, "(d) solid box", n, args, not args.no_baseline)
        t.volume_destroy()
    t.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
