"""Cost of the sparse brick stream on a keyed volume with §13's terrain with caves: host clock around each blocking call,
median of --reps after --warmup, with the spread.  One step per invocation, so that each runs under a time limit of its own:

    encode | encode-filled   blok_hip_volume_encode_bricks over the whole box, the stream's bytes, and the rate at which the call reads the
                             two dense arrays
    download                 the stream to the host (records and payloads, paged)
    restore                  blok_hip_volume_restore_bricks of the whole box's snapshot
    decode                   blok_hip_volume_decode_bricks of the same stream from host arrays
    undo                     encode + restore of a 64^3 region around a brush stroke
    baseline                 what the stream replaces: blok_hip_volume_download and blok_hip_volume_upload of the same box

    python scripts/bricks_timing.py --step encode [--size 1024] [--reps 10] [--warmup 2] [--out profiles/bricks_timing.txt]

Every invocation appends one JSON line to --out.
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

from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("encode", "encode-filled", "download", "restore", "decode", "undo", "baseline")


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def stream_bytes(info) -> int:
    return 8 + 64 + 24 * int(info["n_bricks"][0]) + 4 * (int(info["n_density"][0]) + int(info["n_material"][0]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bricks_timing.txt"))
    args = ap.parse_args()
    n = args.size
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))
    p = T.default_params(n, 0xB10C0001)
    filled = t.volume_generate_terrain(p)
    rec = {"step": args.step, "volume": n, "terrain_voxels": filled, "dense_bytes": 8 * n ** 3, "keyed": t.volume_refresh_counts()[2] == 0}
    if args.step in ("encode", "encode-filled"):
        only = args.step == "encode-filled"
        info = t.volume_encode_bricks(filled_only=only)
        rec.update({k: int(info[k][0]) for k in ("n_bricks", "n_density", "n_material", "n_voxels")}, stream_bytes=stream_bytes(info))
        rec["encode"] = times_ms(lambda: t.volume_encode_bricks(filled_only=only), args.reps, args.warmup)
        # the whole call — classify, two scans, emit and its wait — against the bytes of the two arrays: a lower bound of the classify pass's rate
        rec["dense_read_TB_per_s"] = round(rec["dense_bytes"] / (rec["encode"]["ms_median"] * 1e-3) / 1e12, 3)
    elif args.step == "download":
        info = t.volume_encode_bricks()
        rec["stream_bytes"] = stream_bytes(info)
        rec["download"] = times_ms(lambda: t.volume_bricks_download(), args.reps, args.warmup)
    elif args.step == "restore":
        t.volume_encode_bricks()
        rec["restore"] = times_ms(lambda: t.volume_restore_bricks(), args.reps, args.warmup)
    elif args.step == "decode":
        info = t.volume_encode_bricks()
        s = t.volume_bricks_download()
        rec["stream_bytes"] = stream_bytes(info)
        rec["decode"] = times_ms(lambda: t.volume_decode_bricks(*s), args.reps, args.warmup)
    elif args.step == "undo":
        c = n // 2
        ground = int(T.height(p, np.array([[c, c]], dtype=np.int32))[0])
        lo = (c - 32, max(0, min(ground - 32, n - 64)), c - 32)
        hi = tuple(v + 64 for v in lo)
        centre = tuple(float(v + 32) for v in lo)

        def stroke():
            t.volume_encode_bricks(lo, hi)
            t.volume_apply_brush(centre, 24.0, 1.0, 0)
            t.volume_restore_bricks()
        brush = times_ms(lambda: t.volume_apply_brush(centre, 24.0, 1.0, 0), args.reps, args.warmup)
        info = t.volume_encode_bricks(lo, hi)
        rec.update(region=[lo, hi], stream_bytes=stream_bytes(info), brush_alone=brush)
        rec["encode_brush_restore"] = times_ms(stroke, args.reps, args.warmup)
        rec["encode"] = times_ms(lambda: t.volume_encode_bricks(lo, hi), args.reps, args.warmup)
        rec["restore"] = times_ms(lambda: t.volume_restore_bricks(), args.reps, args.warmup)
    else:
        held = {}

        def download():
            held["v"] = t.volume_download()
        rec["volume_download"] = times_ms(download, max(2, args.reps // 3), 1)
        d, m = held["v"]
        rec["volume_upload"] = times_ms(lambda: t.volume_upload(d, m), max(2, args.reps // 3), 1)
    t.shutdown()
    line = json.dumps(rec)
    print(line, flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
