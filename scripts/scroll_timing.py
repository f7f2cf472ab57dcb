"""Cost of the scroll of the resident volume on a keyed volume with §13's terrain with caves: host clock around each blocking
call, median of --reps after --warmup, with the spread.  One step per invocation, so that each runs under a time limit of its own:

    scroll     blok_hip_volume_scroll by (64, 0, 0), (0, 64, 0), (0, 0, 64), (64, 64, 64) and (0, 0, 0), and PLAN_ONLY
    baseline   the only way without it: blok_hip_volume_download + blok_hip_volume_create + blok_hip_volume_upload of the same box
    copy       a device-to-device hipMemcpy of two arrays the size of the dense ones: the rate a copy of these bytes reaches
    series     40 scrolls by (64, 0, 0) and back, alternating, each call's time kept: the median hides that the runtime gives freed device
               memory back in batches, so the series shows the stalls and the mean shows what a call costs once they are spread over all
    kernel     three scrolls by (64, 0, 0) and nothing else timed: for a run under a kernel trace, which takes the move kernel alone

    python scripts/scroll_timing.py --step scroll [--size 1024] [--reps 10] [--warmup 2] [--out profiles/scroll_timing.txt]

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

STEPS = ("scroll", "baseline", "copy", "series", "kernel")
DELTAS = ((64, 0, 0), (0, 64, 0), (0, 0, 64), (64, 64, 64), (0, 0, 0))


def times_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scroll_timing.txt"))
    args = ap.parse_args()
    n = args.size
    dense_bytes = 8 * n ** 3                       # the two dense arrays: read once and written once by a scroll
    rec = {"step": args.step, "volume": n, "dense_bytes": dense_bytes}
    if args.step == "copy":
        import torch
        words = dense_bytes // 8
        src = [torch.zeros(words, dtype=torch.int32, device="cuda") for _ in range(2)]
        dst = [torch.empty(words, dtype=torch.int32, device="cuda") for _ in range(2)]

        def copy():
            for s, d in zip(src, dst):
                d.copy_(s)
            torch.cuda.synchronize()
        rec["copy"] = times_ms(copy, args.reps, args.warmup)
        rec["copy_gb_per_s_read_plus_write"] = round(2 * dense_bytes / rec["copy"]["ms_median"] / 1e6, 1)
    else:
        t = HipTracer(64, 64).init()
        t.volume_create((0, 0, 0), (n, n, n))
        p = T.default_params(n, 0xB10C0001)
        rec["terrain_voxels"] = t.volume_generate_terrain(p)
        rec["keyed"] = t.volume_refresh_counts()[2] == 0
        if args.step == "scroll":
            rec["scrolls"] = []
            for delta in DELTAS:
                # (the box keeps moving the same way: what a scroll costs does not depend on what the cells hold)
                info = t.volume_scroll(delta, plan_only=True)
                entry = {"delta": list(delta), "n_cells_kept": int(info["n_cells_kept"][0]), "n_exposed": int(info["n_exposed"][0]),
                         "plan_only": times_ms(lambda: t.volume_scroll(delta, plan_only=True), args.reps, args.warmup),
                         "scroll": times_ms(lambda: t.volume_scroll(delta), args.reps, args.warmup)}
                entry["gb_per_s_read_plus_write"] = round(2 * dense_bytes / entry["scroll"]["ms_median"] / 1e6, 1) if any(delta) else None
                rec["scrolls"].append(entry)
                t.volume_generate_terrain(p)       # filled again for the next delta
        elif args.step == "baseline":
            def round_trip():
                d, m = t.volume_download()
                t.volume_create((64, 0, 0), (n, n, n))
                t.volume_upload(d, m)
            rec["download_create_upload"] = times_ms(round_trip, args.reps, args.warmup)
        elif args.step == "series":
            ms = []
            for i in range(40):
                t0 = time.perf_counter()
                t.volume_scroll((64, 0, 0) if i % 2 == 0 else (-64, 0, 0))
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            rec["series_ms"] = ms
            rec["ms_median"], rec["ms_mean"], rec["ms_max"] = round(float(np.median(ms)), 3), round(float(np.mean(ms)), 3), round(float(np.max(ms)), 3)
            rec["calls_above_100_ms"] = [i for i, v in enumerate(ms) if v > 100.0]
        else:
            for _ in range(3):
                t.volume_scroll((64, 0, 0))
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
