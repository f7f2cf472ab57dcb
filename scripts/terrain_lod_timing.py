"""Cost of blok_hip_terrain_reduce beside the route it replaces, on §13's terrain with caves (seed 7): one neighbour box of
--size^3 (default 1024) and the ring of eight around the box at the origin, for --levels K.  Median of --reps after --warmup.  Device times
are a pair of events on the null stream around the blocking calls, host times the clock around them.  One step per invocation, so that each
runs under a time limit of its own:

    composed   the route as it stood before: volume_create at the box, volume_generate_terrain, volume_reduce(VOTE_EXPOSED) — all three by
               the host clock and by events, and generate + reduce alone by events (the create is the allocation of the volume)
    direct     terrain_reduce with VOTE_EXPOSED and with VOTE_EXPOSED | SEAMLESS, by events and by the host clock; and the same call with
               one level, which is the level-1 kernel, the counters' memset and their way back
    trace      each kernel's work a few times and nothing else: the run to put under a kernel trace with statistics, which is where
               terrain_lod_kernel's, terrain_kernel's and lod_level1_kernel's own times come from

    python scripts/terrain_lod_timing.py --step direct --levels 2 [--size 1024] [--reps 20] [--warmup 2] [--out profiles/terrain_lod_timing.txt]

Every invocation but `trace` appends one JSON line to --out.
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

from blok_amd import _ffi                      # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("composed", "direct", "trace")
SEED = 7
VOTE_EXPOSED, SEAMLESS = _ffi.LOD_VOTE_EXPOSED, _ffi.LOD_SEAMLESS


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": len(ms)}


def timed(fn, reps, warmup):
    """(host clock, device events) of fn, which blocks."""
    import torch
    host, device = [], []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            host.append((time.perf_counter() - t0) * 1e3)
            device.append(e0.elapsed_time(e1))
    return {"host": summary(host), "device": summary(device)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "terrain_lod_timing.txt"))
    args = ap.parse_args()
    n, K = args.size, args.levels
    rec = {"step": args.step, "box": n, "levels": K, "seed": SEED}
    t = HipTracer(64, 64).init()
    p = T.default_params(n, SEED)
    ring = [(dx * n, 0, dz * n) for dz in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dz]
    one = [(n, 0, 0)]

    def end(o):
        return (o[0] + n, n, o[2] + n)

    def composed(boxes, create=True):
        for o in boxes:
            if create:
                t.volume_create(o, (n, n, n))
            t.volume_generate_terrain(p)
            t.volume_reduce(None, None, K, VOTE_EXPOSED)

    def direct(boxes, levels, flags):
        for o in boxes:
            t.terrain_reduce(p, o, end(o), levels, flags)

    if args.step == "trace":
        t.volume_create(one[0], (n, n, n))
        for _ in range(args.reps):
            composed(one, create=False)
            direct(one, K, VOTE_EXPOSED)
            direct(one, K, VOTE_EXPOSED | SEAMLESS)
        t.shutdown()
        return 0
    if args.step == "composed":
        rec["one_box_create_generate_reduce"] = timed(lambda: composed(one), args.reps, args.warmup)
        rec["ring_of_eight_create_generate_reduce"] = timed(lambda: composed(ring), args.reps, 1)
        t.volume_create(one[0], (n, n, n))
        rec["one_box_generate_reduce_in_a_standing_volume"] = timed(lambda: composed(one, create=False), args.reps, args.warmup)
        rec["one_box_generate_alone"] = timed(lambda: t.volume_generate_terrain(p), args.reps, args.warmup)
        rec["one_box_reduce_alone"] = timed(lambda: t.volume_reduce(None, None, K, VOTE_EXPOSED), args.reps, args.warmup)
        rec["sum_n"] = int(t.volume_lod_info()["level"][0][0]["sum_n"])
    else:
        for name, flags in (("vote_exposed", VOTE_EXPOSED), ("vote_exposed_seamless", VOTE_EXPOSED | SEAMLESS)):
            rec[f"one_box_{name}"] = timed(lambda: direct(one, K, flags), args.reps, args.warmup)
            rec[f"ring_of_eight_{name}"] = timed(lambda: direct(ring, K, flags), args.reps, args.warmup)
            rec[f"one_box_one_level_{name}"] = timed(lambda: direct(one, 1, flags), args.reps, args.warmup)
        direct(one, K, VOTE_EXPOSED)
        rec["sum_n"] = int(t.volume_lod_info()["level"][0][0]["sum_n"])
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
