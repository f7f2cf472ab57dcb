"""Cost of blok_hip_volume_automaton on a keyed volume with §13's terrain with caves (seed 7): host clock around each
blocking call, median of --reps after --warmup, with the spread.  A call changes the volume, so the terrain is generated again before
every timed call, outside the clock.  One step per invocation, so that each runs under a time limit of its own:

    calls      one step of smooth, despeckle and dilate(26) over the whole box and over a 64^3 region in the middle; the same volume through
               distance_field(R = 2) + edit_by_distance(GROW, d2 = 3), the pair that dilated by the 26-neighbourhood before, with the ratio;
               and a rule that changes nothing, whose call is the decide launch and the counters' way back: no births, no deaths, no commit
    host       at --host-size^3 (default 256): the device's smooth step against blok_hip_volume_download + the host build
               (blok_automaton_voxels), what a caller had to do before
    trace      the work of `calls` over the whole box, --reps times each, and nothing else: the run to put under a kernel trace with
               statistics, which is where the decide, births and deaths kernels' and the commit's kernels' times come from

    python scripts/automaton_timing.py --step calls [--size 1024] [--reps 7] [--warmup 2] [--out profiles/automaton_timing.txt]

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
from blok_amd import automaton as A            # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("calls", "host", "trace")
SEED = 7


def summary(ms, reps):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3), "reps": reps}


def times_ms(fn, reps, warmup, before=None):
    ms = []
    for i in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return summary(ms, reps)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--host-size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "automaton_timing.txt"))
    args = ap.parse_args()
    n = args.host_size if args.step == "host" else args.size
    rec = {"step": args.step, "volume": n}
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))
    p = T.default_params(n, SEED)

    def terrain():
        return t.volume_generate_terrain(p)
    rec["terrain_voxels"] = terrain()
    rec["keyed"] = t.volume_refresh_counts()[2] == 0
    rules = {"smooth": A.smooth(1), "despeckle": A.despeckle(), "dilate26": A.dilate(26, fixed_material=True)}
    mid = n // 2 - 32
    region = ((mid, mid, mid), (mid + 64, mid + 64, mid + 64))
    if args.step == "trace":
        for r in rules.values():
            for _ in range(args.reps):
                terrain()
                t.volume_automaton(r)
        t.shutdown()
        return 0
    if args.step == "calls":
        for name, r in rules.items():
            terrain()
            info, _ = t.volume_automaton(r)
            rec[f"{name}_whole_counts"] = {k: int(info[k][0]) for k in ("steps_run", "n_born", "n_died", "n_filled")}
            rec[f"{name}_whole"] = times_ms(lambda: t.volume_automaton(r), args.reps, args.warmup, terrain)
            rec[f"{name}_region_64"] = times_ms(lambda: t.volume_automaton(r, *region), args.reps, args.warmup, terrain)
        # a step that changes nothing runs the decide kernel alone and no commit: its call time is the decide launch and the counters' way back
        rec["nothing_happens_whole"] = times_ms(lambda: t.volume_automaton(A.rule(26, A.at_least(0, 26), 0)), args.reps, args.warmup)

        def pair():
            t.volume_distance_field(None, None, 2)
            return t.volume_edit_by_distance(_ffi.DISTANCE_GROW, 3, 1.0, 0)
        terrain()
        rec["distance_pair_written"] = pair()
        rec["distance_field_R2_plus_grow_d2_3_whole"] = times_ms(pair, args.reps, args.warmup, terrain)
        rec["dilate26_written"] = rec["dilate26_whole_counts"]["n_born"]
        rec["pair_over_dilate26"] = round(rec["distance_field_R2_plus_grow_d2_3_whole"]["ms_median"] / rec["dilate26_whole"]["ms_median"], 2)
        rec["decide_share_of_a_smooth_call"] = round(rec["nothing_happens_whole"]["ms_median"] / rec["smooth_whole"]["ms_median"], 3)
    else:
        r = rules["smooth"]
        rec["device_smooth_step"] = times_ms(lambda: t.volume_automaton(r), args.reps, args.warmup, terrain)
        terrain()

        def host():
            d, m = t.volume_download()
            return A.automaton_host(d, m, r)
        hd, hm, host_info, _ = host()
        info, _ = t.volume_automaton(r)
        gd, gm = t.volume_download()
        rec["host_equals_device"] = bool(host_info.tobytes() == info.tobytes() and hd.tobytes() == gd.tobytes() and hm.tobytes() == gm.tobytes())
        rec["download_plus_host_build"] = times_ms(host, max(args.reps // 2, 3), 1, terrain)
        rec["host_over_device"] = round(rec["download_plus_host_build"]["ms_median"] / rec["device_smooth_step"]["ms_median"], 1)
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
