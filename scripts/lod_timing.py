"""Cost of blok_hip_volume_reduce and blok_hip_volume_lod_model on a keyed volume with §13's terrain with caves (seed 7): host
clock around each blocking call, median of --reps after --warmup, with the spread.  One step per invocation, so that each runs under a time
limit of its own:

    reduce     the whole box at K = 1 and K = 5, each without and with BLOK_LOD_VOTE_EXPOSED; a 64^3 region in the middle at K = 5;
               lod_model of level 2 (min_count 1), the model destroyed again; and, as the yardstick of the level-1 pass — which reads at most
               the id array (4 bytes a cell) plus the brick masks (1/8 byte a cell) and writes 8 bytes per 8 cells — a device-to-device copy
               of as many bytes as the id array holds, with the ratio
    host       at --host-size^3 (default 256): the device's reduce at K = 5 against blok_hip_volume_download + the host build
               (blok_lod_reduce), what a caller had to do before

    python scripts/lod_timing.py --step reduce [--size 1024] [--reps 7] [--warmup 2] [--out profiles/lod_timing.txt]

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

from blok_amd import lod as L                  # noqa: E402
from blok_amd import terrain as T              # noqa: E402
from blok_amd.tracer import HipTracer          # noqa: E402

STEPS = ("reduce", "host")
SEED = 7


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
    ap.add_argument("--host-size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lod_timing.txt"))
    args = ap.parse_args()
    n = args.size if args.step == "reduce" else args.host_size
    rec = {"step": args.step, "volume": n}
    t = HipTracer(64, 64).init()
    t.volume_create((0, 0, 0), (n, n, n))
    p = T.default_params(n, SEED)
    rec["terrain_voxels"] = t.volume_generate_terrain(p)
    rec["keyed"] = t.volume_refresh_counts()[2] == 0
    if args.step == "reduce":
        import torch
        for levels in (1, 5):
            for flags, name in ((0, "n_vote"), (L.VOTE_EXPOSED, "exposed_vote")):
                info = t.volume_reduce(None, None, levels, flags)
                rec[f"whole_K{levels}_{name}"] = times_ms(lambda: t.volume_reduce(None, None, levels, flags), args.reps, args.warmup)
        top = info["level"][0][4]
        rec["level5"] = {k: int(top[k]) for k in ("n_cells", "n_filled", "n_exposed", "sum_n", "sum_e")}
        mid = n // 2 - 32
        rec["region_64_K5"] = times_ms(lambda: t.volume_reduce((mid, mid, mid), (mid + 64, mid + 64, mid + 64), 5, L.VOTE_EXPOSED), args.reps, args.warmup)
        t.volume_reduce(None, None, 2, L.VOTE_EXPOSED)

        def model():
            t.model_destroy(t.volume_lod_model(2, 1))
        rec["lod_model_K2"] = times_ms(model, args.reps, args.warmup)
        rec["lod_model_K2_voxels"] = t.last_capture_voxels
        src = torch.empty(4 * n ** 3, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()
        rec["d2d_copy_of_the_id_bytes"] = times_ms(copy, args.reps, args.warmup)
        rec["id_bytes"] = 4 * n ** 3
        for name in ("n_vote", "exposed_vote"):
            rec[f"K1_{name}_over_copy"] = round(rec[f"whole_K1_{name}"]["ms_median"] / rec["d2d_copy_of_the_id_bytes"]["ms_median"], 2)
    else:
        info = t.volume_reduce(None, None, 5, L.VOTE_EXPOSED)
        rec["device_reduce_K5"] = times_ms(lambda: t.volume_reduce(None, None, 5, L.VOTE_EXPOSED), args.reps, args.warmup)

        def host():
            d, m = t.volume_download()
            return L.reduce_host(d, m, (0, 0, 0), None, None, 5, L.VOTE_EXPOSED)
        levels, host_info = host()
        rec["host_equals_device"] = bool(host_info.tobytes() == info.tobytes() and all(
            levels[j - 1][plane].tobytes() == t.volume_lod_download(j, plane).tobytes() for j in range(1, 6) for plane in range(3)))
        rec["download_plus_host_build"] = times_ms(host, max(args.reps // 2, 3), 1)
        rec["host_over_device"] = round(rec["download_plus_host_build"]["ms_median"] / rec["device_reduce_K5"]["ms_median"], 1)
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
