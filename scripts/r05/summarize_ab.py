"""Condenses an interleaved A/B visit (two kernel libraries, "base" and "new") into profiles/r05_*: the bench lines (default and --full),
rocprofv3 kernel statistics per library and the VALU counters per launch of the frame's kernels.
usage: summarize_ab.py <dir with bench_*_N.json, full_*_N.json, trace_*/, pmc_*/> [tag of the profiles/ files, default r05]"""
import csv
import json
import statistics
import sys
from collections import defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
src = Path(sys.argv[1])
dst = ROOT / "profiles"
TAG = sys.argv[2] if len(sys.argv) > 2 else "r05"
KERNELS = ("joint_kernel<(blok::RayMode)0>", "trace_kernel<(blok::RayMode)0>", "beam_kernel<(blok::RayMode)0>")


def lines(prefix):
    out = defaultdict(list)
    for p in sorted(src.glob(f"{prefix}_*_*.json")):
        _, v, rep = p.stem.split("_")
        out[v].append((int(rep), json.loads(p.read_text())))
    return {v: [d for _, d in sorted(r)] for v, r in out.items()}


report = []
bench = lines("bench")
report.append("python bench.py --gpus 1 (200 steps, three frames in flight), interleaved base/new per repetition: value (Mrays/s), ms_per_step")
for v in ("base", "new"):
    vals = [d["value"] for d in bench.get(v, [])]
    ms = [d["ms_per_step"] for d in bench.get(v, [])]
    if vals:
        report.append(f"  {v:4s} " + "  ".join(f"{x:8.0f}" for x in vals) + f"   median {statistics.median(vals):8.0f}   ms " + " ".join(f"{x:.4f}" for x in ms))
if bench.get("base") and bench.get("new"):
    gain = statistics.median(d["value"] for d in bench["new"]) / statistics.median(d["value"] for d in bench["base"]) - 1
    report.append(f"  median gain {100 * gain:+.1f} %")
full = lines("full")
if full:
    report.append("")
    report.append("python bench.py --gpus 1 --full --no-cpu-baseline, interleaved: value, kernel_ms_alone, poses A/B/C ms_per_frame_alone, configs[4] paths ms_per_frame")
    for v in ("base", "new"):
        for d in full.get(v, []):
            c = d["config"]
            poses = " ".join(f"{k} {p['ms_per_frame_alone']:.4f}" for k, p in c.get("poses", {}).items())
            paths = c.get("also_measured_paths", {}).get("ms_per_frame", float("nan"))
            report.append(f"  {v:4s} value {d['value']:8.0f}  alone {c['kernel_ms_alone']:.4f} ms  {poses}  paths {paths:.2f} ms")
for v in ("base", "new"):
    stats = list((src / f"trace_{v}").glob("**/*kernel_stats.csv"))
    if stats:
        (dst / f"{TAG}_kernel_stats_{v}.csv").write_text(stats[0].read_text())
pmc = {}
for v in ("base", "new"):
    files = list((src / f"pmc_{v}").glob("**/*counter_collection.csv"))
    if not files:
        continue
    per = defaultdict(lambda: defaultdict(float))          # (kernel, dispatch) -> counter -> value
    for row in csv.DictReader(files[0].open()):
        k = next((k for k in KERNELS if k in row["Kernel_Name"]), None)
        if k:
            per[(k, row.get("Dispatch_Id") or row.get("Correlation_Id"))][row["Counter_Name"]] += float(row["Counter_Value"])
    out = {}
    for k in KERNELS:
        ds = [c for (kk, _), c in per.items() if kk == k]
        if ds:
            out[k] = {"launches": len(ds), **{name: statistics.mean(c[name] for c in ds if name in c) for name in sorted({n for c in ds for n in c})}}
            a = out[k]
            if a.get("SQ_ACTIVE_INST_VALU"):
                a["lane_utilisation"] = a["SQ_THREAD_CYCLES_VALU"] / (64 * a["SQ_ACTIVE_INST_VALU"])
    pmc[v] = out
if pmc:
    (dst / f"{TAG}_pmc.json").write_text(json.dumps(pmc, indent=1) + "\n")
    report.append("")
    report.append("rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU (default bench, 60 steps), mean per launch:")
    for k in KERNELS:
        row = [f"  {k:34s}"]
        for v in ("base", "new"):
            a = pmc.get(v, {}).get(k)
            if a:
                row.append(f"{v} {a['SQ_INSTS_VALU'] / 1e6:7.2f} M VALU ({a['launches']} launches, lanes {a.get('lane_utilisation', float('nan')):.3f})")
        b, n = pmc.get("base", {}).get(k), pmc.get("new", {}).get(k)
        if b and n:
            row.append(f"change {100 * (n['SQ_INSTS_VALU'] / b['SQ_INSTS_VALU'] - 1):+.1f} %")
        report.append("  ".join(row))
print("\n".join(report))
