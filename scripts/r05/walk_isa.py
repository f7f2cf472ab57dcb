"""What the compiler made of the walk and the search, without a GPU.  Compiles trace_kernels.hip with the build's flags (blok_amd/build.py) to
gfx950 assembly and prints
  * per kernel: VGPRs, SGPRs, spilled SGPRs / VGPRs and scratch bytes (the code object's metadata);
  * trace_kernel<Rect>'s walk loop (walk_loop in trace_core.h) by block: the trip's top (child bit, occupancy), the step (with the rare ascent),
    the descent (push, rank, fetch, the three enter_axis) and the far planes' evaluation; per block the full-rate and half-rate VALU counts
    (~2.2 and ~4.2 cycles per wave64 instruction; v_cndmask in its VCC form ~20), the v_cndmask among them, and how many
    plane evaluations (v_fma_f32) it holds;
  * the search's loops in beam_kernel<Rect>: v_writelane / v_readlane and scratch instructions.
usage: walk_isa.py [--src DIR] [--asm FILE]   (DIR: a tree's blok_amd/csrc/hip, default this tree's; --asm: read FILE instead of compiling)"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

KERNELS = {
    "trace_kernel<Rect>": "12trace_kernelILNS_7RayModeE0EEEvNS_9TraceArgsE",
    "joint_kernel<Rect>": "12joint_kernelILNS_7RayModeE0EEEvNS_9TraceArgsEj",
    "beam_kernel<Rect>": "11beam_kernelILNS_7RayModeE0EEEvNS_9TraceArgsEj",
    "path_kernel<false>": "11path_kernelILb0EEEvNS_8PathArgsE",
}
FULL = {"v_fma_f32", "v_mul_f32", "v_sub_f32", "v_subrev_f32", "v_add_f32", "v_mov_b32", "v_add_u32", "v_sub_u32", "v_subrev_u32",
        "v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_mac_f32", "v_fmac_f32"}


def compile_asm(src: Path) -> str:
    from blok_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "trace_kernels.s"
        cmd = [b.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++20", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC",
               f"-I{ROOT / 'include'}", f"-I{src}", "--cuda-device-only", "-S", str(src / "trace_kernels.hip"), "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True)
        return out.read_text()


def resources(asm: str, mangled: str) -> dict:
    i = asm.index(".name:           _ZN4blok12_GLOBAL__N_1" + mangled)
    block = asm[asm.rindex("  - .", 0, i):]
    block = block[:block.index("\n  - .", 10) if "\n  - ." in block[10:] else len(block)]
    get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
    return {k: get(k) for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}


def body(asm: str, mangled: str) -> list[str]:
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN4blok12_GLOBAL__N_1" + mangled + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def is_insn(l: str) -> bool:
    return l.startswith("\t") and not l.strip().startswith((".", ";"))


def op(l: str) -> str:
    return re.sub(r"_e(32|64)$", "", l.split()[0])


def blocks_of(lines: list[str]):
    """[(label, [instructions])] in layout order; fall-through blocks (the compiler's "; %bb.N" comments) count as blocks of their own."""
    out, cur = [], ("entry", [])
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; (%bb\.\d+):", l.strip())
        if m:
            out.append(cur)
            cur = (m.group(1), [])
        elif is_insn(l):
            cur[1].append(l.strip())
    out.append(cur)
    return out


def walk_loop(lines: list[str]):
    """The walk loop's blocks: the loop whose body holds the node fetch (global_load_dwordx3), the stack push (ds_write_b128) and the
    ascent's stack read (ds_read_b96), the innermost such loop."""
    blocks = blocks_of(lines)
    index = {lab: k for k, (lab, _) in enumerate(blocks)}
    loops = []
    for k, (_, ins) in enumerate(blocks):
        for l in ins:
            m = re.match(r"s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
            if m and m.group(1) in index and index[m.group(1)] <= k:
                loops.append((index[m.group(1)], k))
    best = None
    for a, b in loops:
        text = "\n".join(l for _, ins in blocks[a:b + 1] for l in ins)
        if "global_load_dwordx3" in text and "ds_write_b128" in text and "ds_read_b96" in text:
            if best is None or b - a < best[1] - best[0]:
                best = (a, b)
    a = best[0]
    b = max(e for h, e in loops if h == a)          # every back edge to that header: the trip's last block may branch back on its own
    return blocks[a:b + 1]


def classify(ins: list[str]) -> dict:
    c = {"full": 0, "half": 0, "cndmask": 0, "cndmask_vcc": 0, "plane_fma": 0, "salu": 0}
    for l in ins:
        o = op(l)
        if o.startswith("v_") and not o.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            if o in FULL:
                c["full"] += 1
            else:
                c["half"] += 1
            if o == "v_cndmask_b32":
                c["cndmask"] += 1
                if l.split()[0].endswith("_e32"):
                    c["cndmask_vcc"] += 1
            if o == "v_fma_f32":
                c["plane_fma"] += 1
        elif o.startswith("s_"):
            c["salu"] += 1
    return c


def role(ins: list[str]) -> str:
    text = "\n".join(ins)
    ops = [op(l) for l in ins]
    if "global_load_dwordx3" in text or "ds_write_b128" in text:
        return "descend"
    if "ds_read_b96" in text:
        return "ascent"
    if "v_bfe_u32" in ops and "v_bitop3_b32" in ops or ops.count("v_bfe_u32") >= 3:
        return "top"
    if "v_ffbl_b32" in ops or "v_min3_f32" in ops:
        return "step"
    if ops.count("v_fma_f32") == 3 and ops.count("v_mul_f32") >= 3 and "v_cndmask_b32" not in ops:
        return "far planes"
    return "control"


def report(asm: str) -> None:
    print("kernel                 VGPR  SGPR  SGPR spill  VGPR spill  scratch B")
    for name, mangled in KERNELS.items():
        r = resources(asm, mangled)
        print(f"{name:22s} {r['vgpr_count']:4d}  {r['sgpr_count']:4d}  {r['sgpr_spill_count']:10d}  {r['vgpr_spill_count']:10d}  {r['private_segment_fixed_size']:9d}")
    print()
    print("trace_kernel<Rect> walk loop, by block (full / half-rate VALU; cndmask; plane fma; SALU):")
    totals: dict[str, dict] = {}
    for lab, ins in walk_loop(body(asm, KERNELS["trace_kernel<Rect>"])):
        c = classify(ins)
        r = role(ins)
        print(f"  {lab:14s} {r:11s} full {c['full']:3d}  half {c['half']:3d}  cndmask {c['cndmask']:2d} (vcc {c['cndmask_vcc']})  plane fma {c['plane_fma']:2d}  salu {c['salu']:3d}")
        t = totals.setdefault(r, dict.fromkeys(c, 0))
        for k in c:
            t[k] += c[k]
    print("  by role (cycles ~ 2.2 full + 4.2 half):")
    for r, c in totals.items():
        print(f"    {r:11s} full {c['full']:3d}  half {c['half']:3d}  cndmask {c['cndmask']:2d}  plane fma {c['plane_fma']:2d}  ~{2.2 * c['full'] + 4.2 * c['half']:6.1f} cycles")
    print()
    lines = body(asm, KERNELS["beam_kernel<Rect>"])
    n = lambda pat: sum(1 for l in lines if is_insn(l) and re.search(pat, l))
    print(f"beam_kernel<Rect>: v_writelane {n('v_writelane')}, v_readlane {n('v_readlane')}, scratch instructions {n('scratch_')}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=Path, default=ROOT / "blok_amd" / "csrc" / "hip")
    ap.add_argument("--asm", type=Path)
    a = ap.parse_args()
    report(a.asm.read_text() if a.asm else compile_asm(a.src.resolve()))


if __name__ == "__main__":
    main()
