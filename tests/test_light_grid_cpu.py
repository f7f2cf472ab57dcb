"""CPU: the light grid (include/blok_hip.h, "the light grid"; include/blok_world.h: blok_light_grid_build).  The host build against the
numpy model of tests/light_grid_reference.py — for every cell, the loop over all lights with the predicate — in all three arrays, over
tests/light_grid_cases.py; the limits; the partition identity the sampling rule of DESIGN.md §34 rests on, in exact rationals; and the
stand-alone program of tests/host_harness/light_grid_main.cpp under ASan + UBSan."""
from __future__ import annotations

import os
import re
import struct
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import lights as LT
from blok_amd._ffi import LIGHT_GRID_INFO, LIGHT_GRID_ITEM, BlokError
from tests import light_grid_cases as GC
from tests import light_grid_reference as GR

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
CASES = GC.table()


def test_abi_symbols_sizes_and_version():
    header = (ROOT / "include" / "blok_hip.h").read_text()
    for name in ("blok_hip_build_light_grid", "blok_hip_light_grid_info", "blok_hip_light_grid_download", "blok_hip_light_grid_clear"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _ffi.HIP_SYMBOLS
        assert hasattr(_ffi.hip_lib(), name)
    assert "blok_light_grid_build" in _ffi.HOST_SYMBOLS and hasattr(_ffi.host_lib(), "blok_light_grid_build")
    assert LIGHT_GRID_ITEM.itemsize == 8 and LIGHT_GRID_INFO.itemsize == 72
    assert _ffi.hip_lib().blok_hip_abi_version() >= (1 << 16) | 29
    for fn in ("build_grid", "grid_info", "grid_download", "clear_grid", "host_build_grid"):
        assert callable(getattr(LT, fn))
    mirror = (ROOT / "include" / "blok" / "hip_tracer.hpp").read_text()
    assert "blok_hip_build_light_grid" in mirror and "blok_hip_light_grid_clear" in mirror


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_build_equals_the_numpy_model(case):
    assert int(LT.check(case.lights)["n"][0]) == len(case.lights)
    for c, reach in case.params:
        cell_lo, dim, want_start, want_faces, want_items = GR.build(case.lights, c, reach)
        start, faces, items, info = LT.host_build_grid(case.lights, c, reach, 192)
        lens = np.diff(want_start.astype(np.int64))
        print(f"{case.name}: c {c} R {reach}: {len(case.lights)} lights -> dim {dim.tolist()} at {cell_lo.tolist()}, {len(want_items)} items, longest {int(lens.max())}")
        assert info["cell_lo"][0].tolist() == cell_lo.tolist() and info["dim"][0].tolist() == dim.tolist()
        assert start.tobytes() == want_start.tobytes()
        assert faces.tobytes() == want_faces.tobytes()
        assert items.tobytes() == want_items.tobytes()
        assert (int(info["n_cells"][0]), int(info["n_items"][0]), int(info["n_nonempty"][0]), int(info["max_items"][0])) == \
               (len(want_faces), len(want_items), int((lens > 0).sum()), int(lens.max()))
        assert (int(info["cell_log2"][0]), int(info["reach"][0]), int(info["share"][0]), int(info["reserved"][0])) == (c, reach, 192, 0)
        assert int(info["bytes"][0]) == 4 * (len(start) + len(faces)) + 8 * len(items)
        # every light is listed by its own cells at least, lists ascend, faces never pass A
        assert set(items["light"].tolist()) == set(range(len(case.lights)))
        for g in np.nonzero(lens > 1)[0][:64]:
            seg = items["light"][start[g]:start[g + 1]].astype(np.int64)
            assert np.all(np.diff(seg) > 0)
        assert int(faces.max()) <= int((case.lights["du"].astype(np.int64) * case.lights["dv"]).sum())


def test_what_the_cases_are_built_to_hit():
    """The cases' own claims: where the voxel rule matters, how many cells a rectangle spans, how long the crowded lists are."""
    by_name = {c.name: c for c in CASES}
    for a in range(3):
        t = by_name[f"emitting voxels beside a cell boundary, axis {a}"].lights
        cmin, cmax = GR.cell_ranges(t, 3)
        # plane 64: the + face (first) emits from voxel 63, cell 7; the - face from voxel 64, cell 8.  plane 65: both in cell 8; 63: both in 7
        assert cmin[:6, a].tolist() == [7, 8, 8, 8, 7, 7] and cmin[6:, a].tolist() == [-1, 0, -9, -8]
    t = by_name["rectangles over 2 and 3 cells"].lights
    cmin, cmax = GR.cell_ranges(t, 3)
    spans = sorted(set(map(tuple, (cmax - cmin + 1).tolist())))
    assert any(2 in s for s in spans) and any(3 in s for s in spans)
    for n in (63, 64, 65, 300):
        start, faces, items, info = LT.host_build_grid(by_name[f"{n} lights in one cell"].lights, 6, 0)
        assert int(info["n_cells"][0]) == 1 and int(info["max_items"][0]) == n
    start, faces, items, info = LT.host_build_grid(by_name["two distant clusters"].lights, 3, 0)
    assert int(info["n_nonempty"][0]) < int(info["n_cells"][0]), "empty cells between the clusters"
    start, faces, items, info = LT.host_build_grid(by_name["a 65 536-long rectangle"].lights, 12, 0)
    assert int(info["dim"][0][0]) == 16


@pytest.mark.parametrize("name,lights,c,reach,passes", GC.limit_cases(), ids=[l[0] for l in GC.limit_cases()])
def test_limits(name, lights, c, reach, passes):
    if passes:
        start, faces, items, info = LT.host_build_grid(lights, c, reach)
        assert int(info["n_cells"][0]) == 2 ** 24 and len(items) == 2 and int(faces.sum()) == 2 and int(info["n_nonempty"][0]) == 2
        assert int(start[-1]) == 2
    else:
        with pytest.raises(BlokError) as e:
            LT.host_build_grid(lights, c, reach)
        assert e.value.status == BLOK_ERR_UNSUPPORTED


def test_parameters_out_of_range_are_refused():
    t = CASES[0].lights
    for c, reach, share in ((1, 0, 128), (13, 0, 128), (4, 4, 128), (4, 1, 0), (4, 1, 256)):
        with pytest.raises(BlokError) as e:
            LT.host_build_grid(t, c, reach, share)
        assert e.value.status == BLOK_ERR_INVALID_ARG
    with pytest.raises(BlokError) as e:
        LT.host_build_grid(t[:0], 4, 1, 128)
    assert e.value.status == BLOK_ERR_INVALID_ARG


@pytest.mark.parametrize("case", [c for c in CASES if len(c.lights) <= 65], ids=[c.name for c in CASES if len(c.lights) <= 65])
def test_partition_identity_in_exact_rationals(case):
    """The list of a cell is exactly {L : in(L, g)} and faces[g] its face sum, so the densities of DESIGN.md §34 sum to 1 over the table's
    faces: for shading cells inside the grid, on its rim and outside it, with the list and A_g taken from the HOST build's arrays."""
    c, reach = case.params[min(1, len(case.params) - 1)]
    share = 192
    start, faces, items, info = LT.host_build_grid(case.lights, c, reach, share)
    cell_lo, dim = info["cell_lo"][0].astype(np.int64), info["dim"][0].astype(np.int64)
    cmin, cmax = GR.cell_ranges(case.lights, c)
    area = [int(d) * int(e) for d, e in zip(case.lights["du"], case.lights["dv"])]
    a_all = sum(area)
    inside = cell_lo + dim // 2
    rim = [cell_lo, cell_lo + dim - 1, cell_lo + (dim[0] - 1, 0, 0)]
    outside = [cell_lo - 1, cell_lo + dim, cell_lo + (dim[0], 0, 0)]
    own = [cmin[0], cmax[-1]]                                   # cells that hold a light: A_g > 0 for certain
    n_lit = 0
    for g in [inside, *rim, *outside, *own]:
        rel = np.asarray(g) - cell_lo
        if np.all((rel >= 0) & (rel < dim)):
            i = int((rel[2] * dim[1] + rel[1]) * dim[0] + rel[0])
            members, a_g = items["light"][start[i]:start[i + 1]].tolist(), int(faces[i])
        else:
            members, a_g = [], 0
        assert members == np.nonzero(GR.listed(cmin, cmax, reach, g))[0].tolist()
        assert a_g == sum(area[m] for m in members)
        w_glob = (Fraction(256 - share, 256) if a_g else Fraction(1)) / a_all
        total = sum(area[m] * (Fraction(share, 256) / a_g) for m in members) + a_all * w_glob
        assert total == 1 and total == GR.density_sum(case.lights, c, reach, share, g)
        n_lit += 1 if a_g else 0
    assert n_lit >= 2


def test_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "light_grid_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(SRC / "light_grid_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/light_grid.cpp")], check=True)
    files = []
    for case in CASES:
        c, reach = case.params[-1]
        _, _, start, faces, items = GR.build(case.lights, c, reach)
        files.append(tmp_path / f"case_{len(files)}.bin")
        files[-1].write_bytes(struct.pack("<QQQII", len(case.lights), len(faces), len(items), c, reach) + case.lights.tobytes() + start.tobytes() + faces.tobytes()
                              + items.tobytes())
    run = subprocess.run([os.fspath(exe), *map(os.fspath, files)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "light_grid_main: ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count(" items\n") == len(files)
