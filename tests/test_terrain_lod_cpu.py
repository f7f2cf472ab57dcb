"""CPU: the host build of terrain_reduce (blok_terrain_reduce, blok_amd.lod.terrain_reduce_host) against the composition that defines it —
terrain.eval_box, then lod.reduce_host (tests/terrain_lod_cases.py) — planes and infos byte for byte over the case table, for 1, 3 and 5
levels and all four flag combinations; the partition promise of SEAMLESS; the error table; and the tile arithmetic of
csrc/common/terrain_lod_core.h beside a per-voxel loop in a program of its own under the sanitizers."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import lod as HL
from blok_amd._ffi import BlokError
from tests import terrain_cases as TC
from tests import terrain_lod_cases as TLC

ROOT = Path(__file__).resolve().parent.parent
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5


def test_abi_is_at_least_1_20():
    assert _ffi.hip_lib().blok_hip_abi_version() >= (1 << 16) | 20
    assert HL.SEAMLESS == 2 and not HL.SEAMLESS & HL.VOTE_EXPOSED


def test_the_reference_tells_the_flags_apart():
    TLC.check_reference_tells_the_flags_apart()


def test_the_table_holds_what_it_must():
    names = set(TLC.CASE_IDS)
    for axis, edge in zip("xyz", TLC.TILE):
        assert {f"edge_{axis}{edge - 1}", f"edge_{axis}{edge}", f"edge_{axis}{edge + 1}"} <= names
    for name, _, lo, hi in TLC.CASES:
        if name.startswith("edge_"):
            assert all(c % 2 for c in lo), name
    assert TLC.REGIONS["above"][0][1] > 28 and TLC.REGIONS["deep"][1][1] < -150 and TLC.REGIONS["far_x"][0][0] == (1 << 30) - 70
    # the deep region has no surface: every filled voxel is rock or ore; the region above has no voxel
    assert set(np.unique(TLC.voxel_ids({}, *TLC.REGIONS["deep"])).tolist()) == {3, 4}
    assert TLC.voxel_ids({}, *TLC.REGIONS["above"]).size == 0


@pytest.mark.parametrize("name,kw,lo,hi", TLC.CASES, ids=TLC.CASE_IDS)
def test_host_build_matches_the_composition(name, kw, lo, hi):
    TLC.check_reference_tells_the_flags_apart()
    p = TLC.params_of(kw)
    for levels in TLC.ALL_LEVELS:
        for flags in TLC.ALL_FLAGS:
            TLC.same(HL.terrain_reduce_host(p, lo, hi, levels, flags), TLC.reference(kw, lo, hi, levels, flags), f"{name} K={levels} flags={flags}")


def test_seamless_planes_of_a_union_are_the_parts_concatenated():
    """The first region under SEAMLESS, cut at multiples of 8 into 2 x 2 x 2 parts, K = 3: the parts' planes, placed by their grids, are the
    whole's."""
    lo, hi = TLC.LARGE["large_a"]
    cut = (8, 0, 0)
    assert all(l < c < h and c % 8 == 0 for l, c, h in zip(lo, cut, hi))
    p = TLC.params_of({})
    for flags in (TLC.SEAMLESS, TLC.SEAMLESS | TLC.VOTE_EXPOSED):
        whole, winfo = HL.terrain_reduce_host(p, lo, hi, 3, flags)
        TLC.same((whole, winfo), TLC.reference({}, lo, hi, 3, flags))
        built = [[np.full_like(plane, 0xABCD) for plane in level] for level in whole]
        for part in range(8):
            plo = tuple(cut[a] if (part >> a) & 1 else lo[a] for a in range(3))
            phi = tuple(hi[a] if (part >> a) & 1 else cut[a] for a in range(3))
            levels, info = HL.terrain_reduce_host(p, plo, phi, 3, flags)
            for j in range(3):
                off = [int(info["level"][0][j]["clo"][a]) - int(winfo["level"][0][j]["clo"][a]) for a in range(3)]
                ext = [int(c) for c in info["level"][0][j]["cext"]]
                for plane in range(3):
                    built[j][plane][off[2]:off[2] + ext[2], off[1]:off[1] + ext[1], off[0]:off[0] + ext[0]] = levels[j][plane]
        for j in range(3):
            for plane in range(3):
                assert built[j][plane].tobytes() == whole[j][plane].tobytes(), (flags, j + 1, plane)
    # ... and without SEAMLESS the cut faces hide voxels: the promise is SEAMLESS's alone
    whole = HL.terrain_reduce_host(p, lo, hi, 1, 0)[0]
    part = HL.terrain_reduce_host(p, lo, (cut[0], hi[1], hi[2]), 1, 0)[0]
    assert part[0][1].tobytes() != whole[0][1][:, :, :part[0][1].shape[2]].tobytes()


def test_host_build_errors():
    lo, hi = (-8, -24, -8), (8, 30, 8)
    big = 1 << 30
    table = [
        (dict(levels=0), BLOK_ERR_INVALID_ARG), (dict(levels=6), BLOK_ERR_INVALID_ARG), (dict(flags=4), BLOK_ERR_INVALID_ARG), (dict(flags=8), BLOK_ERR_INVALID_ARG),
        (dict(lo=None), BLOK_ERR_INVALID_ARG), (dict(hi=None), BLOK_ERR_INVALID_ARG), (dict(lo=(9, -24, -8)), BLOK_ERR_INVALID_ARG),
        (dict(kw=dict(flags=1)), BLOK_ERR_INVALID_ARG), (dict(kw=dict(flags=4)), BLOK_ERR_INVALID_ARG), (dict(kw=dict(flags=3)), BLOK_ERR_INVALID_ARG),
        (dict(kw=dict(cave_octaves=5)), BLOK_ERR_INVALID_ARG), (dict(kw=dict(density=0.0)), BLOK_ERR_INVALID_ARG),
        (dict(lo=(big - 3, 0, 0), hi=(big + 1, 4, 4)), BLOK_ERR_UNSUPPORTED), (dict(lo=(-big - 1, 0, 0), hi=(-big + 4, 4, 4)), BLOK_ERR_UNSUPPORTED),
        (dict(lo=(0, 0, 0), hi=(65537, 1, 1)), BLOK_ERR_UNSUPPORTED), (dict(lo=(0, 0, 0), hi=(65536, 65536, 4)), BLOK_ERR_UNSUPPORTED),      # 2^31 level-1 cells
    ]
    for change, rc in table:
        args = dict(kw={}, lo=lo, hi=hi, levels=1, flags=0)
        args.update(change)
        with pytest.raises(BlokError) as e:
            HL.terrain_reduce_host(TLC.params_of(args["kw"]), args["lo"], args["hi"], args["levels"], args["flags"])
        assert e.value.status == rc, change
    assert _ffi.host_lib().blok_terrain_reduce(None, HL._vec(lo), HL._vec(hi), 1, 0, None, 0, None) == BLOK_ERR_INVALID_ARG
    # the limits themselves pass: a coordinate of 2^30, an extent of 65536 (the plan alone), and volume_reduce's host build refuses bit 2
    info = np.zeros(1, dtype=HL.INFO)
    p = TLC.params_of({})
    assert _ffi.host_lib().blok_terrain_reduce(C.byref(p), HL._vec((big - 65536, 0, 0)), HL._vec((big, 2, 2)), 5, 3, None, 0, _ffi.ptr(info)) == 0
    assert [int(c) for c in info["level"][0][0]["cext"]] == [32768, 1, 1] and int(info["flags"][0]) == 3
    with pytest.raises(BlokError) as e:
        HL.reduce_host(np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2), np.uint32), flags=HL.SEAMLESS)
    assert e.value.status == BLOK_ERR_INVALID_ARG
    # too small an array is refused; an empty region is fine and empty
    raw = np.zeros(8, dtype=np.uint8)
    assert _ffi.host_lib().blok_terrain_reduce(C.byref(p), HL._vec(lo), HL._vec(hi), 1, 0, _ffi.ptr(raw), 8, None) == BLOK_ERR_INVALID_ARG
    levels, info = HL.terrain_reduce_host(p, (0, 0, 0), (8, 0, 8), 2, 0)
    assert [l[0].size for l in levels] == [0, 0] and int(info["level"][0][0]["n_cells"]) == 0 and [int(c) for c in info["ext"][0]] == [8, 0, 8]


def test_tile_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/terrain_lod_main.cpp): the column words of terrain_lod_core.h — exposure, voters, depth
    classes, the cell — beside a per-voxel loop over seeded tiles; nothing loaded into Python is sanitized."""
    exe = tmp_path / "terrain_lod_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/terrain_lod_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/lod.cpp")], check=True)
    run = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[-1].startswith("ok ") and int(lines[-1].split()[1]) >= 300, run.stdout
