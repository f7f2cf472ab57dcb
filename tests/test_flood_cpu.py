"""CPU: the numpy model of the flood (tests/flood_reference.py) against hand-written cases, the host build (blok_flood_field /
blok_flood_edit, blok_amd/flood.py) against the model on every shape the GPU tests run, and — from the model alone — what makes the GPU
cases hard.  Every comparison is exact."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import flood as F
from blok_amd._ffi import BlokError
from tests import flood_reference as R

BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
ROOT = Path(__file__).resolve().parent.parent
FAR = R.FAR


def grid(rows):
    """One z layer from strings, '.' passable (empty), '#' filled: (density, ids) [1][y][x]."""
    p = np.array([[c == "." for c in row] for row in rows])[None]
    return R.volume_of(p)


def steps_of(rows, seeds, K=R.MAX_STEPS, flags=0):
    d, m = grid(rows)
    return R.field(d, m, (0, 0, 0), None, None, seeds, K, flags)[0][0]


# ---- the model against hand-written cases ----------------------------------------------------------------------------------------------------
def test_model_corridor_with_a_bend():
    got = steps_of(["....#",
                    "###.#",
                    "#...#"], [(0, 0, 0)])
    F_ = FAR
    assert got.tolist() == [[0, 1, 2, 3, F_], [F_, F_, F_, 4, F_], [F_, 7, 6, 5, F_]]


def test_model_wall_with_one_hole():
    got = steps_of(["..#..",
                    "..#..",
                    ".....",
                    "..#.."], [(0, 0, 0)])
    assert got[0].tolist() == [0, 1, FAR, 7, 8] and got[2].tolist() == [2, 3, 4, 5, 6] and got[3].tolist() == [3, 4, FAR, 6, 7]


def test_model_caps():
    row = ["........"]
    assert steps_of(row, [(2, 0, 0)], K=0).tolist() == [[FAR, FAR, 0, FAR, FAR, FAR, FAR, FAR]]      # K = 0: the seeds alone
    got = steps_of(row, [(0, 0, 0)], K=5)[0].tolist()
    assert got == [0, 1, 2, 3, 4, 5, FAR, FAR]                     # a path of exactly K is kept, one of K + 1 is FAR
    d, m = grid(row)
    info = R.field(d, m, (0, 0, 0), None, None, [(0, 0, 0)], 5, 0)[1]
    assert [int(info[k][0]) for k in ("farthest", "n_seed", "n_reached", "n_unreached")] == [5, 1, 5, 2]
    info = R.field(d, m, (0, 0, 0), None, None, [(0, 0, 0)], 9, 0)[1]
    assert int(info["farthest"][0]) == 7 < 9 and int(info["n_unreached"][0]) == 0      # below the cap: the flood ended on its own


def test_model_seed_on_an_impassable_cell_and_diagonal_contact():
    rows = [".#",
            "#."]
    assert steps_of(rows, [(1, 0, 0)]).tolist() == [[FAR, FAR], [FAR, FAR]]      # the seed is filled: ignored, no seed at all
    assert steps_of(rows, [(0, 0, 0)]).tolist() == [[0, FAR], [FAR, FAR]]        # diagonal contact is not a step
    assert steps_of(rows, [(1, 0, 0)], flags=R.THROUGH_FILLED).tolist() == [[FAR, 0], [FAR, FAR]]
    assert steps_of(rows, [(0, 0, 0), (0, 0, 0), (1, 1, 0)]).tolist() == [[0, FAR], [FAR, 0]]      # duplicates are harmless


def test_model_faces_materials_and_regions():
    d = np.ones((1, 3, 4), np.float32)
    m = np.array([[[1, 1, 2, 2], [1, 2, 2, 1], [1, 1, 1, 1]]], np.uint32)
    got = R.field(d, m, (10, 20, 30), None, None, [(10, 20, 30)], 9, R.THROUGH_FILLED | R.SAME_MATERIAL, 1)[0][0]
    assert got.tolist() == [[0, 1, FAR, FAR], [1, FAR, FAR, 6], [2, 3, 4, 5]]
    # the -X face of a region that is the box without its first column: the region's own outermost layer, and no path through the column
    e = np.zeros((1, 3, 4), np.float32)
    got, info = R.field(e, m, (10, 20, 30), (11, 20, 30), (14, 23, 31), None, 9, R.seed_face(1))
    assert got[0].tolist() == [[0, 1, 2]] * 3 and info["lo"][0].tolist() == [11, 20, 30] and info["ext"][0].tolist() == [3, 3, 1]
    got, _ = R.field(e, m, (10, 20, 30), None, None, None, 9, R.seed_face(2))      # +Y: the high side
    assert got[0].tolist() == [[2] * 4, [1] * 4, [0] * 4]


# ---- the host build against the model ----------------------------------------------------------------------------------------------------------
def host(case):
    return F.flood_field_host(case["d"], case["m"], case["origin"], case["lo"], case["hi"], case["seeds"], case["K"], case["flags"], case["material"])


def same(got, want, tag):
    assert got[0].dtype == np.uint16 and got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), tag
    assert got[1].tobytes() == want[1].tobytes(), (tag, got[1], want[1])


def test_host_build_on_the_noise_boxes_in_all_modes():
    """13 x 10 x 7 at a negative origin, 30 %, 45 % and 90 % passable; all modes, whole and ragged regions, listed and face seeds."""
    cases = R.noise_cases()
    assert len(cases) > 80 and {c["flags"] & 3 for c in cases} == {0, 1, 3}
    for case in cases:
        same(host(case), R.model_of(case), case["name"])


def test_host_build_on_the_hard_cases_and_the_long_corridors():
    for case in R.hard_cases() + [R.corridor(axis) for axis in range(3)]:
        same(host(case), R.model_of(case), case["name"])


def test_zero_negative_minus_zero_and_nan_densities_are_empty():
    d = np.array([[[1.0, 0.0, -0.0, -2.0, np.nan, 1e-30, 1.0]]], np.float32)
    m = np.arange(7, dtype=np.uint32)[None, None]
    for flags, seed in ((0, (1, 0, 0)), (R.THROUGH_FILLED, (5, 0, 0))):
        got = F.flood_field_host(d, m, (0, 0, 0), None, None, [seed], 9, flags)
        same(got, R.field(d, m, (0, 0, 0), None, None, [seed], 9, flags), flags)
    assert F.flood_field_host(d, None, (0, 0, 0), None, None, [(1, 0, 0)], 9, 0)[0][0, 0].tolist() == [FAR, 0, 1, 2, 3, FAR, FAR]
    assert F.flood_field_host(d, None, (0, 0, 0), None, None, [(5, 0, 0)], 9, R.THROUGH_FILLED)[0][0, 0].tolist() == [FAR] * 5 + [0, 1]


def scene_edit_cases():
    """(tag, lo, hi, seeds, K, flags, flood material, op, d) on the 40 x 36 x 33 scene: the edits the GPU tests apply."""
    a, b = R.world(R.BLOCK_A[0]), R.world(R.BLOCK_B[0])
    inside = R.world((R.HOLE[0], R.HOLE[1], R.HOLED[0][2] + 1))
    return [("seal", None, None, None, R.MAX_STEPS, R.ALL_FACES, 0, R.FILL_UNREACHED, 0),
            ("pour", R.world((0, 0, 0)), R.world((40, 36, R.HOLE[2] - 3)), [inside], R.MAX_STEPS, 0, 0, R.FILL, R.MAX_STEPS),
            ("plug", None, None, [R.world(R.HOLE)], 40, 0, 0, R.FILL, 3),
            ("paint A", None, None, [a], R.MAX_STEPS, R.THROUGH_FILLED | R.SAME_MATERIAL, 3, R.PAINT, R.MAX_STEPS),
            ("paint", (7, -4, 14), (43, 28, 43), [b], 20, R.THROUGH_FILLED, 0, R.PAINT, 12),
            ("clear", None, None, [b], 30, R.THROUGH_FILLED, 0, R.CLEAR, 7)]


def test_the_four_edits_with_counts():
    o = R.SCENE_ORIGIN
    for tag, lo, hi, seeds, K, flags, fm, op, dd in scene_edit_cases():
        d, m = R.scene()
        hd, hm = d.copy(), m.copy()
        want = R.field(d, m, o, lo, hi, seeds, K, flags, fm)
        got = F.flood_field_host(hd, hm, o, lo, hi, seeds, K, flags, fm)
        same(got, want, tag)
        n = F.flood_edit_host(hd, hm, o, *got, op, dd, 0.75, 6)
        assert n == R.edit(d, m, *want, op, dd, 0.75, 6, origin=o) > 0, tag
        assert hd.tobytes() == d.tobytes() and hm.tobytes() == m.tobytes(), tag
        if tag == "seal":
            assert n == R.CLOSED_INSIDE and int(want[1]["farthest"][0]) < R.MAX_STEPS      # exactly the closed box's inside
        if tag == "paint A":
            assert n == 9 * 9 * 8 and hd.tobytes() == R.scene()[0].tobytes(), "PAINT leaves the densities bit-identical"
            assert int((hm == 4).sum()) == 7 * 10 * 11                                     # the touching block of another id is left alone
        if tag == "pour":
            assert n == 9 * 8 * 4                                                          # the holed box's inside below the region's top


def test_edits_judge_the_cells_as_they_are_now():
    o = R.SCENE_ORIGIN
    d, m = R.scene()
    for op, flags, seeds in ((R.FILL, R.ALL_FACES, None), (R.FILL_UNREACHED, R.ALL_FACES, None), (R.PAINT, R.THROUGH_FILLED, [R.world((13, 26, 21))]),
                             (R.CLEAR, R.THROUGH_FILLED, [R.world((13, 26, 21))])):
        steps, info = F.flood_field_host(d, m, o, None, None, seeds, 9, flags)
        kept = steps.copy()
        d[0, 0, 0:2] = 2.5; m[0, 0, 0:2] = 8                       # filled after the field: FILL must skip them
        d[5, 5, 5:7] = 1.0; m[5, 5, 5:7] = 8                       # ... in the closed box: FILL_UNREACHED must skip them
        d[14, 18, 5] = 0.0; m[14, 18, 5] = 0                       # cleared after the field: PAINT and CLEAR must skip it
        hd, hm = d.copy(), m.copy()
        n = F.flood_edit_host(hd, hm, o, steps, info, op, 4, 1.25, 6)
        assert n == R.edit(d, m, steps, info, op, 4, 1.25, 6, origin=o) > 0
        assert hd.tobytes() == d.tobytes() and hm.tobytes() == m.tobytes() and steps.tobytes() == kept.tobytes()
        assert (op in (R.FILL, R.FILL_UNREACHED) or (d[14, 18, 5] == 0 and m[14, 18, 5] == 0)) and (op != R.FILL or m[0, 0, 0] == 8) and (op != R.FILL_UNREACHED or m[5, 5, 5] == 8)


def test_host_error_table():
    d, m = R.noise()
    o = R.NOISE_ORIGIN
    seeds = R.picked_seeds(d, m, o, None, None, 0, 0)

    def refused(status, fn, *a, **k):
        with pytest.raises(BlokError) as e:
            fn(*a, **k)
        assert e.value.status == status, (a, k)

    field = lambda **k: F.flood_field_host(d, m, o, **k)
    refused(BLOK_ERR_INVALID_ARG, field, seeds=seeds, max_steps=65535)
    refused(BLOK_ERR_INVALID_ARG, field, seeds=seeds, flags=R.SAME_MATERIAL)
    refused(BLOK_ERR_INVALID_ARG, field, seeds=seeds, flags=4)
    refused(BLOK_ERR_INVALID_ARG, field, lo=(0, 2, 0), hi=(1, 1, 1))
    refused(BLOK_ERR_UNSUPPORTED, field, lo=(-6, 0, 0), hi=(1, 1, 1))
    refused(BLOK_ERR_INVALID_ARG, field, seeds=[(8, 0, 0)])                                # a seed outside the box
    refused(BLOK_ERR_INVALID_ARG, field, lo=(-4, -2, -1), hi=(7, 6, 4), seeds=[(-5, 0, 0)])      # ... inside the box, outside the region
    lib = _ffi.host_lib()
    assert lib.blok_flood_field(_ffi.ptr(d), None, None, 13, 10, 7, None, None, None, 1, 3, 0, 0, None, None) == BLOK_ERR_INVALID_ARG      # NULL seeds, n_seeds > 0
    steps, info = field(seeds=seeds, max_steps=3)
    assert steps.size == 13 * 10 * 7 and field(lo=(0, 0, 0), hi=(0, 3, 2))[0].size == 0    # an empty region is fine
    before = d.tobytes(), m.tobytes()
    sized = lambda info_: steps if steps.size == int(np.prod(info_["ext"][0].astype(np.int64))) else np.full(int(np.prod(info_["ext"][0].astype(np.int64))), FAR, np.uint16)
    edit = lambda info_, op, dd, value=1.0: F.flood_edit_host(d, m, o, sized(info_), info_, op, dd, value, 6)
    refused(BLOK_ERR_INVALID_ARG, edit, info, 4, 1)                                        # an unknown op
    refused(BLOK_ERR_INVALID_ARG, edit, info, R.PAINT, 1)                                  # an op on the wrong kind of field
    refused(BLOK_ERR_INVALID_ARG, edit, info, R.CLEAR, 1)
    refused(BLOK_ERR_INVALID_ARG, edit, info, R.FILL, 4)                                   # d above max_steps
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(BLOK_ERR_INVALID_ARG, edit, info, R.FILL, 1, bad)
        refused(BLOK_ERR_INVALID_ARG, edit, info, R.FILL_UNREACHED, 0, bad)
    for name, value, status in (("version", 2, BLOK_ERR_INVALID_ARG), ("flags", 1 << 20, BLOK_ERR_INVALID_ARG), ("flags", R.SAME_MATERIAL, BLOK_ERR_INVALID_ARG),
                                ("max_steps", 65535, BLOK_ERR_INVALID_ARG), ("ext", [14, 10, 7], BLOK_ERR_UNSUPPORTED), ("lo", [-6, -3, -2], BLOK_ERR_UNSUPPORTED)):
        forged = info.copy()
        forged[name][0] = value
        refused(status, edit, forged, R.FILL, 1)                                           # a forged info is checked, never trusted
    assert (d.tobytes(), m.tobytes()) == before
    assert edit(info, R.FILL, 0) == int(info["n_seed"][0])                                 # d = 0: the seeds themselves


def _checksum(a):
    w = np.ascontiguousarray(a).reshape(-1)
    w = (w.view(np.uint32) if w.dtype.itemsize == 4 else w).astype(np.uint64)
    return int((w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_host_build_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/flood_main.cpp) over case files: the noise boxes in all modes with an edit each, the hard
    cases, one long corridor, and calls that are refused; nothing loaded into Python is sanitized."""
    exe = tmp_path / "flood_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/flood_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/flood.cpp")], check=True)
    cases = R.noise_cases()[::3] + R.hard_cases() + [R.corridor(1, 2048)]
    refused = dict(cases[0], name="refused seed", seeds=[(100, 0, 0)]), dict(cases[0], name="refused flags", flags=R.SAME_MATERIAL), dict(cases[0], name="refused region", lo=(-9, 0, 0), hi=(1, 1, 1))
    files, want = [], []
    for i, case in enumerate(cases + list(refused)):
        nx, ny, nz = case["shape"]
        whole = case["lo"] is None
        seeds = np.asarray(case["seeds"] if case["seeds"] is not None else [], np.int32).reshape(-1, 3)
        op = (R.PAINT, R.CLEAR)[i % 2] if case["flags"] & R.THROUGH_FILLED else (R.FILL, R.FILL_UNREACHED)[i % 2]
        dd = min(case["K"], 4)
        head = np.array([nx, ny, nz, *case["origin"], int(whole), *(case["lo"] or (0, 0, 0)), *(case["hi"] or (0, 0, 0)), len(seeds), case["K"], case["flags"], case["material"], op, dd], np.int32)
        path = tmp_path / f"case{i}.bin"
        path.write_bytes(head.tobytes() + case["d"].tobytes() + case["m"].tobytes() + seeds.tobytes())
        files.append(os.fspath(path))
        if i >= len(cases):
            want.append(None)
            continue
        d, m = case["d"].copy(), case["m"].copy()
        steps, info = host(case)
        n = F.flood_edit_host(d, m, case["origin"], steps, info, op, dd, 0.75, 6)
        want.append(f"0 0 {int(info['farthest'][0])} {int(info['n_seed'][0])} {int(info['n_reached'][0])} {int(info['n_unreached'][0])} {n} {_checksum(steps)} {_checksum(d)} {_checksum(m)}")
    run = subprocess.run([os.fspath(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(files)
    for line, expected, case in zip(lines, want, cases + list(refused)):
        if expected is None:
            assert line.split()[0] in ("-1", "-5") and line.split()[1] == "-99", (case["name"], line)
        else:
            assert line == expected, (case["name"], line, expected)


# ---- from the model alone: what makes the GPU cases hard -------------------------------------------------------------------------------------
def test_the_maze_has_cells_first_reached_through_few_bricks_and_lowered_later():
    d, m, seed = R.maze()
    p = d == 0
    assert 0.40 < p.mean() < 0.50
    start = np.zeros(p.shape, bool)
    start[seed[2], seed[1], seed[0]] = True
    pools = R.pockets(p)
    nx, ny, _ = R.MAZE_SHAPE
    assert p[seed[2], seed[1], seed[0]] and seed[0] + nx * (seed[1] + ny * seed[2]) in pools[0] and len(pools[0]) > len(pools[1]), "the seed lies in the largest pocket"
    hard = R.claims(p, start)
    info = R.field(d, m, (0, 0, 0), None, None, [seed], R.MAX_STEPS, 0)[1]
    print(hard, info)
    assert hard["crossing_gap"] >= 2 and 30 <= int(info["farthest"][0]) <= 60 and int(info["n_unreached"][0]) > 0


def test_the_snake_needs_twenty_sweeps_inside_one_brick():
    d, m, seed = R.snake()
    steps, info = R.field(d, m, (0, 0, 0), None, None, [seed], R.MAX_STEPS, 0)
    assert int(info["farthest"][0]) >= 20 and steps[2, 0, 0] == 20 and steps[0, 3, 0] == 9 and steps[1, 3, 0] == 10
    assert int(info["n_unreached"][0]) == 0 and int(info["n_reached"][0]) == 20
    start = np.zeros((4, 4, 4), bool)
    start[0, 0, 0] = True
    assert R.claims(d == 0, start) == {"crossing_gap": 0, "longest_in_brick": 20}


def test_the_caps_cut_the_line_boxes_and_the_tunnels_cross_every_face():
    for axis in range(3):
        shape, d, m, seed = R.line_box(axis)
        for K in (255, 599):
            steps = R.field(d, m, (0, 0, 0), None, None, [seed], K, 0)[0]
            assert steps.tobytes() == R.manhattan(shape, seed, K).tobytes()
            assert (steps == K).any() and (steps == FAR).any(), "cells at exactly K and FAR at K + 1 both exist"
        for end in range(2):
            shape, d, m, seed = R.tunnel(12, axis, end)
            steps, info = R.field(d, m, (0, 0, 0), None, None, [seed], R.MAX_STEPS, 0)
            assert int(info["farthest"][0]) == 11 and int(info["n_reached"][0]) == 11 and int(info["n_unreached"][0]) == 0
            far_end = [2 if (a - axis) % 3 == 1 else 1 for a in range(3)]
            far_end[axis] = 0 if end else 11
            assert steps[far_end[2], far_end[1], far_end[0]] == 11  # the only route: through three bricks along the axis, in one direction
