"""CPU: the host builds (blok_column_field / blok_scatter, blok_amd/columns.py) against the numpy model of the contract
(tests/columns_reference.py) on every case the GPU tests run, and — from the model alone — what makes those cases hard.  Every comparison
is exact."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import columns as K
from blok_amd._ffi import BlokError
from tests import columns_reference as R
from tests import limit_cases as LC

BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
ROOT = Path(__file__).resolve().parent.parent


def host_field(c):
    return K.column_field_host(c["d"], c["m"], c["origin"], c["lo"], c["hi"], c["axis"], c["flags"])


def same_field(got, want, tag):
    assert got[0].dtype == np.uint16 and got[1].dtype == np.uint32
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), tag


def scene_field(lo=None, hi=None):
    d, m = R.scene()
    return R.field(d, m, R.SCENE_ORIGIN, lo, hi, 1, 0)


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
def test_record_sizes():
    """The sizes the header states: every record a multiple of 8 bytes."""
    assert _ffi.COLUMNS_INFO.itemsize == 64 and _ffi.SCATTER_ENTRY.itemsize == 24 and _ffi.SCATTER_PARAMS.itemsize == 64 and _ffi.SCATTER_INFO.itemsize == 72
    assert _ffi.INSTANCE.itemsize == 32
    text = (ROOT / "include" / "blok_hip.h").read_text()
    for record, size in (("blok_columns_info", 64), ("blok_scatter_entry", 24), ("blok_scatter_params", 64), ("blok_scatter_info", 72)):
        assert f"}} {record};" in text and f"/* {size} bytes */" in text.split(f"}} {record};")[1].splitlines()[0]
    src = "#include \"blok_hip.h\"\n_Static_assert(sizeof(blok_columns_info) == 64 && sizeof(blok_scatter_entry) == 24 && sizeof(blok_scatter_params) == 64 && " \
          "sizeof(blok_scatter_info) == 72, \"sizes\");\nint main(void) { return 0; }\n"
    r = subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", "-fsyntax-only", "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the model against hand-written cases -------------------------------------------------------------------------------------------------
def test_model_field_by_hand():
    d = np.zeros((1, 6, 3), np.float32)             # [z][y][x]: 3 columns along y of 6 cells
    m = np.arange(18, dtype=np.uint32).reshape(1, 6, 3) + 100
    d[0, 1, 0] = d[0, 4, 0] = 1.0                   # column 0: cells 1 and 4
    d[0, 5, 2] = np.float32(np.nan); d[0, 0, 2] = -1.0      # column 2: nothing filled
    d[0, 0, 1] = 0.5                                # column 1: cell 0
    top, mat, info = R.field(d, m, (10, 20, 30), None, None, 1, 0)
    assert top.tolist() == [4, 0, R.NONE] and mat.tolist() == [112, 101, 0]
    assert [int(info[k][0]) for k in ("n_columns", "n_hit", "min_top", "max_top")] == [3, 2, 0, 4]
    top, mat, _ = R.field(d, m, (10, 20, 30), None, None, 1, R.FROM_LOW)
    assert top.tolist() == [1, 0, R.NONE] and mat.tolist() == [103, 101, 0]
    top, mat, info = R.field(d, m, (10, 20, 30), (10, 22, 30), (13, 26, 31), 1, 0)      # cells 2 .. 5: column 0 sees cell 4 as local 2
    assert top.tolist() == [2, R.NONE, R.NONE] and info["lo"][0].tolist() == [10, 22, 30]
    top, _, info = R.field(d, m, (10, 20, 30), None, None, 0, 0)                        # along x: 6 columns (cp = y), the highest x
    assert top.tolist() == [1, 0, R.NONE, R.NONE, 0, R.NONE] and int(info["n_columns"][0]) == 6


def test_model_hash_matches_the_terrain_hash_of_the_host_library():
    """hash3 restated in numpy against the product's terrain: lattice2 is hash3(i, 0x100 + salt, j, seed) & 0xFFFF — checked through
    Python integers here, and the model's scatter against the host build below."""
    def py_hash3(x, y, z, s):
        M = 0xFFFFFFFF
        h = ((x * 0x9E3779B1) ^ (y * 0x85EBCA77) ^ (z * 0xC2B2AE3D) ^ s) & M
        h ^= h >> 16; h = h * 0x85EBCA6B & M; h ^= h >> 13; h = h * 0xC2B2AE35 & M; h ^= h >> 16
        return h
    for x, z, s in ((0, 0, 0), (1, 2, 3), (-1, -7, 0xFFFFFFFF), (123456, -98765, R.SEED)):
        assert int(R.hash3(x, 0x5CA70001, z, s)) == py_hash3(x & 0xFFFFFFFF, 0x5CA70001, z & 0xFFFFFFFF, s)


# ---- the host field against the model ------------------------------------------------------------------------------------------------------
def test_host_field_equals_the_model_on_the_noise_boxes():
    cases = R.noise_cases()
    for c in cases:
        same_field(host_field(c), R.model_of(c), c["name"])
    d5 = R.noise(0.05)[0]
    assert 0.02 < (d5 > 0).mean() < 0.09 and 0.4 < (R.noise(0.5)[0] > 0).mean() < 0.6
    whole = [c for c in cases if c["lo"] is None and c["axis"] == 1 and c["flags"] == 0]
    sparse, dense = (R.model_of(c) for c in whole)
    assert (sparse[0] == R.NONE).mean() > 0.5, "fill 0.05: mostly NONE"
    assert (dense[0] >= 8).mean() > 0.5, "fill 0.5: early hits from the top"
    empty = [R.model_of(c) for c in cases if c["hi"] == (0, 4, 4)]
    assert all(e[0].size == 0 and int(e[2]["n_columns"][0]) == 0 and int(e[2]["min_top"][0]) == R.NONE for e in empty)


@pytest.mark.parametrize("c", R.seam_cases() + R.stair_cases(), ids=lambda c: c["name"].replace(" ", "-"))
def test_host_field_equals_the_model_on_seams_and_stairs(c):
    same_field(host_field(c), R.model_of(c), c["name"])


@pytest.mark.parametrize("which", ["LOW", "HIGH"])
def test_host_field_equals_the_model_in_the_limit_boxes(which):
    for axis in range(3):
        for flags in (0, R.FROM_LOW):
            c = R.limit_case(which, axis, flags)
            want = R.model_of(c)
            same_field(host_field(c), want, c["name"])
            assert 0 < int(want[2]["n_hit"][0]) < int(want[2]["n_columns"][0])


@pytest.mark.parametrize("box", LC.LONG_BOXES, ids=LC.LONG_IDS)
def test_long_box_closed_form_is_pinned_to_the_model(box):
    """long_expected is what the GPU test holds the 16384-cell boxes against: here it equals field() at LENGTH_PINNED cells, and the host
    build too."""
    short = box.shortened()
    assert short.length == LC.LENGTH_PINNED
    d, m = R.long_fill(short)
    for flags in (0, R.FROM_LOW):
        top, material, info = R.field(d, m, short.origin, None, None, short.axis, flags)
        want = R.long_expected(short, flags)
        assert top.tobytes() == want[0].tobytes() and material.tobytes() == want[1].tobytes()
        same_field(K.column_field_host(d, m, short.origin, None, None, short.axis, flags), (top, material, info), box.name)
        hit = top[top != R.NONE]
        assert 0 in hit.tolist() or short.length - 1 in hit.tolist()
        assert (top == R.NONE).any() and len(set((hit // 64).tolist())) > 3
    full = R.long_expected(box, 0)[0]
    assert int(full[full != R.NONE].max()) == LC.L - 1 and int(R.long_expected(box, R.FROM_LOW)[0].min()) == 0


# ---- from the model alone: what makes the field cases hard ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.hard_cases(), ids=lambda c: c["name"].replace(" ", "-"))
def test_hard_field_cases_are_hard(c):
    """Columns that hit in the region's first cell, in its last cell, and not at all; tops in more than one brick along the axis; the
    region cuts the brick of its first and of its last cell."""
    top, _, info = R.model_of(c)
    axis = c["axis"]
    l, h = R.local_region(c["d"].shape, c["origin"], c["lo"], c["hi"])
    n = h[axis] - l[axis]
    assert (top == 0).any() and (top == n - 1).any() and (top == R.NONE).any(), c["name"]
    bricks = {(int(t) + l[axis]) // 4 for t in top[top != R.NONE]}
    assert len(bricks) > 1
    assert l[axis] % 4 != 0 and h[axis] % 4 != 0, "both end bricks are cut by the region"
    assert l[axis] // 4 in bricks and (h[axis] - 1) // 4 in bricks, "... and hold tops"
    same_field(host_field(c), (top, _, info), c["name"])


# ---- scatter: the host build against the model --------------------------------------------------------------------------------------------
def run_both(lo, hi, p, ent):
    f = scene_field(lo, hi)
    trace = []
    want = R.scatter(*f, p, ent, trace)
    got = K.scatter_host(*f, p, ent)
    assert got[0].dtype == _ffi.INSTANCE and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    counted = K.scatter_host(*f, p, ent, count_only=True)
    assert counted[0] is None and counted[1].tobytes() == want[1].tobytes(), "a NULL table returns the same info"
    return f, want, trace


MAIN = R.main_scatter_cases()


@pytest.mark.parametrize("case", MAIN, ids=[c[0].replace(" ", "-") for c in MAIN])
def test_main_scatter_cases_equal_the_model_and_are_hard(case):
    """With the default seed: every n_rejected slot and n_placed non-zero, every entry and all eight orientations placed, a footprint window
    cut by the region's edge; and every placed anchor lands on its target cell by the header's record-back rule."""
    name, lo, hi, p, ent = case
    f, (table, info), trace = run_both(lo, hi, p, ent)
    info = info[0]
    assert int(info["n_placed"]) > 0 and all(int(n) > 0 for n in info["n_rejected"]), (name, info)
    assert int(info["n_cells"]) == int(info["n_placed"]) + int(info["n_rejected"].sum()) == len(trace)
    placed = [t for t in trace if t[2] == 0]
    assert {t[3] for t in placed} == set(range(len(ent))), "every entry"
    assert {(t[4], t[5]) for t in placed} == {(r, m) for r in range(4) for m in range(2)}, "all eight orientations"
    assert {(tuple(i["axis"]), int(i["flip"])) for i in table} == {((0, 1, 2), 0), ((2, 1, 0), 4), ((0, 1, 2), 5), ((2, 1, 0), 1),
                                                                   ((0, 1, 2), 1), ((2, 1, 0), 5), ((0, 1, 2), 4), ((2, 1, 0), 0)}
    assert any(t[6] and t[2] in (0, 5) for t in trace), "a footprint window cut by the region's edge was checked"
    # the anchor rule, and the order
    top2 = f[0].reshape(int(f[2]["ext"][0][2]), int(f[2]["ext"][0][0]))
    flo = [int(v) for v in f[2]["lo"][0]]
    placed.sort(key=lambda t: (t[1], t[0]))
    assert len(placed) == len(table)
    for t, inst in zip(placed, table):
        X, Z, e = t[0], t[1], t[3]
        target = (X, flo[1] + int(top2[Z - flo[2], X - flo[0]]) + 1 - int(ent["sink"][e]), Z)
        assert R.anchor_lands_on(inst, ent["anchor"][e]) == target and int(inst["model"]) == int(ent["model"][e])
        assert inst["reserved"].tolist() == [0, 0, 0]


SWEEP = R.sweep_scatter_cases()


@pytest.mark.parametrize("case", SWEEP, ids=[c[0].replace(" ", "-") for c in SWEEP])
def test_sweep_scatter_cases_equal_the_model(case):
    name, lo, hi, p, ent = case
    _, (table, info), _ = run_both(lo, hi, p, ent)
    if int(p["probability"][0]) == 0:
        assert len(table) == 0 and int(info["n_rejected"][0][0]) == int(info["n_cells"][0]) > 0


def test_scatter_of_an_empty_field_and_of_a_field_without_candidates():
    f = scene_field((0, 0, 20), (0, 5, 25))
    table, info = K.scatter_host(*f, R.scene_params(), R.entries(R.ENTRIES3))
    assert len(table) == 0 and info.tobytes() == R.scatter(*f, R.scene_params(), R.entries(R.ENTRIES3))[1].tobytes() and int(info["n_cells"][0]) == 0


# ---- seamlessness ----------------------------------------------------------------------------------------------------------------------------
def placements_in(lo, hi, keep_lo, keep_hi, p, ent, radius):
    """Scatter over [lo, hi) widened by `radius` in x and z, filtered to the candidates in [keep_lo, keep_hi): {(X, Z): record bytes}."""
    wlo, whi = (lo[0] - radius, lo[1], lo[2] - radius), (hi[0] + radius, hi[1], hi[2] + radius)
    f = scene_field(wlo, whi)
    trace = []
    table, _ = R.scatter(*f, p, ent, trace)
    got = K.scatter_host(*f, p, ent)[0]
    assert got.tobytes() == table.tobytes()
    placed = sorted((t for t in trace if t[2] == 0), key=lambda t: (t[1], t[0]))
    return {(t[0], t[1]): rec.tobytes() for t, rec in zip(placed, table) if keep_lo[0] <= t[0] < keep_hi[0] and keep_lo[2] <= t[1] < keep_hi[2]}


@pytest.mark.parametrize("c,radius", [(0, 3), (2, 2), (3, 0)])
def test_scatter_is_seamless_over_the_halves_of_a_region(c, radius):
    """The same world column gets the same decision whatever region was taken: a region and its two halves, each field taken `radius`
    wider and filtered to its own columns, give the same placements.  The regions lie off the cell grid and across x = 0."""
    o = R.SCENE_ORIGIN
    lo, hi = (o[0] + 9, o[1], o[2] + 10), (o[0] + 71, o[1] + 40, o[2] + 69)
    mid = o[0] + 37
    assert lo[0] < 0 < mid and mid % (1 << c) != 0 or c == 0
    p, ent = R.scene_params(cell_log2=c, radius=radius, probability=50000), R.entries(R.ENTRIES3)
    whole = placements_in(lo, hi, lo, hi, p, ent, radius)
    left = placements_in(lo, (mid, hi[1], hi[2]), lo, (mid, hi[1], hi[2]), p, ent, radius)
    right = placements_in((mid, lo[1], lo[2]), hi, (mid, lo[1], lo[2]), hi, p, ent, radius)
    assert len(whole) >= 10 and left and right and not set(left) & set(right)      # (not vacuous: placements on both sides)
    assert {**left, **right} == whole


def test_candidates_use_arithmetic_shifts_either_side_of_zero():
    """Cells -1 and 0 are different cells with candidates inside their own 2^c columns: a field across x = 0 and z = 0."""
    d = np.ones((40, 2, 40), np.float32)
    m = np.ones(d.shape, np.uint32)
    f = R.field(d, m, (-20, 0, -20), None, None, 1, 0)
    for c in (1, 3, 4):
        p, ent = R.params(cell_log2=c, flags=R.ANY_MATERIAL), R.entries([(0, 1, (0, 0, 0), 0)])
        trace = []
        want = R.scatter(*f, p, ent, trace)
        got = K.scatter_host(*f, p, ent)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        S = 1 << c
        cells = {(X >> c, Z >> c) for X, Z, *_ in trace}
        assert len(cells) == len(trace) and (-1, -1) in cells and (0, 0) in cells and (-1, 0) in cells, "one candidate per cell, on both sides of zero"
        assert all((X >> c) * S <= X < (X >> c) * S + S for X, Z, *_ in trace)
        # the same world columns from a field that starts elsewhere
        g = R.field(d, m, (-20, 0, -20), (-13, 0, -9), (17, 2, 11), 1, 0)
        sub = []
        R.scatter(*g, p, ent, sub)
        assert {(t[0], t[1]) for t in sub} == {(t[0], t[1]) for t in trace if -13 <= t[0] < 17 and -9 <= t[1] < 11}


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_host_field_refusals():
    d, m = R.noise(0.5)
    o = R.NOISE_ORIGIN

    def refused(status, *a):
        with pytest.raises(BlokError) as e:
            K.column_field_host(d, m, o, *a)
        assert e.value.status == status, a

    refused(BLOK_ERR_INVALID_ARG, None, None, 3)                                   # axis above 2
    refused(BLOK_ERR_INVALID_ARG, None, None, 1, 2)                                # unknown flag bits
    refused(BLOK_ERR_INVALID_ARG, None, None, 1, 1 << 31)
    refused(BLOK_ERR_INVALID_ARG, (0, 2, 0), (1, 1, 1), 1)                         # lo above hi
    refused(BLOK_ERR_UNSUPPORTED, (-6, 0, 0), (1, 1, 1), 1)                        # a region that leaves the box
    refused(BLOK_ERR_UNSUPPORTED, (0, 0, 0), (1, 1, 6), 1)
    lib = _ffi.host_lib()
    vec = lambda v: (C.c_int32 * 3)(*v)
    top, mat = np.zeros(200, np.uint16), np.zeros(200, np.uint32)
    args = (_ffi.ptr(d), _ffi.ptr(m), vec(o), 13, 10, 7)
    assert lib.blok_column_field(*args, vec((0, 0, 0)), None, 1, 0, _ffi.ptr(top), _ffi.ptr(mat), None) == BLOK_ERR_INVALID_ARG      # one region pointer
    assert lib.blok_column_field(*args, None, vec((1, 1, 1)), 1, 0, _ffi.ptr(top), _ffi.ptr(mat), None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_column_field(*args, None, None, 1, 0, None, _ffi.ptr(mat), None) == BLOK_ERR_INVALID_ARG                         # a NULL array, a region with cells
    assert lib.blok_column_field(*args, None, None, 1, 0, _ffi.ptr(top), None, None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_column_field(None, _ffi.ptr(m), vec(o), 13, 10, 7, None, None, 1, 0, _ffi.ptr(top), _ffi.ptr(mat), None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_column_field(*args, None, None, 1, 0, _ffi.ptr(top), _ffi.ptr(mat), None) == 0                                   # out_info may be NULL
    assert lib.blok_column_field(*args, vec((0, 0, 0)), vec((0, 4, 4)), 1, 0, None, None, None) == 0                                 # an empty region needs no arrays


def test_host_scatter_refusals():
    f = scene_field()
    ent = R.entries(R.ENTRIES3)

    def refused(p=None, e=ent, field=f):
        with pytest.raises(BlokError) as err:
            K.scatter_host(*field, R.scene_params() if p is None else p, e)
        assert err.value.status == BLOK_ERR_INVALID_ARG

    refused(R.scene_params(flags=8))                                               # unknown flag bits
    bad = R.scene_params(); bad["reserved"][0][5] = 1
    refused(bad)                                                                   # a non-zero reserved word
    refused(R.scene_params(cell_log2=9))
    refused(R.scene_params(probability=65537))
    refused(R.scene_params(radius=9))
    refused(R.scene_params(max_rise=0x10000))
    refused(R.scene_params(max_drop=0x10000))
    refused(R.scene_params(min_y=5, max_y=4))
    refused(e=ent[:0])                                                             # no entries
    refused(e=R.entries([R.ENTRIES3[0]] * 17))                                     # more than 16
    refused(e=R.entries([(0, 0, (0, 0, 0), 0)]))                                   # a zero weight
    refused(e=R.entries([(0, 5, (0, 0, 0), 0), (0, 65536, (0, 0, 0), 0)]))         # a weight above 65535
    d, m = R.scene()
    refused(field=R.field(d, m, R.SCENE_ORIGIN, None, None, 1, R.FROM_LOW))        # the wrong direction
    refused(field=R.field(d, m, R.SCENE_ORIGIN, None, None, 0, 0))                 # the wrong axis
    refused(field=R.field(d, m, R.SCENE_ORIGIN, None, None, 2, 0))
    lib = _ffi.host_lib()
    p = R.scene_params()
    out = np.zeros(1, _ffi.SCATTER_INFO)
    a = (_ffi.ptr(f[0]), _ffi.ptr(f[1]), _ffi.ptr(f[2]))
    assert lib.blok_scatter(*a, None, _ffi.ptr(ent), 3, None, 0, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG                              # NULL parameters
    assert lib.blok_scatter(*a, _ffi.ptr(p), None, 3, None, 0, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG                                # NULL entries
    assert lib.blok_scatter(a[0], a[1], None, _ffi.ptr(p), _ffi.ptr(ent), 3, None, 0, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG         # no column info
    assert lib.blok_scatter(None, a[1], a[2], _ffi.ptr(p), _ffi.ptr(ent), 3, None, 0, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG         # a NULL plane
    assert lib.blok_scatter(a[0], None, a[2], _ffi.ptr(p), _ffi.ptr(ent), 3, None, 0, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG
    assert lib.blok_scatter(*a, _ffi.ptr(p), _ffi.ptr(ent), 3, None, 0, None) == 0                                                   # out_info may be NULL
    n = int(K.scatter_host(*f, p, ent, count_only=True)[1]["n_placed"][0])
    table = np.zeros(n, _ffi.INSTANCE)
    assert n > 1 and lib.blok_scatter(*a, _ffi.ptr(p), _ffi.ptr(ent), 3, _ffi.ptr(table), n - 1, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG      # a table too small ...
    assert not table.tobytes().strip(b"\0"), "... and nothing written"


# ---- the host builds under sanitizers, in a program of their own -----------------------------------------------------------------------------
def _checksum(a):
    w = np.ascontiguousarray(a).reshape(-1)
    w = (w.view(np.uint32) if w.dtype.itemsize >= 4 else w).astype(np.uint64)
    return int((w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_host_builds_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/columns_main.cpp) over case files: noise boxes, the hard field cases, a seam box, the main
    scatter cases and some of the sweep, and calls that are refused; nothing loaded into Python is sanitized."""
    exe = tmp_path / "columns_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/columns_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/columns.cpp")], check=True)
    d, m = R.scene()
    scene_case = lambda lo, hi: R.case("scene", R.SCENE_ORIGIN, d, m, lo, hi, 1, 0)
    jobs = [(c, None, None) for c in R.noise_cases()[::5] + R.hard_cases() + R.seam_cases()[:4]]
    jobs += [(scene_case(lo, hi), p, ent) for _, lo, hi, p, ent in MAIN + SWEEP[::4]]
    first = R.noise_cases()[0]
    jobs += [(dict(first, name="refused axis", axis=3), None, None), (dict(first, name="refused region", lo=(-9, 0, 0), hi=(1, 1, 1)), None, None),
             (dict(scene_case(None, None), name="refused scatter"), R.scene_params(radius=9), R.entries(R.ENTRIES3)),
             (dict(scene_case(None, None), name="refused direction", flags=R.FROM_LOW), R.scene_params(), R.entries(R.ENTRIES3))]
    files, want = [], []
    for i, (c, p, ent) in enumerate(jobs):
        nx, ny, nz = c["shape"]
        whole = c["lo"] is None
        head = np.array([nx, ny, nz, *c["origin"], int(whole), *(c["lo"] or (0, 0, 0)), *(c["hi"] or (0, 0, 0)), c["axis"], c["flags"], 0 if ent is None else len(ent)], np.int32)
        path = tmp_path / f"case{i}.bin"
        path.write_bytes(head.tobytes() + c["d"].tobytes() + c["m"].tobytes() + (b"" if ent is None else p.tobytes() + ent.tobytes()))
        files.append(os.fspath(path))
        if c["name"] in ("refused axis", "refused region"):
            want.append(("-1" if c["name"] == "refused axis" else "-5", None))
            continue
        top, material, info = R.model_of(c)
        line = f"0 {int(info['n_columns'][0])} {int(info['n_hit'][0])} {int(info['min_top'][0])} {int(info['max_top'][0])} {_checksum(top)} {_checksum(material)}"
        if ent is None:
            line += " -99 0 0 0 0 0 0 0 0"
        elif c["name"].startswith("refused"):
            line += " -1 0 0 0 0 0 0 0 0"
        else:
            table, s = R.scatter(top, material, info, p, ent)
            s = s[0]
            line += f" 0 {int(s['n_cells'])} {int(s['n_placed'])} " + " ".join(str(int(n)) for n in s["n_rejected"]) + f" {_checksum(table.view(np.uint32))}"
        want.append((line, c["name"]))
    run = subprocess.run([os.fspath(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(files)
    for line, (expected, name) in zip(lines, want):
        if name is None:
            assert line.split()[0] == expected and line.split()[7] == "-99", line
        else:
            assert line == expected, (name, line, expected)
