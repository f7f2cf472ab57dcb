"""CPU: the numpy model of the sweep's contract (tests/sweep_reference.py) pinned to hand-written cases, the host build
(blok_sweep_voxels, through blok_amd.sweep) pinned to the model on every shape the GPU tests use, what makes those shapes hard asserted
from the model alone, and the host function's error table."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import stamp as ST
from blok_amd import sweep as SW
from blok_amd._ffi import BlokError
from tests import sweep_reference as R

BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
FAR = 0xFFFFFFFF
LINE_ORIGIN = (-5, -3, -2)                                     # a negative box origin throughout


def line_box(axis, n=80):
    """An empty box n long along `axis` and 3 thick across, [z][y][x]."""
    shape = [3, 3, 3]
    shape[axis] = n
    return np.zeros(tuple(shape[::-1]), dtype=np.float32)


def cell(d, axis, c, u=1, v=1):
    """The index of the cell at c along the axis, (u, v) across, of a [z][y][x] array."""
    p = [0, 0, 0]
    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = c, u, v
    return (p[2], p[1], p[0])


def voxel_at(axis, c, u=1, v=1):
    p = [0, 0, 0]
    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = c, u, v
    return (tuple(LINE_ORIGIN[a] + p[a] for a in range(3)), (0, 1, 2), 0)


def both(d, origin, xyz, place, direction, max_distance, flags=0):
    """The model's answer, after checking that the host build gives the same."""
    want = R.sweep(d, origin, xyz, place, direction, max_distance, flags)
    got = SW.sweep_voxels_host(d, origin, xyz, ST.placement(*place), direction, max_distance, flags)
    assert (int(got["n_overlap"]), int(got["travel"]), int(got["blocked"])) == want, (place, direction, max_distance, flags)
    return want


ONE = np.zeros((1, 3), dtype=np.int32)


@pytest.mark.parametrize("direction", range(6))
def test_the_model_on_hand_written_lines(direction):
    axis, step = direction // 2, (-1 if direction & 1 else 1)
    start = 3 if step > 0 else 76
    for k in (1, 2, 4, 5, 16, 17, 64, 65):                     # an obstacle k cells ahead: k - 1 free steps
        d = line_box(axis)
        d[cell(d, axis, start + step * k)] = 1.0
        assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 100) == (0, k - 1, 1), k
        # a filled column one aside, a filled cell directly behind and the start cell itself filled: none of them blocks
        for c in range(80):
            d[cell(d, axis, c, u=2)] = 1.0
            d[cell(d, axis, c, v=0)] = 1.0
        d[cell(d, axis, start - step)] = 1.0
        assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 100) == (0, k - 1, 1), k
        d[cell(d, axis, start)] = 1.0
        assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 100) == (1, k - 1, 1), k
    d = line_box(axis)
    d[cell(d, axis, start + step * 10)] = 1.0
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 9) == (0, 9, 0)        # the obstacle at max_distance + 1: not blocked
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 10) == (0, 9, 1)       # at max_distance: blocked one short of it
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 0) == (0, 0, 0)        # the pure overlap test
    d[cell(d, axis, start)] = 0.25
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 0) == (1, 0, 0)
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, FAR) == (1, 9, 1)
    # zero, negative and NaN densities are empty
    d = line_box(axis)
    d[cell(d, axis, start + step * 1)] = -1.0
    d[cell(d, axis, start + step * 2)] = np.nan
    d[cell(d, axis, start + step * 3)] = -0.0
    d[cell(d, axis, start)] = np.nan
    d[cell(d, axis, start + step * 7)] = 1e-30
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, 50) == (0, 6, 1)
    # nothing ahead: free for any distance, or up to the box's wall with the flag (cells start + 1 .. 79, or start - 1 .. 0)
    d = line_box(axis)
    to_wall = 79 - start if step > 0 else start
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, FAR) == (0, FAR, 0)
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, FAR, R.BOX_IS_SOLID) == (0, to_wall, 1)
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, start), direction, to_wall, R.BOX_IS_SOLID) == (0, to_wall, 0)
    # starting outside: in front of the box the voxel flies in (12 empty cells, then the box's 80), behind it nothing is ahead
    before = -13 if step > 0 else 92
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, before), direction, 1000) == (0, 1000, 0)
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, before), direction, 1000, R.BOX_IS_SOLID) == (1, 0, 1)
    d[cell(d, axis, 40)] = 1.0
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, before), direction, 1000) == (0, 52 if step > 0 else 51, 1)
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, 92 if step > 0 else -13), direction, 1000) == (0, 1000, 0)
    # a column that misses the box across: free without the flag, stuck with it
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, 20, u=3), direction, 30) == (0, 30, 0)
    assert both(d, LINE_ORIGIN, ONE, voxel_at(axis, 20, u=-1), direction, 30, R.BOX_IS_SOLID) == (1, 0, 1)


def test_the_host_build_equals_the_model_on_every_shared_case():
    models = R.models()
    total = 0
    for scene, d in R.scenes().items():
        want = R.expected(scene)
        for (tag, name, place, direction, max_distance, flags), w in zip(R.cases()[scene], want):
            got = SW.sweep_voxels_host(d, R.ORIGIN, models[name], ST.placement(*place), direction, max_distance, flags)
            assert (int(got["n_overlap"]), int(got["travel"]), int(got["blocked"])) == w, (scene, tag)
            total += 1
    assert total > 600


def test_what_makes_the_shapes_hard():
    models, scenes = R.models(), R.scenes()
    # the comb: the minimum comes from the middle tooth alone, neither the first nor the last voxel of the list or of x-fastest order
    place = R.at(R.COMB_AT)
    _, free, v = R.per_voxel(scenes["plate"], R.ORIGIN, models["comb"], place, 3, 100)
    best = [i for i in range(len(v)) if free[i] == min(free)]
    assert min(free) == 5 and [tuple(v[i]) for i in best] == [(8, 1, 0)]
    order = sorted(range(len(v)), key=lambda i: (v[i][2], v[i][1], v[i][0]))
    assert best[0] not in (order[0], order[-1])
    listed = [tuple(p) for p in models["comb"].tolist()]
    assert listed.index((8, 1, 0)) not in (0, len(listed) - 1)
    # its twin: three teeth achieve the same minimum
    _, free, v = R.per_voxel(scenes["plate"], R.ORIGIN, models["comb"], R.at(R.COMB_TIE_AT), 3, 100)
    assert min(free) == 3 and sorted(tuple(v[i]) for i in range(len(v)) if free[i] == 3) == [(4, 1, 0), (8, 1, 0), (12, 1, 0)]
    # the cup: the one overlapping voxel has a filled predecessor in its brick, and the travel is 0 although the voxels of the leading
    # face (the floor) are free; the twin overlaps only where there is no predecessor and travels
    for tag, local, want_pred, want in (("cup", R.CUP_AT, True, (1, 0, 1)), ("twin", (R.CUP_AT[0], R.CUP_AT[1], R.CUP_AT[2] + 8), False, (1, 19, 1))):
        place = R.at(local)
        overlaps, free, v = R.per_voxel(scenes["plate"], R.ORIGIN, models["cup"], place, 3, 100)
        pred = R.in_brick_predecessor(models["cup"], place, 3)
        assert int(overlaps.sum()) == 1 and bool(pred[overlaps][0]) == want_pred, tag
        assert R.sweep(scenes["plate"], R.ORIGIN, models["cup"], place, 3, 100) == want, tag
        floor = [i for i in range(len(v)) if v[i][1] == 0]
        assert all(free[i] == 19 for i in floor), tag
    # the long bar: a tree of three levels or more
    assert R.model_levels(models["bar"]) >= 3 and R.model_levels(models["one voxel"]) == 1
    # the 48 orientations x 6 directions give at least 12 distinct results
    results = {w for (tag, *_), w in zip(R.cases()["thinned"], R.expected("thinned")) if tag.startswith("small ")}
    assert len(results) >= 12, len(results)
    assert len({w[1] for w in results}) >= 8
    # the obstacle runs meet bit 0 and bit 3 of a brick behind 4-, 16- and 64-voxel boundaries on x and y, 4 and 16 on z
    seen = {(axis, c % 4, next(b for b in (64, 16, 4) if (c // b) != (start[axis] // b))) for axis, _, start, c in R.obstacle_runs()}
    for axis in range(3):
        for bit in (0, 3):
            for boundary in (4, 16, 64) if axis < 2 else (4, 16):
                assert (axis, bit, boundary) in seen, (axis, bit, boundary)
    for (tag, _, _, _, max_distance, _), w in zip(R.cases()["runs"], R.expected("runs")):
        if max_distance == 100:
            assert w[0] == 0 and w[2] == 1, tag                # (the run's own obstacle stops it, nothing else does: see the next lines)
    for (axis, step, start, c) in R.obstacle_runs():
        w = R.sweep(R.scenes()["runs"], R.ORIGIN, ONE, R.at(start), 2 * axis + (step < 0), 100)
        assert w == (0, abs(c - start[axis]) - 1, 1), (axis, step, c)


def test_the_host_functions_error_table():
    lib = _ffi.host_lib()
    d = np.zeros((4, 4, 4), dtype=np.float32)
    xyz = np.zeros((1, 3), dtype=np.int32)
    o = (C.c_int32 * 3)(0, 0, 0)
    good = ST.placement((1, 1, 1))

    def call(density=d, n=1, voxels=xyz, place=good, direction=3, flags=0, result=True, shape=(4, 4, 4)):
        out = np.full(1, 77, dtype=_ffi.SWEEP_RESULT)
        rc = lib.blok_sweep_voxels(None if density is None else _ffi.ptr(density), o, *shape, None if voxels is None else _ffi.ptr(voxels), n,
                                   None if place is None else _ffi.ptr(place), direction, 5, flags, _ffi.ptr(out) if result else None)
        return rc, (int(out["n_overlap"][0]), int(out["travel"][0]), int(out["blocked"][0]))

    assert call() == (0, (0, 5, 0))                            # an empty box: free for the whole distance
    bad_axis, bad_flip, bad_reserved = good.copy(), good.copy(), good.copy()
    bad_axis["axis"][0] = (0, 0, 2)
    bad_flip["flip"][0] = 8
    bad_reserved["reserved"][0] = (0, 1, 0)
    untouched = (77, 77, 77)
    for tag, kwargs in (("null placement", dict(place=None)), ("axis", dict(place=bad_axis)), ("flip", dict(place=bad_flip)),
                        ("reserved", dict(place=bad_reserved)), ("direction", dict(direction=6)), ("flag bits", dict(flags=2)),
                        ("flag bits high", dict(flags=0x80000001)), ("null list", dict(voxels=None)), ("null density", dict(density=None))):
        assert call(**kwargs) == (BLOK_ERR_INVALID_ARG, untouched), tag
    assert call(result=False)[0] == BLOK_ERR_INVALID_ARG
    assert call(shape=(2048, 2048, 2048)) == (BLOK_ERR_UNSUPPORTED, untouched)
    assert call(n=0, voxels=None, density=None) == (0, (0, 5, 0))          # an empty list: nothing overlaps, nothing stops
    with pytest.raises(BlokError) as e:
        SW.sweep_voxels_host(d, (0, 0, 0), xyz, good, 9, 5)
    assert e.value.status == BLOK_ERR_INVALID_ARG
