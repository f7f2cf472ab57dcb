"""CPU: the sweep in boxes whose extents are no multiples of 4, where the last brick along an axis is partial.  The host build
(blok_sweep_voxels) against the numpy model (tests/sweep_reference.py) on every line box of 1 .. 13 cells from every start, and on the odd
box's shared cases the GPU tests use; hand-written numbers for a model that reaches the far wall; and, from the model alone, that the
cases do what they are for."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import stamp as ST
from blok_amd import sweep as SW
from tests import sweep_reference as R

FAR = R.FAR
ONE = np.zeros((1, 3), dtype=np.int32)
LINE_ORIGIN = (-5, -3, -2)


def host(d, origin, xyz, place, direction, max_distance, flags):
    got = SW.sweep_voxels_host(d, origin, xyz, ST.placement(*place), direction, max_distance, flags)
    return (int(got["n_overlap"]), int(got["travel"]), int(got["blocked"]))


def line(axis, n, filled=()):
    """A box n long along `axis` and one cell across, [z][y][x], with the cells `filled` along the axis."""
    shape = [1, 1, 1]
    shape[axis] = n
    d = np.zeros(tuple(shape[::-1]), dtype=np.float32)
    for c in filled:
        p = [0, 0, 0]
        p[axis] = c
        d[p[2], p[1], p[0]] = 1.0
    return d


def voxel_on_line(axis, c):
    p = [0, 0, 0]
    p[axis] = c
    return (tuple(LINE_ORIGIN[a] + p[a] for a in range(3)), (0, 1, 2), 0)


@pytest.mark.parametrize("direction", range(6))
def test_hand_written_far_walls(direction):
    """The contract's numbers spelled out: with the box solid, a voxel at p in a box n long takes n - 1 - p steps towards + and p towards
    -, whatever n is modulo 4."""
    axis, step = direction // 2, (-1 if direction & 1 else 1)
    for n, p, want in ((2, 0, 1), (1, 0, 0), (5, 0, 4), (6, 1, 4), (7, 3, 3), (9, 8, 0), (13, 2, 10), (97, 90, 6), (78, 70, 7), (61, 3, 57)):
        start, travel = (p, want) if step > 0 else (n - 1 - p, want)
        d = line(axis, n)
        assert R.sweep(d, LINE_ORIGIN, ONE, voxel_on_line(axis, start), direction, 200, R.BOX_IS_SOLID) == (0, travel, 1), (n, p)
        assert host(d, LINE_ORIGIN, ONE, voxel_on_line(axis, start), direction, 200, R.BOX_IS_SOLID) == (0, travel, 1), (n, p)
        assert host(d, LINE_ORIGIN, ONE, voxel_on_line(axis, start), direction, travel, R.BOX_IS_SOLID) == (0, travel, 0), (n, p)
        assert host(d, LINE_ORIGIN, ONE, voxel_on_line(axis, start), direction, 200, 0) == (0, 200, 0), (n, p)
    # one cell in front of a box of one cell: the voxel stands in the solid outside, steps into the box's one empty cell and meets the
    # wall behind it
    before = -1 if step > 0 else 1
    assert host(line(axis, 1), LINE_ORIGIN, ONE, voxel_on_line(axis, before), direction, 5, R.BOX_IS_SOLID) == (1, 1, 1)
    assert host(line(axis, 1), LINE_ORIGIN, ONE, voxel_on_line(axis, before), direction, 5, 0) == (0, 5, 0)
    # an obstacle in the last, partial brick: 5 cells, the obstacle in cell 4 (towards +) or cell 0 of a walk that entered through cell 4
    d = line(axis, 5, filled=(4,) if step > 0 else (0,))
    assert host(d, LINE_ORIGIN, ONE, voxel_on_line(axis, 1 if step > 0 else 7), direction, 50, R.BOX_IS_SOLID) == (0 if step > 0 else 1, 2 if step > 0 else 0, 1)
    assert host(d, LINE_ORIGIN, ONE, voxel_on_line(axis, 1 if step > 0 else 7), direction, 50, 0) == (0, 2 if step > 0 else 6, 1)


@pytest.mark.parametrize("axis", range(3))
def test_every_line_box_from_every_start(axis):
    """Boxes 1 .. 13 long, empty and with obstacles, starts from 6 cells in front to 5 behind, both directions, both settings of the
    flag, distances on both sides of every wall: the host build gives the model's answer."""
    rng = np.random.default_rng(5 + axis)
    total = walls = 0
    for n in range(1, 14):
        contents = [()]
        contents.append((n - 1,))
        contents.append(tuple(int(c) for c in np.nonzero(rng.random(n) < 0.3)[0]))
        for filled in contents:
            d = line(axis, n, filled)
            for p in range(-6, n + 6):
                place = voxel_on_line(axis, p)
                for direction in (2 * axis, 2 * axis + 1):
                    for flags in (0, R.BOX_IS_SOLID):
                        for max_distance in (0, 1, 3, 5, 30):
                            want = R.sweep(d, LINE_ORIGIN, ONE, place, direction, max_distance, flags)
                            assert host(d, LINE_ORIGIN, ONE, place, direction, max_distance, flags) == want, (n, filled, p, direction, flags, max_distance)
                            total += 1
                            walls += bool(flags and not filled and 0 <= p < n and want[2])
    assert total > 10000 and walls >= 182                      # at max_distance 30 alone: every start inside, both directions (2 x (1 + .. + 13))


def test_the_host_build_equals_the_model_on_every_odd_case():
    models = R.models()
    total = 0
    for scene, d in R.odd_scenes().items():
        want = R.odd_expected(scene)
        for (tag, name, place, direction, max_distance, flags), w in zip(R.odd_cases()[scene], want):
            assert host(d, R.ODD_ORIGIN, models[name], place, direction, max_distance, flags) == w, (scene, tag)
            total += 1
    assert total > 3000


def test_what_the_odd_cases_are_for():
    assert all(n % 4 for n in R.ODD_SHAPE)
    d = R.odd_scenes()["odd lines"]
    cases, want = R.odd_cases()["odd lines"], R.odd_expected("odd lines")
    # a voxel inside the box on a clear column, the box solid, any distance: it stops at the wall, n - 1 - p or p steps on; every axis and
    # direction, every position of the last partial brick and the brick before it
    reached = set()
    for (tag, name, place, direction, max_distance, flags), w in zip(cases, want):
        if not tag.startswith("wall ") or not flags or max_distance != FAR:
            continue
        axis, step = direction // 2, (-1 if direction & 1 else 1)
        n, p = R.ODD_SHAPE[axis], place[0][axis] - R.ODD_ORIGIN[axis]
        if 0 <= p < n:
            assert w == (0, n - 1 - p if step > 0 else p, 1), tag
            reached.add((direction, n - 1 - p if step > 0 else p))
        else:
            assert w == (1, n if 0 <= p + step < n else 0, 1), tag      # in the solid outside: stuck, unless the first step enters the box
    for direction in range(6):
        for k in range(6):
            assert (direction, k) in reached, (direction, k)
    # every obstacle lies in the last partial brick of its axis, in the full brick before it, or one brick further, and is met from inside
    # the box and by a walk that enters the box from behind its far end
    for axis, columns in R.ODD_OBSTACLES.items():
        last = (R.ODD_SHAPE[axis] - 1) // 4
        assert {c // 4 for _, c in columns} == {last, last - 1}
        assert any(c // 4 == last and c % 4 == 0 for _, c in columns)
        for across, c in columns:
            x, y, z = R.odd_cell(axis, across, c)
            assert d[z, y, x] > 0
            n = R.ODD_SHAPE[axis]
            assert R.sweep(d, R.ODD_ORIGIN, ONE, R.odd_at(R.odd_cell(axis, across, n - 10)), 2 * axis, FAR, R.BOX_IS_SOLID) == (0, c - (n - 10) - 1, 1)
            assert R.sweep(d, R.ODD_ORIGIN, ONE, R.odd_at(R.odd_cell(axis, across, n + 5)), 2 * axis + 1, FAR, 0) == (0, n + 5 - c - 1, 1)
    # the larger models come to rest against the far wall too, and the cup does so with voxels that do not scan
    walls = {(tag.split()[0], direction) for (tag, _, _, direction, _, flags), w in zip(cases, want)
             if tag.split()[0] in ("cube", "cup", "ell") and flags and w[0] == 0 and w[2] == 1 and w[1] > 0}
    for name in ("cube", "cup", "ell"):
        for direction in (0, 2, 4):
            assert (name, direction) in walls, (name, direction)
    # in the thinned scene the orientations disagree, and some travels end at a wall: blocked with the flag, free without it
    cases, want = R.odd_cases()["odd thinned"], R.odd_expected("odd thinned")
    by_tag = {tag: w for (tag, *_), w in zip(cases, want)}
    small = {tag: w for tag, w in by_tag.items() if tag.startswith("small ")}
    assert len(set(small.values())) >= 12
    at_wall = [tag for tag, w in small.items() if tag.endswith(" 1") and w[2] == 1 and by_tag[tag[:-1] + "0"][2] == 0]
    assert len(at_wall) >= 12, len(at_wall)
