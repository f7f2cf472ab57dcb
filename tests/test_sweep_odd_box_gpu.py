"""GPU: blok_hip_volume_sweep_models in volumes whose extents are no multiples of 4, where the last brick along an axis is partial,
against the numpy model of the contract (tests/sweep_reference.py).  Both brick layouts.  tests/test_sweep_odd_box_cpu.py pins the host
build on the same cases and asserts what they are for: models that reach the far wall in all six directions with and without
BLOK_SWEEP_BOX_IS_SOLID, obstacles in the last partial brick, walks that enter the box through it."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import stamp as ST
from tests import sweep_reference as R

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
ONE = np.zeros((1, 3), dtype=np.int32)


def _tracer(w=64, h=64):
    from blok_amd.tracer import HipTracer
    return HipTracer(w, h).init()


def ids_of(d):
    return np.ascontiguousarray(np.where(R.filled_cells(d), 5, 0).astype(np.uint32))


def as_tuples(records):
    return [(int(r["n_overlap"]), int(r["travel"]), int(r["blocked"])) for r in records]


def volume(t, keyed, d, m, origin, shape):
    t.set_volume_layout(keyed)
    t.volume_create(origin, shape)
    t.volume_upload(d, m)


def unchanged(t, d, m, tag):
    gd, gm = t.volume_download()
    assert gd.tobytes() == d.tobytes() and gm.tobytes() == m.tobytes(), tag


@LAYOUTS
def test_every_odd_case_gives_the_reference_record(keyed):
    """The odd box's cases as one table per (direction, max_distance, flags), and the one-voxel and model cases against the walls singly
    too."""
    t = _tracer()
    ids = None
    for scene, d in R.odd_scenes().items():
        m = ids_of(d)
        volume(t, keyed, d, m, R.ODD_ORIGIN, R.ODD_SHAPE)
        ids = ids or {name: t.model_create(xyz, np.arange(1, len(xyz) + 1, dtype=np.uint32)) for name, xyz in R.models().items()}
        cases, want = R.odd_cases()[scene], R.odd_expected(scene)
        groups = {}
        for i, (tag, name, place, direction, max_distance, flags) in enumerate(cases):
            groups.setdefault((direction, max_distance, flags), []).append(i)
            if max_distance == R.FAR:
                got = as_tuples(t.volume_sweep_models(ST.placement(*place, model=ids[name]), direction, max_distance, flags))
                assert got == [want[i]], (scene, tag, got, want[i])
        for (direction, max_distance, flags), members in groups.items():
            table = np.concatenate([ST.placement(*cases[i][2], model=ids[cases[i][1]]) for i in members])
            got = as_tuples(t.volume_sweep_models(table, direction, max_distance, flags))
            wanted = [want[i] for i in members]
            assert got == wanted, (scene, direction, max_distance, flags, [(cases[members[j]][0], got[j], wanted[j]) for j in range(len(members)) if got[j] != wanted[j]][:5])
        unchanged(t, d, m, scene)
    t.shutdown()


@LAYOUTS
@pytest.mark.parametrize("shape", [(13, 6, 5), (1, 2, 3), (5, 9, 2)], ids=lambda s: "x".join(map(str, s)))
def test_small_boxes_from_every_start(keyed, shape):
    """Boxes of a few cells, one brick or a partial one along an axis: one voxel from every start on the box's middle lines, from 6 cells in
    front to 5 behind, both directions along every axis, both settings of the flag."""
    origin = (-5, -3, -2)
    rng = np.random.default_rng(sum(shape))
    d = np.where(rng.random(shape[::-1]) < 0.15, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    d[0, 0, 0] = np.nan
    m = ids_of(d)
    t = _tracer()
    volume(t, keyed, d, m, origin, shape)
    one = t.model_create(ONE, np.ones(1, dtype=np.uint32))
    starts = []
    for axis in range(3):
        for across in ((0, 0), (shape[(axis + 1) % 3] - 1, shape[(axis + 2) % 3] - 1)):
            for c in range(-6, shape[axis] + 6):
                p = [0, 0, 0]
                p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = c, across[0], across[1]
                starts.append((tuple(origin[a] + p[a] for a in range(3)), (0, 1, 2), 0))
    table = np.concatenate([ST.placement(*place, model=one) for place in starts])
    for direction in range(6):
        for flags in (0, R.BOX_IS_SOLID):
            for max_distance in (0, 1, 3, 30, R.FAR):
                want = [R.sweep(d, origin, ONE, place, direction, max_distance, flags) for place in starts]
                got = as_tuples(t.volume_sweep_models(table, direction, max_distance, flags))
                assert got == want, (direction, flags, max_distance, [(starts[i][0], got[i], want[i]) for i in range(len(starts)) if got[i] != want[i]][:5])
    unchanged(t, d, m, "small box")
    t.shutdown()
