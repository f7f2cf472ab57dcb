"""CPU: every case of tests/sun_map_cases.py can fail.  The GPU module (tests/test_sun_map_writers_gpu.py) holds the map behind each edit
against the reference; a case whose edit would leave a kept map valid anyway proves nothing about the writer's box or bit.  Here, with the
numpy references alone and a frame laid by bounds_reference.sun_frame over the tree's cube:

    fills            in at least 20 texels the new world's lower bound stands more than one voxel above the old world's UPPER bound — a
                     map kept as it was is too low there — and every such texel lies in the texel range of the box the case declares
                     (Verdict.reached's arithmetic, no margin): an edit outside its declared box would show here;
    clears           at least 50 cells go from filled to empty and none the other way;
    writes_nothing   the arrays stay byte-equal.

The counts are conditions on the inputs (a case that misses one is enlarged), not measurements of the product."""
from __future__ import annotations

import types

import numpy as np
import pytest

from tests import bounds_reference as B
from tests import sun_map_cases as SC
from tests.test_sun_map_gpu import CUBE, ORIGIN, TOP, Verdict

MIN_TEXELS, MIN_CLEARED = 20, 50


def frame_of(case):
    """(info, delta): the frame of the tree's cube; for a scroll, of a cube that holds the box before and after."""
    origin, edge = (tuple(c - 96 for c in ORIGIN), 256.0) if case.lattice_moves else (ORIGIN, float(CUBE[0]))
    info = B.sun_frame(origin, edge)
    return info, B.sun_delta(info, np.asarray(origin, dtype=np.float64), edge)


def reached(info, delta, box):
    """Verdict.reached for a frame that no product reported."""
    stub = types.SimpleNamespace(info=info, delta=delta, map=np.zeros((info["nv"], info["nu"])))
    return Verdict.reached(stub, *box)


@pytest.fixture(scope="module")
def outcomes():
    """Per case: the world before and after the reference's edit, once."""
    out = {}
    for case in SC.CASES:
        before = case.world()
        after = before.copy()
        case.on_model(after)
        out[case.name] = (before, after)
    return out


def test_the_table_holds_every_family_and_every_class():
    families = {f: [c for c in SC.CASES if c.family == f] for f in SC.FAMILIES}
    assert set(families) == {"apply_shapes", "stamp_affine", "stamp_models", "automaton", "terrain", "voxelize", "flood", "distance", "brush", "capture", "scroll"}
    assert {c.cls for c in SC.CASES} == {SC.FILLS, SC.CLEARS, SC.WRITES_NOTHING}
    for family in ("apply_shapes", "stamp_affine", "stamp_models", "automaton"):
        assert {SC.FILLS, SC.CLEARS} <= {c.cls for c in families[family]}, family
    assert {c.cls for c in families["terrain"]} == {SC.FILLS, SC.WRITES_NOTHING}
    assert len(families["brush"]) == 4 and {c.cls for c in families["brush"]} == {SC.FILLS, SC.CLEARS, SC.WRITES_NOTHING}
    assert all(c.box is None for c in families["scroll"]) and len(families["scroll"]) == 4


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_the_base_content_stays_below_top(case):
    w = case.world()
    tall = w.filled()[:, TOP:, :]
    assert not tall.any() or case.family == "brush", case                # (the brush that digs: at the corner of edit_brush, above TOP)
    corners = np.asarray(ORIGIN) + B.CORNERS * CUBE[0]
    if case.box is not None:                                              # the declared box lies in the volume and touches a face of it
        lo, hi = case.box
        assert all(ORIGIN[a] <= lo[a] < hi[a] <= ORIGIN[a] + CUBE[a] for a in range(3)), case.box
        assert any(lo[a] == corners[0][a] or hi[a] == corners[7][a] for a in range(3)), case.box


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.cls == SC.FILLS], ids=lambda c: c.name)
def test_a_kept_map_would_be_too_low_behind_a_filling_case(case, outcomes):
    before, after = outcomes[case.name]
    info, delta = frame_of(case)
    with np.errstate(invalid="ignore"):
        _, hi_before = B.sun_map_bounds(B.voxels_of(before.filled(), before.origin), info, delta)
        lo_after, _ = B.sun_map_bounds(B.voxels_of(after.filled(), after.origin), info, delta)
    too_low = lo_after > hi_before + 1.0
    held = too_low & (hi_before > -B.K_BEAM_NONE)                        # (the others held no bound at all before the edit)
    print(f"[sun map cases] {case.name}: {int(too_low.sum())} texels of {too_low.size} too low if the map were kept, {int(held.sum())} of them "
          f"held a bound, too low by up to {float((lo_after - hi_before)[held].max(initial=0.0)):.1f} voxels")
    assert int(too_low.sum()) >= MIN_TEXELS, (case, int(too_low.sum()))
    if case.box is not None:
        outside = too_low & ~reached(info, delta, case.box)
        assert not outside.any(), (case, "texels outside the declared box", int(outside.sum()))


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.cls == SC.CLEARS], ids=lambda c: c.name)
def test_a_clearing_case_clears_and_fills_nothing(case, outcomes):
    before, after = outcomes[case.name]
    born, died = SC.changed(before, after)
    assert born == 0 and died >= MIN_CLEARED, (case, born, died)
    lo, hi = case.box
    inside = np.zeros(before.d.shape, bool)
    inside[before.slices(lo, hi)] = True
    assert not ((before.filled() != after.filled()) & ~inside).any(), (case, "cells outside the declared box changed")


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.cls == SC.WRITES_NOTHING], ids=lambda c: c.name)
def test_a_case_that_writes_nothing_leaves_the_arrays(case, outcomes):
    before, after = outcomes[case.name]
    assert after.origin == before.origin and after.d.tobytes() == before.d.tobytes() and after.m.tobytes() == before.m.tobytes(), case


def test_the_shifted_table_is_the_same_table_elsewhere():
    """The tightening cycle of the GPU module runs the cases at two places of a larger box."""
    shift = (184, 84, 184)
    moved = {c.name: c for c in SC.table(shift)}
    for case in SC.CASES:
        if case.box is not None:
            assert moved[case.name].box == tuple(tuple(c + s for c, s in zip(corner, shift)) for corner in case.box), case
