"""GPU: blok_hip_volume_automaton against the numpy model of the contract (tests/automaton_reference.py, pinned to the host build in
tests/test_automaton_cpu.py) over the case table of tests/automaton_cases.py, in both brick layouts.  After every call: the whole download
bit for bit, the info and the per-step counts; the column field taken WITHOUT a rebuild — a reader of the masks where they lie — against
its reference; the rebuilt tree against volume_tree_reference, which is what shows a stale mask, occupancy word or dirty flag; and a
following set_voxels with its rebuild.  Then the error table with the download unchanged, and a held distance snapshot.

The kernel paths and the cases that take them (automaton_cases.py):
  wave seam of the decide kernel (a row of 68 bricks: lanes 0 .. 3 of a second wave) ........ every "long/..." case
  ragged last brick (z extent 41 and 33: cells past the box's end) ............................ "ragged/...", "high/..."; with "... solid" they count as filled
  outside-solid bricks (neighbour bricks beyond the grid are all ones) ........................ every "... solid" case
  no-voter birth (the vote's fallback id) ...................................................... "house/whole/births at 0", "... births at 0, solid"
  region cut inside a brick (the born and died words masked to the region's cells) ............ every ".../unaligned/..." case, "house/cell/...", "house/column/..."
  a wave of the births or deaths kernel that leaves at once (word 0) .......................... "house/column/...", "house/cell/...": most bricks of the region's rows
  the launch skipped when a step has no birth, or no death ..................................... "erode ...", "despeckle", "dilate ...", "fill pits x2"
  a brick whose 27 words are all ones, or all 0 (all counts at one end of the table) .......... every "slabs/..." case
  the early stop ................................................................................ "house/whole/despeckle x5", "house/whole/nothing happens"

Not covered: BLOK_ERR_UNSUPPORTED for a volume above 2^32 cells (its two arrays alone are 32 GiB), BLOK_ERR_OOM."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import automaton as A
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import automaton_cases as K
from tests import automaton_reference as R
from tests import columns_reference as CO
from tests import distance_reference as DR
from tests.conftest import SEED
from tests.volume_tree_reference import box_levels, reference_tree

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(64, 64).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def arrays_equal(t, d, m, tag):
    gd, gm = t.volume_download()
    assert gd.tobytes() == d.tobytes(), (tag, "density", int((gd.view(np.uint32) != d.view(np.uint32)).sum()))
    assert gm.tobytes() == m.tobytes(), (tag, "ids", int((gm != m).sum()))


def tree_equal(t, d, m, origin, mats, tag):
    """After a rebuild the tree is reference_tree of the expected arrays, byte for byte."""
    st = t.volume_rebuild(mats)
    filled = R.filled_of(d)
    if not filled.any():
        assert st.n_voxels == 0, tag
        return
    levels = box_levels(d.shape[::-1])
    ref_nodes, ref_mats = reference_tree(filled, m, levels)
    assert (st.n_voxels, st.n_tree_nodes, st.levels, tuple(st.origin)) == (len(ref_mats), len(ref_nodes), levels, tuple(origin)), tag
    nodes, ids = t.download_tree()
    assert nodes.tobytes() == ref_nodes.tobytes(), (tag, "nodes")
    assert ids.tobytes() == ref_mats.tobytes(), (tag, "materials")


def columns_equal(t, d, m, origin, tag):
    """The column field reads the masks as they lie: taken before any rebuild."""
    top, material, info = CO.field(d, m, origin)
    got = t.volume_column_field()
    assert got.tobytes() == info.tobytes(), (tag, got, info)
    assert t.volume_columns_download(0).tobytes() == top.tobytes() and t.volume_columns_download(1).tobytes() == material.tobytes(), tag


def begin(t, keyed, c):
    d0, m0 = K.content(c["shape"])
    t.set_volume_layout(keyed)
    t.volume_create(c["origin"], c["shape"])
    t.volume_upload(d0, m0)
    return d0, m0


# ---- device against reference ----------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("name", [c["name"] for c in K.table()])
def test_automaton_matches_the_model(tr, mats, keyed, name):
    c = next(c for c in K.table() if c["name"] == name)
    d, m, want_info, want_counts, _ = K.expected(c)
    begin(tr, keyed, c)
    info, counts = tr.volume_automaton(c["rule"], c["lo"], c["hi"])
    print(f"{name}: model {want_info} {want_counts.tolist()}, device {info} {counts.tolist()}")
    assert info.tobytes() == want_info.tobytes() and counts.tobytes() == want_counts.tobytes()
    arrays_equal(tr, d, m, name)
    columns_equal(tr, d, m, c["origin"], name)
    tree_equal(tr, d, m, c["origin"], mats, name)
    # a following edit and its rebuild: a voxel set in the first brick, one cleared in the last
    o, (nx, ny, nz) = c["origin"], c["shape"]
    d2, m2 = d.copy(), m.copy()
    d2[1, 1, 1], m2[1, 1, 1] = 1.5, 9
    d2[nz - 2, ny - 2, nx - 2], m2[nz - 2, ny - 2, nx - 2] = 0.0, 0
    tr.volume_set_voxels([(o[0] + 1, o[1] + 1, o[2] + 1), (o[0] + nx - 2, o[1] + ny - 2, o[2] + nz - 2)], [9, 0], [1.5, 0.0])
    arrays_equal(tr, d2, m2, name + " + set_voxels")
    tree_equal(tr, d2, m2, c["origin"], mats, name + " + set_voxels")


@LAYOUTS
def test_a_second_call_steps_what_the_first_left(tr, mats, keyed):
    """Two calls of one step are one call of two: the masks the first call's commit leaves are what the second call counts from."""
    c = next(c for c in K.table() if c["name"] == "house/unaligned/smooth x2")
    d, m, want_info, want_counts, _ = K.expected(c)
    begin(tr, keyed, c)
    one = A.smooth(1)
    for k in range(2):
        info, counts = tr.volume_automaton(one, c["lo"], c["hi"])
        assert counts.tobytes() == want_counts[k:k + 1].tobytes()
    assert int(info["n_filled"][0]) == int(want_info["n_filled"][0])
    arrays_equal(tr, d, m, "two calls")
    tree_equal(tr, d, m, c["origin"], mats, "two calls")


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_volume_untouched(mats):
    from blok_amd.tracer import HipTracer
    from tests.test_automaton_cpu import bad_rules
    t = HipTracer(64, 64).init()
    try:
        with pytest.raises(BlokError) as e:
            t.volume_automaton(A.smooth())
        assert e.value.status == BLOK_ERR_NO_WORLD
        origin, shape = K.BOXES["ragged"]
        d0, m0 = K.content(shape)
        t.volume_create(origin, shape)
        t.volume_upload(d0, m0)
        hi = tuple(origin[a] + shape[a] for a in range(3))
        table = [(r, {}, BLOK_ERR_INVALID_ARG) for _, r in bad_rules()]
        ok = A.smooth()
        table += [(ok, dict(lo=origin), BLOK_ERR_INVALID_ARG), (ok, dict(hi=hi), BLOK_ERR_INVALID_ARG),
                  (ok, dict(lo=(origin[0] + 2, origin[1], origin[2]), hi=(origin[0] + 1, hi[1], hi[2])), BLOK_ERR_INVALID_ARG),
                  (ok, dict(lo=(origin[0] - 1, origin[1], origin[2]), hi=hi), BLOK_ERR_UNSUPPORTED), (ok, dict(lo=origin, hi=(hi[0], hi[1], hi[2] + 1)), BLOK_ERR_UNSUPPORTED)]
        for r, kw, status in table:
            with pytest.raises(BlokError) as e:
                t.volume_automaton(r, **kw)
            assert e.value.status == status, (r, kw)
        assert t._lib.blok_hip_volume_automaton(t._ctx, None, None, None, None, None) == BLOK_ERR_INVALID_ARG      # a null rule
        arrays_equal(t, d0, m0, "after the refusals")
        tree_equal(t, d0, m0, origin, mats, "after the refusals")
        # null outputs are fine, and an empty region is a call that does nothing
        r = A.erode(6)
        assert t._lib.blok_hip_volume_automaton(t._ctx, None, None, _ffi.ptr(r), None, None) == 0
        d, m, _, _ = A.automaton_host(d0, m0, r, origin)
        arrays_equal(t, d, m, "null outputs")
        info, counts = t.volume_automaton(A.smooth(3), origin, (origin[0], hi[1], hi[2]))
        assert int(info["steps_run"][0]) == 0 and not counts.any() and int(info["n_filled"][0]) == 0 and [int(v) for v in info["ext"][0]] == [0, shape[1], shape[2]]
        arrays_equal(t, d, m, "empty region")
    finally:
        t.shutdown()


# ---- independence -------------------------------------------------------------------------------------------------------------------------------
def test_a_held_distance_snapshot_is_untouched():
    from blok_amd.tracer import HipTracer
    t = HipTracer(64, 64).init()
    try:
        origin, shape = K.BOXES["high"]
        d0, m0 = K.content(shape)
        t.volume_create(origin, shape)
        t.volume_upload(d0, m0)
        info = t.volume_distance_field(None, None, 3)
        held = t.volume_distance_download()
        want, want_info = DR.field(d0, origin, None, None, 3, 0)
        assert held.tobytes() == want.tobytes() and info.tobytes() == want_info.tobytes()
        t.volume_automaton(A.smooth(2))
        assert t.volume_distance_download().tobytes() == want.tobytes() and t.volume_distance_info().tobytes() == want_info.tobytes()
        # and the next field is of the stepped volume
        d, m, _, _ = A.automaton_host(d0, m0, A.smooth(2), origin)
        t.volume_distance_field(None, None, 3)
        assert t.volume_distance_download().tobytes() == DR.field(d, origin, None, None, 3, 0)[0].tobytes()
    finally:
        t.shutdown()
