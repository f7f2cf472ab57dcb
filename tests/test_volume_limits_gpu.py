"""GPU: every family of kernels on the resident volume — rebuild and edits, terrain, voxelize, quads, stamp and capture, components and
capture-component, sweep, the brick stream, the distance field and its edits — on the cases of tests/limit_cases.py: the families' own
scenes in boxes that touch the ends of the int16 lattice (LOW, HIGH, MIXED), and boxes of 16384 cells on one axis (7 tree levels, 256 mask
words to a row, runs, components, columns and distance rows across thousands of bricks).  Each family is checked the way its own GPU test
checks it, exactly, against the reference that tests/test_volume_limits_cpu.py pins the host build to on the same cases (and whose
hardness it asserts); after the edits, arrays and the rebuilt tree byte for byte (check() of tests/test_volume_rebuild_gpu.py, tree_equal
of tests/test_stamp_gpu.py).  Both brick layouts allowed and refused (a long box takes the general one either way).

Not covered: volumes above 2^30 cells and the refusals above 2^32 cells (see the families' own tests)."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import distance as D
from blok_amd import stamp as ST
from blok_amd import terrain as T
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import bricks_reference as BR
from tests import components_reference as CR
from tests import distance_reference as DR
from tests import limit_cases as LC
from tests import stamp_reference as SR
from tests import sweep_reference as SWR
from tests.conftest import SEED
from tests.terrain_cases import prior
from tests.test_bricks_gpu import encode_check, make, model_of
from tests.test_components_gpu import labelled_equals
from tests.test_distance_gpu import EDIT_REGIONS, edit_check, field_check
from tests.test_quads_gpu import _check as quads_check
from tests.test_stamp_gpu import Both, arrays_equal, captured_equals_created, tree_equal
from tests.test_sweep_gpu import as_tuples, ids_of
from tests.test_volume_rebuild_gpu import FH, FW, Pair, boundary_sequence, check, check_frames
from tests.test_voxelize_cpu import shim, shim_voxelize      # noqa: F401  (module fixture)
from tests.volume_tree_reference import DenseModel, OutsideBox

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
LIMIT = pytest.mark.parametrize("which", LC.LIMITS)
LONG = pytest.mark.parametrize("box", LC.LONG_BOXES, ids=LC.LONG_IDS)
LO, HI = LC.LATTICE_LO, LC.LATTICE_HI
MODES = (SR.SET, SR.KEEP, SR.ERASE)
_cache = {}


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(FW, FH).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def once(key, build):
    """What the reference gives for content that is never changed, computed once (the layouts share it)."""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def bits_equal(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def prior_with_empties(shape_xyz=LC.SHAPE):
    d0, m0 = prior(tuple(shape_xyz)[::-1])
    d0[::3, ::2, ::5] = -0.5
    d0[1::7, ::3, ::2] = np.nan
    return np.ascontiguousarray(d0), np.ascontiguousarray(m0)


def refused(status, call, *args, **kw):
    with pytest.raises(BlokError) as e:
        call(*args, **kw)
    assert e.value.status == status, (e.value, args, kw)
    return str(e.value)


# ---- rebuild and edits ------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@LIMIT
def test_boundary_sequence_and_frames_in_the_limit_boxes(tr, mats, keyed, which):
    """The brushes of the sequence end on faces at -32768 and 32768: the float arithmetic of voxel centres there."""
    p = Pair(tr, LC.limit_origin(which, LC.REBUILD_SHAPE), LC.REBUILD_SHAPE, keyed, mats)
    boundary_sequence(p)
    if which in LC.FRAME_FLOORS:
        check_frames(p, which, LC.FRAME_FLOORS[which])


@LAYOUTS
@LONG
def test_upload_set_voxels_and_brushes_in_the_long_boxes(tr, mats, keyed, box):
    p = Pair(tr, box.origin, box.shape, keyed, mats)
    p.check("created")
    p.upload(*LC.sparse_fill(box))
    p.check("sparse fill")
    ends = LC.end_voxels(box)
    p.set_voxels(ends, 200 + np.arange(len(ends)), np.linspace(0.25, 1.0, len(ends)).astype(np.float32))
    p.check("voxels at both ends")
    p.set_voxels(ends[:3], None, np.zeros(3, dtype=np.float32))
    p.check("three of them emptied")
    for centre, radius, value, mode, is_refused in LC.end_brushes(box):
        if is_refused:                                            # an edit outside the box: BLOK_ERR_UNSUPPORTED, nothing written
            with pytest.raises(OutsideBox):
                p.model.brush(centre, radius, value, mode)
            refused(BLOK_ERR_UNSUPPORTED, tr.volume_apply_brush, centre, radius, value, mode)
        else:
            p.brush(centre, radius, value, mode)
        p.check(("brush", centre, radius, mode))
    for beyond in (box.world(box.length, 0, 0), box.world(-1, 0, 0), box.world(0, box.nu, 0), box.world(0, 0, -1)):
        xyz = [box.world(0, 0, 0), beyond]
        with pytest.raises(OutsideBox):
            p.model.set_voxels(xyz, [1, 2], [1.0, 1.0])
        refused(BLOK_ERR_UNSUPPORTED, tr.volume_set_voxels, xyz, [1, 2], [1.0, 1.0])
    p.check("refused set_voxels")


# ---- terrain ----------------------------------------------------------------------------------------------------------------------------------
def terrain_check(t, p, origin, shape, lo, hi, d0, m0):
    """generate over [lo, hi) on top of (d0, m0) equals the host evaluation inside and the prior content outside; returns the arrays."""
    t.volume_upload(d0, m0)
    n = t.volume_generate_terrain(p, lo, hi)
    d, m = t.volume_download()
    lo = origin if lo is None else lo
    hi = LC.box_hi(origin, shape) if hi is None else hi
    sl = tuple(slice(lo[a] - origin[a], hi[a] - origin[a]) for a in (2, 1, 0))
    ed, em, en = T.eval_box(p, lo, hi, d0[sl], m0[sl])
    rd, rm = d0.copy(), m0.copy()
    rd[sl], rm[sl] = ed, em
    assert bits_equal(d, rd) and np.array_equal(m, rm) and n == en
    return rd, rm, n


@LAYOUTS
@LIMIT
def test_terrain_in_the_limit_boxes(tr, mats, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    tr.set_volume_layout(keyed)
    tr.volume_create(origin, LC.SHAPE)
    d0, m0 = prior(LC.SHAPE[::-1])
    zero = np.zeros_like(d0), np.zeros_like(m0)
    ragged = BR.scene_regions(origin)[1]
    for tag, p, kw in LC.limit_terrain_cases(origin):           # each pinned to the numpy reference in tests/test_volume_limits_cpu.py
        before = (d0, m0) if kw["flags"] & 4 else zero
        d, m, n = terrain_check(tr, p, origin, LC.SHAPE, None, None, *before)
        assert n > 10000 and (tag != "tall" or all(LC.faces_filled(d)))      # the tall one writes voxels on the +Y face too
        tree_equal(tr, d, m, origin, mats, (which, tag))
        terrain_check(tr, p, origin, LC.SHAPE, *ragged, d0, m0)


@LAYOUTS
@LONG
def test_terrain_in_the_long_boxes(tr, mats, keyed, box):
    tr.set_volume_layout(keyed)
    tr.volume_create(box.origin, box.shape)
    d0, m0 = LC.sparse_fill(box)
    zero = np.zeros_like(d0), np.zeros_like(m0)
    for flags in LC.LONG_TERRAIN_FLAGS:
        p, _ = LC.long_terrain_params(box, flags)
        d, m, n = terrain_check(tr, p, box.origin, box.shape, None, None, *((d0, m0) if flags & 4 else zero))
        assert n > 16384
        tree_equal(tr, d, m, box.origin, mats, (box.name, flags))
    lo, hi = LC.bricks_regions(box)[2]                            # a region off the brick grid on the long axis
    terrain_check(tr, p, box.origin, box.shape, lo, hi, d0, m0)


# ---- voxelize ---------------------------------------------------------------------------------------------------------------------------------
def voxelize_check(shim, t, pos, tri, origin, shape, solid, d0, m0, material=3, density=1.5):
    t.volume_upload(d0, m0)
    n = t.volume_voxelize_mesh(pos, tri, material=material, density=density, solid=solid)
    d, m = t.volume_download()
    rc, dr, mr, nr = shim_voxelize(shim, pos, tri, origin, shape, material=material, density=density, solid=solid, dens=d0, ids=m0)
    assert rc == 0 and bits_equal(d, dr) and np.array_equal(m, mr) and n == nr
    return d, m


@LAYOUTS
@LIMIT
def test_voxelize_a_mesh_with_faces_on_the_lattice_planes(shim, tr, mats, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    (pos, tri), _, _ = LC.limit_mesh(which)
    tr.set_volume_layout(keyed)
    tr.volume_create(origin, LC.SHAPE)
    d0, m0 = prior_with_empties()
    for solid in (False, True):
        d, m = voxelize_check(shim, tr, pos, tri, origin, LC.SHAPE, solid, d0, m0)
        assert int((d > 0).sum()) > int((d0 > 0).sum()) + 1000
        tree_equal(tr, d, m, origin, mats, (which, solid))


@LAYOUTS
@LONG
def test_voxelize_a_prism_along_the_long_boxes(shim, tr, mats, keyed, box):
    pos, tri, _ = LC.prism(box)
    tr.set_volume_layout(keyed)
    tr.volume_create(box.origin, box.shape)
    zero = box.zeros(np.float32), box.zeros(np.uint32)
    for solid in (False, True):
        d, m = voxelize_check(shim, tr, pos, tri, box.origin, box.shape, solid, *zero)
        want = LC.prism_expected(box, solid)
        assert np.array_equal(d, np.where(want, np.float32(1.5), np.float32(0))) and np.array_equal(m, np.where(want, 3, 0))
        tree_equal(tr, d, m, box.origin, mats, (box.name, solid))
    d, m = voxelize_check(shim, tr, pos, tri, box.origin, box.shape, True, *LC.sparse_fill(box))      # over content
    tree_equal(tr, d, m, box.origin, mats, (box.name, "over content"))


# ---- quads ------------------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@LIMIT
def test_quads_in_the_limit_boxes(tr, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    vol = make(tr, keyed, origin, LC.SHAPE, *prior_with_empties())
    regions = BR.scene_regions(origin)                            # the ragged regions of tests/test_quads_gpu.py, moved with the box
    for ignore in (False, True):
        for lo, hi in regions:
            quads_check(tr, origin, lo, hi, ignore, vol)
    p, _ = LC.terrain_params(origin[1], 4)                        # a denser field whose runs and stacks do merge
    tr.volume_generate_terrain(p)
    vol = tr.volume_download()
    for lo, hi in regions[:2]:
        q = quads_check(tr, origin, lo, hi, False, vol)
    assert len(q) > 1000


@LAYOUTS
@LONG
def test_quads_in_the_long_boxes(tr, keyed, box):
    n = box.length
    vol = make(tr, keyed, box.origin, box.shape, *LC.quads_fill(box, "slab"))
    q = quads_check(tr, box.origin, volume=vol)
    assert len(q) == 6 and sorted(max(int(r["du"]), int(r["dv"])) for r in q)[2:] == [n] * 4
    lo, hi = LC.bricks_regions(box)[2]
    q = quads_check(tr, box.origin, lo, hi, True, vol)
    assert len(q) == 4 and all(max(int(r["du"]), int(r["dv"])) == n - 3 for r in q)      # the slab goes on beyond both ends of the region
    vol = make(tr, keyed, box.origin, box.shape, *LC.quads_fill(box, "seams"))
    for ignore in (False, True):
        q = quads_check(tr, box.origin, ignore=ignore, volume=vol)
        assert len(q) >= (4 * len(LC.SEAM_RUNS) if not ignore else 12)      # four side faces to a run; one material: three pieces of six faces
        quads_check(tr, box.origin, lo, hi, ignore, vol)
    vol = make(tr, keyed, box.origin, box.shape, *LC.sparse_fill(box))
    quads_check(tr, box.origin, volume=vol)
    assert len(tr.volume_quads_download(0, 100, page=7)) == 100


# ---- stamp and capture ------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@LIMIT
def test_stamps_flush_against_the_lattice_clipped_and_refused(tr, mats, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    xyz, mm = SR.small_model()
    b = Both(tr, keyed, origin, LC.SHAPE, *prior_with_empties(), [(xyz, mm)])
    written = 0
    for end in (1, -1):
        for k, place in enumerate(LC.stamp_flush(xyz, end)):
            written += b.stamp([(0, place)], MODES[k % 3], 0.5 + k % 4, ("flush", end, k))
        for k, place in enumerate(LC.stamp_beyond(xyz, end)):
            text = refused(BLOK_ERR_INVALID_ARG, tr.volume_stamp_models, ST.placement(*place, model=b.ids[0]), MODES[k % 3], 1.0)
            assert "world box outside" in text
            refused(BLOK_ERR_INVALID_ARG, tr.volume_sweep_models, ST.placement(*place, model=b.ids[0]), k % 6, 10)
        arrays_equal(tr, b.d, b.m, ("refused", end))
    for k, place in enumerate(LC.stamp_clipped(origin, LC.SHAPE)):
        written += b.stamp([(0, place)], MODES[k % 3], 2.0, ("clipped", k))
    for k, place in enumerate(LC.stamp_flush_in(xyz, origin, LC.SHAPE)):
        written += b.stamp([(0, place)], MODES[(k + 1) % 3], 0.75, ("flush in the box", k))
    table = [(0, p) for p in LC.stamp_flush(xyz, 1)[::5] + LC.stamp_flush(xyz, -1)[::7] + LC.stamp_clipped(origin, LC.SHAPE)[::9]]
    written += b.stamp(table, SR.SET, 1.25, "one table")
    assert written > 2000
    tree_equal(tr, b.d, b.m, origin, mats, which)
    tr.model_destroy(b.ids[0])


@LAYOUTS
@LIMIT
def test_capture_and_cut_in_the_limit_boxes(tr, mats, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    hi = LC.box_hi(origin, LC.SHAPE)
    d, m = prior_with_empties()
    make(tr, keyed, origin, LC.SHAPE, d, m)
    d, m = d.copy(), m.copy()
    corner_hi, corner_lo = (tuple(h - 21 for h in hi), hi), (origin, tuple(o + 19 for o in origin))
    for tag, (lo, rhi) in (("whole box", (None, None)), ("far corner", corner_hi), ("near corner", corner_lo), ("ragged", BR.scene_regions(origin)[1])):
        captured_equals_created(tr, d, m, origin, lo, rhi, tag)
    arrays_equal(tr, d, m, "capture reads only")
    for tag, (lo, rhi) in (("far corner", corner_hi), ("near corner", corner_lo)):
        captured_equals_created(tr, d, m, origin, lo, rhi, tag, cut=True)
        SR.cut(d, m, origin, lo, rhi)
        arrays_equal(tr, d, m, ("cut", tag))
    tree_equal(tr, d, m, origin, mats, "cut")


@LAYOUTS
@LONG
def test_stamp_capture_and_cut_in_the_long_boxes(tr, mats, keyed, box):
    """The whole-box capture of a 16384-cell box is a model of seven levels: model_create builds it from the same list (its extent is
    within 4^7), so the contract's first line applies — byte-identical, not the refusal."""
    xyz, mm = LC.rod_model()
    b = Both(tr, keyed, box.origin, box.shape, *LC.sparse_fill(box), [(xyz, mm)])
    places = LC.long_stamp_places(box)
    written = [b.stamp([(0, place)], MODES[k % 3], 1.5, (box.name, k)) for k, place in enumerate(places)]
    assert all(n > 0 for n in written[:3]) and sum(written) > 1000      # (a KEEP over an earlier SET of the same cells writes nothing)
    assert b.stamp([(0, p) for p in places], SR.SET, 0.75, "one table") > 1000
    tree_equal(tr, b.d, b.m, box.origin, mats, "stamped")
    got, info = captured_equals_created(tr, b.d, b.m, box.origin, None, None, "whole box")
    assert info["levels"] == 7
    lo, hi = LC.bricks_regions(box)[2]
    captured_equals_created(tr, b.d, b.m, box.origin, lo, hi, "off the brick grid", cut=True)
    SR.cut(b.d, b.m, box.origin, lo, hi)
    arrays_equal(tr, b.d, b.m, "cut")
    tree_equal(tr, b.d, b.m, box.origin, mats, "cut")
    refused(BLOK_ERR_UNSUPPORTED, tr.volume_capture_model, lo, hi)              # nothing left in it: refused, no id consumed
    assert tr.model_create(xyz[:1], mm[:1]) == got + 4


# ---- components -------------------------------------------------------------------------------------------------------------------------------
def component_equals_created(t, d, m, origin, snapshot, rec, tag, cut=False):
    """component_equals_created of tests/test_components_gpu.py for a box at `origin`."""
    xyz, mm, _ = CR.members(d, m, origin, snapshot, rec)
    assert len(mm) > 0, tag
    got, at = t.volume_capture_component(int(rec["label"]), cut=cut)
    assert at == tuple(rec["lo"].tolist()) and t.last_capture_voxels == len(mm), (tag, at, t.last_capture_voxels)
    want = t.model_create(xyz, mm)
    assert want == got + 1, tag
    gn, gm, gi = t.model_download(got)
    wn, wm, wi = t.model_download(want)
    assert gi == wi and gn.tobytes() == wn.tobytes() and gm.tobytes() == wm.tobytes(), (tag, gi, wi)
    if cut:
        CR.clear_members(d, m, origin, snapshot, rec)
    return gi


@LAYOUTS
@LIMIT
def test_components_in_the_limit_boxes(tr, mats, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    tr.set_volume_layout(keyed)
    tr.volume_create(origin, LC.SHAPE)
    uploaded = None
    for name, (d, m, lo, hi) in CR.cases(origin).items():
        if uploaded is not d:
            tr.volume_upload(d, m)
            uploaded = d
        labelled_equals(tr, d, lo, hi, name, once(("components", which, name), lambda: CR.expected(name, origin)), origin=origin)
    # capture-component and CUT: the largest piece of the whole box, and pieces whose bounds lie on the lattice's ends
    name = "whole box"
    d0, m0, lo, hi = CR.cases(origin)[name]
    labels, records = CR.expected(name, origin)
    d, m = d0.copy(), m0.copy()
    tr.volume_upload(d, m)
    labelled_equals(tr, d, lo, hi, name, (labels, records), origin=origin)
    largest = records[np.argmax(records["n_voxels"])]
    ends = LC.components_at_lattice_ends(records, origin, LC.SHAPE)      # one of several voxels on every face that is an end of the lattice
    assert [f for f, _ in ends] == {"LOW": [1, 3, 5], "HIGH": [0, 2, 4], "MIXED": [1, 2]}[which] and int(largest["n_voxels"]) > 500
    pieces = {int(rec["label"]): (("face", face), rec) for face, rec in ends}
    pieces.setdefault(int(largest["label"]), ("largest", largest))
    for cut in (False, True):
        for tag, rec in pieces.values():
            component_equals_created(tr, d, m, origin, (labels, lo, hi), rec, (tag, cut), cut)
            arrays_equal(tr, d, m, (tag, cut))
    tree_equal(tr, d, m, origin, mats, "cut")


@LAYOUTS
@LONG
def test_components_in_the_long_boxes(tr, mats, keyed, box):
    d0, m0 = LC.components_fill(box)
    make(tr, keyed, box.origin, box.shape, d0, m0)
    d, m = d0.copy(), m0.copy()
    labels, records = once(("components", box.name), lambda: LC.components_expected(box))
    labelled_equals(tr, d, None, None, box.name, (labels, records), origin=box.origin)
    whole = records[records["label"] == box.index(0, *LC.BAR_AT)][0]
    info = component_equals_created(tr, d, m, box.origin, (labels, None, None), whole, "the whole bar")
    assert info["levels"] == 7 and int(whole["n_voxels"]) == box.length
    longest = records[records["label"] != whole["label"]]
    longest = longest[np.argmax(longest["n_voxels"])]
    component_equals_created(tr, d, m, box.origin, (labels, None, None), longest, "the longest piece, cut", cut=True)
    component_equals_created(tr, d, m, box.origin, (labels, None, None), whole, "the whole bar, cut", cut=True)
    arrays_equal(tr, d, m, "cut")
    tree_equal(tr, d, m, box.origin, mats, "cut")
    assert tr.volume_label_components() == (len(records) - 2, int(records["n_voxels"].sum()) - box.length - int(longest["n_voxels"]))
    # a region off the brick grid on the long axis: the reference's own labelling where it is fast (no piece of it is longer than 70 cells)
    lo, hi = list(box.origin), list(box.hi)
    lo[box.axis], hi[box.axis] = box.origin[box.axis] + 1, box.origin[box.axis] + 70
    labelled_equals(tr, d0, tuple(lo), tuple(hi), "the near end", once(("components", box.name, "near"), lambda: CR.label(d, box.origin, tuple(lo), tuple(hi))), origin=box.origin)


# ---- sweep ------------------------------------------------------------------------------------------------------------------------------------
def sweeps_equal(t, cases, want, ids, tag):
    """One call per case, then the same cases as one table per (direction, max_distance, flags): both equal the reference."""
    groups = {}
    for i, case in enumerate(cases):
        _, name, place, direction, max_distance, flags = case[:6]
        got = as_tuples(t.volume_sweep_models(ST.placement(*place, model=ids[name]), direction, max_distance, flags))
        assert got == [want[i]], (tag, case[0], got, want[i])
        groups.setdefault((direction, max_distance, flags), []).append(i)
    for (direction, max_distance, flags), members in groups.items():
        table = np.concatenate([ST.placement(*cases[i][2], model=ids[cases[i][1]]) for i in members])
        got = as_tuples(t.volume_sweep_models(table, direction, max_distance, flags))
        assert got == [want[i] for i in members], (tag, direction, max_distance, flags)


@pytest.fixture(scope="module")
def sweep_models(tr):
    return {name: tr.model_create(xyz, np.arange(1, len(xyz) + 1, dtype=np.uint32)) for name, xyz in SWR.models().items()}


@LAYOUTS
@LIMIT
def test_sweeps_in_the_limit_boxes(tr, sweep_models, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    for scene, d in SWR.scenes().items():
        m = ids_of(d)
        make(tr, keyed, origin, LC.SHAPE, d, m)
        sweeps_equal(tr, SWR.cases(origin)[scene], SWR.expected(scene, origin), sweep_models, (which, scene))
        arrays_equal(tr, d, m, scene)


@LAYOUTS
@LONG
def test_sweeps_in_the_long_boxes(tr, sweep_models, keyed, box):
    d = LC.sweep_fill(box)
    m = ids_of(d)
    make(tr, keyed, box.origin, box.shape, d, m)
    cases = LC.sweep_cases(box)
    sweeps_equal(tr, cases, [c[6] for c in cases], sweep_models, box.name)
    # larger models along the long axis, against the reference's own sweep: the bar (70 cells, three levels) and the cube
    more = []
    a = box.axis
    for name, t0 in (("bar", 20), ("cube", 7), ("bar", box.length - 100)):
        for direction in (2 * a, 2 * a + 1):
            for max_distance, flags in ((LC.FAR, 0), (LC.FAR, SWR.BOX_IS_SOLID), (16300, 0)):
                place = (box.world(t0, *LC.OBSTACLE_AT), (a, box.u_axis, box.v_axis), 0)
                more.append((f"{name} {t0} {direction} {max_distance} {flags}", name, place, direction, max_distance, flags))
    want = once(("sweep", box.name), lambda: [SWR.sweep(d, box.origin, SWR.models()[c[1]], *c[2:6]) for c in more])
    assert any(w[1] > 16000 and w[2] == 1 for w in want)
    sweeps_equal(tr, more, want, sweep_models, box.name)
    arrays_equal(tr, d, m, box.name)


# ---- the brick stream -------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@LIMIT
def test_bricks_in_the_limit_boxes(tr, mats, keyed, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    d0, m0 = BR.scene(origin)
    vol = make(tr, keyed, origin, LC.SHAPE, d0, m0)
    for flags in (0, BR.FILLED_ONLY):
        for lo, hi in BR.scene_regions(origin) + BR.scene_aligned(origin)[1:]:
            encode_check(tr, vol, origin, lo, hi, flags, key=("limit scene", which))
    # undo, then a copy from one end of the box to the other, both ways of writing
    lo, hi = BR.scene_regions(origin)[1]
    s = encode_check(tr, vol, origin, lo, hi, 0, key=("limit scene", which))
    tr.volume_apply_brush(tuple(float(c) + 9.5 for c in lo), 9.0, 2.0, 0)
    tr.volume_restore_bricks()
    check(tr, model_of(origin, LC.SHAPE, d0, m0), "undo", mats)
    far = tuple(origin[a] + LC.SHAPE[a] - (hi[a] - lo[a]) for a in range(3))
    for dst, keep in ((far, False), (origin, True)):
        now = tr.volume_download()
        want = BR.decode(now[0], now[1], origin, s, dst, BR.KEEP_OTHERS if keep else 0)
        tr.volume_restore_bricks(dst, keep)
        check(tr, model_of(origin, LC.SHAPE, *want), (dst, keep), mats)
    refused(BLOK_ERR_UNSUPPORTED, tr.volume_restore_bricks, tuple(c + 1 for c in far))      # one cell beyond the box, and at HIGH beyond the lattice


@LAYOUTS
@LONG
def test_bricks_in_the_long_boxes(tr, mats, keyed, box):
    d0, m0 = LC.bricks_fill(box)
    vol = make(tr, keyed, box.origin, box.shape, d0, m0)
    regions = LC.bricks_regions(box)
    for flags in (0, BR.FILLED_ONLY):
        for lo, hi in regions:
            s = encode_check(tr, vol, box.origin, lo, hi, flags, key=("long", box.name))
            assert len(s[1]) >= 4096
    # the last stream (off the brick grid at both ends, filled cells only) written one cell further, then the whole box undone
    whole = encode_check(tr, vol, box.origin, None, None, 0, key=("long", box.name))
    tr.volume_decode_bricks(*s, dst_lo=box.origin, keep_others=True)
    want = BR.decode(d0, m0, box.origin, s, box.origin, BR.KEEP_OTHERS)
    check(tr, model_of(box.origin, box.shape, *want), "moved by a cell", mats)
    tr.volume_restore_bricks()
    check(tr, model_of(box.origin, box.shape, d0, m0), "undo", mats)
    assert BR.same_stream(tr.volume_bricks_download(), whole)


# ---- the distance field and its edits -----------------------------------------------------------------------------------------------------------
@LAYOUTS
@LIMIT
def test_distance_fields_and_edits_in_the_limit_boxes(tr, mats, keyed, which):
    origin = LC.limit_origin(which, LC.DISTANCE_SHAPE)
    d, m = LC.distance_scene()
    make(tr, keyed, origin, LC.DISTANCE_SHAPE, d, m)
    for lo, hi, radius, flags in DR.scene_cases(origin):
        want = once(("distance", which, lo, hi, radius, flags), lambda: DR.field(d, origin, lo, hi, radius, flags))
        field_check(tr, want, lo, hi, radius, flags, pieces=lo is not None and flags == 0)
    model = DenseModel(origin, LC.DISTANCE_SHAPE)
    model.upload(d, m)
    regions = DR.moved(EDIT_REGIONS, origin)
    total = 0
    for i, (op, d2) in enumerate(((D.GROW, 9), (D.SHRINK, 2), (D.HOLLOW, 3), (D.GROW, 16), (D.HOLLOW, 1), (D.SHRINK, 9))):
        lo, hi = regions[i % len(regions)]
        total += edit_check(tr, model, mats, f"{which} op {op} d2 {d2} region {lo}..{hi}", lo, hi, op, d2, 0.75, 6)
    assert total > 0


def long_field_check(t, want, box, lo, hi, radius, flags):
    """field_check without its 7-cell pages (a long box has 2^21 cells), then the download in three uneven pieces."""
    l = (0, 0, 0) if lo is None else tuple(lo[a] - box.origin[a] for a in range(3))
    got = field_check(t, (want, DR.make_info(box.origin, l, want.shape[::-1], radius, flags, want)), lo, hi, radius, flags, pieces=False)
    n = got.size
    pieces = [t.volume_distance_download(0, n // 3, page=100003), t.volume_distance_download(n // 3, 5), t.volume_distance_download(n // 3 + 5, n - n // 3 - 5)]
    assert np.concatenate(pieces).tobytes() == want.tobytes()
    return got


@LAYOUTS
@LONG
def test_distance_fields_in_the_long_boxes(tr, mats, keyed, box):
    sources = LC.distance_sources(box)
    d, m = DR.volume_with(box.shape, sources)
    make(tr, keyed, box.origin, box.shape, d, m)
    for radius in (255, 64):
        want = once(("distance", box.name, radius), lambda: DR.from_sources(box.shape, sources, radius))
        got = long_field_check(tr, want, box, None, None, radius, 0)
        if radius == 255:
            assert (got == 65025).any() and (got == DR.FAR).any()
    lo, hi = LC.bricks_regions(box)[2]
    l = tuple(lo[a] - box.origin[a] for a in range(3))
    whole = _cache[("distance", box.name, 255)]
    cut = np.ascontiguousarray(whole[l[2]:hi[2] - box.origin[2], l[1]:hi[1] - box.origin[1], l[0]:hi[0] - box.origin[0]])
    long_field_check(tr, cut, box, lo, hi, 255, 0)
    # GROW by the closed form's field: balls around the sources, cut by the box
    model = DenseModel(box.origin, box.shape)
    model.upload(d, m)
    want = DR.from_sources(box.shape, sources, 3)
    info = DR.make_info(box.origin, (0, 0, 0), box.shape, 3, 0, want)
    field_check(tr, (want, info), None, None, 3, 0, pieces=False)
    n = tr.volume_edit_by_distance(D.GROW, 9, 1.25, 6)
    assert n == DR.edit(model.density, model.ids, want, info, DR.GROW, 9, 1.25, 6, origin=box.origin) > 100
    check(tr, model, "grown", mats)


@LAYOUTS
@LONG
def test_shrink_and_hollow_a_rod_along_the_long_boxes(tr, mats, keyed, box):
    d, m = LC.rod_fill(box)
    make(tr, keyed, box.origin, box.shape, d, m)
    for flags in (DR.TO_EMPTY, DR.TO_EMPTY | DR.BOX_IS_SOLID):
        want = once(("rod", box.name, flags), lambda: DR.field(d, box.origin, None, None, 2, flags))
        field_check(tr, want, None, None, 2, flags, pieces=False)
    model = DenseModel(box.origin, box.shape)
    model.upload(d, m)
    lo, hi = LC.bricks_regions(box)[2]
    assert edit_check(tr, model, mats, "hollow", lo, hi, D.HOLLOW, 1, radius=2) >= box.length - 16      # the rod's middle line goes
    assert edit_check(tr, model, mats, "grow", lo, hi, D.GROW, 2, 0.5, 9, radius=2) > 8 * (box.length - 16)        # the line comes back, and a skin around the rod
    assert edit_check(tr, model, mats, "shrink", None, None, D.SHRINK, 1, radius=1) > 8 * (box.length - 16)


# ---- error lines at the limits ----------------------------------------------------------------------------------------------------------------
@LAYOUTS
@LIMIT
def test_regions_and_placements_one_cell_beyond_the_lattice_are_refused(tr, keyed, which):
    """A region that leaves the box — here also the lattice — is BLOK_ERR_UNSUPPORTED, a placement whose world box leaves the lattice
    BLOK_ERR_INVALID_ARG; the volume and the four snapshots stay as they were."""
    origin = LC.limit_origin(which, LC.SHAPE)
    hi = LC.box_hi(origin, LC.SHAPE)
    d, m = prior_with_empties()
    make(tr, keyed, origin, LC.SHAPE, d, m)
    inner_lo, inner_hi = tuple(o + 3 for o in origin), tuple(h - 3 for h in hi)
    quads = tr.volume_extract_quads(inner_lo, inner_hi)
    n_components = tr.volume_label_components(inner_lo, inner_hi)[0]
    components = tr.volume_components_download(0, n_components)
    tr.volume_encode_bricks(inner_lo, inner_hi)
    bricks = tr.volume_bricks_download()
    tr.volume_distance_field(inner_lo, inner_hi, 4)
    dist, dist_info = tr.volume_distance_download(), tr.volume_distance_info()
    xyz, mm = SR.small_model()
    model = tr.model_create(xyz, mm)
    p, _ = LC.terrain_params(origin[1], 0)
    beyond = []                                                   # (lo, hi) one cell beyond each end of the lattice that the box touches
    for a in range(3):
        if origin[a] == LO:
            beyond.append((tuple(LO - 1 if k == a else origin[k] for k in range(3)), inner_hi))
        if hi[a] == HI:
            beyond.append((inner_lo, tuple(HI + 1 if k == a else hi[k] for k in range(3))))
    assert len(beyond) == (2 if which == "MIXED" else 3)
    places = [pl for end in (1, -1) for pl in LC.stamp_beyond(xyz, end)[::7]]

    def unchanged(tag):
        arrays_equal(tr, d, m, tag)
        assert tr.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes(), tag
        assert tr.volume_components_download(0, n_components).tobytes() == components.tobytes(), tag
        assert BR.same_stream(tr.volume_bricks_download(), bricks), tag
        assert tr.volume_distance_download().tobytes() == dist.tobytes() and tr.volume_distance_info().tobytes() == dist_info.tobytes(), tag

    for lo, rhi in beyond:
        for call, args in ((tr.volume_extract_quads, (lo, rhi)), (tr.volume_label_components, (lo, rhi)), (tr.volume_encode_bricks, (lo, rhi)),
                           (tr.volume_distance_field, (lo, rhi, 4)), (tr.volume_capture_model, (lo, rhi)), (tr.volume_capture_model, (lo, rhi, True)),
                           (tr.volume_generate_terrain, (p, lo, rhi))):
            refused(BLOK_ERR_UNSUPPORTED, call, *args)
        refused(BLOK_ERR_UNSUPPORTED, tr.volume_set_voxels, [inner_lo, lo, tuple(c - 1 for c in rhi)], [1, 2, 3], [1.0, 1.0, 1.0])
        centre = tuple((lo[a] + 2.5) if lo[a] < origin[a] else (rhi[a] - 2.5) if rhi[a] > hi[a] else origin[a] + 10.5 for a in range(3))
        refused(BLOK_ERR_UNSUPPORTED, tr.volume_apply_brush, centre, 2.49, 1.0, 0)      # a brush whose box ends one cell beyond the lattice
        unchanged((lo, rhi))
    for k, place in enumerate(places):
        inst = ST.placement(*place, model=model)
        assert "world box outside" in refused(BLOK_ERR_INVALID_ARG, tr.volume_stamp_models, inst, MODES[k % 3], 1.0)
        assert "world box outside" in refused(BLOK_ERR_INVALID_ARG, tr.volume_sweep_models, inst, k % 6, LC.FAR)
        assert "world box outside" in refused(BLOK_ERR_INVALID_ARG, tr.check_instances, inst)
    unchanged("placements")
    assert tr.model_create(xyz, mm) == model + 1                   # no refused capture took a model id
    tr.model_destroy(model)
