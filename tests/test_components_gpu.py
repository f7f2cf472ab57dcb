"""GPU: blok_hip_volume_label_components and blok_hip_volume_capture_component against the numpy model of their contract
(tests/components_reference.py): the downloaded label array and record table byte for byte and the two counts, on shapes chosen where the
kernels can go wrong (tests/components_reference.py: cases, and tests/test_components_cpu.py, which pins what makes each of them hard);
captured components against blok_hip_model_create's models byte for byte; a cut piece traced as an instance against the uncut world.
Both brick layouts unless said.

Not covered: BLOK_ERR_UNSUPPORTED for a volume above 2^32 cells and for a region of 2^32 cells (the two arrays of such a volume alone are
32 GiB), and BLOK_ERR_OOM.
Boxes at the ends of the int16 lattice and boxes of 16384 cells on one axis are covered in tests/test_volume_limits_gpu.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import stamp as ST
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import components_reference as R
from tests.conftest import SEED
from tests.test_stamp_gpu import arrays_equal, face_rays, tree_equal
from tests.volume_tree_reference import DenseModel

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
ORIGIN, SHAPE = R.ORIGIN, R.SHAPE


def _tracer(w=64, h=64):
    from blok_amd.tracer import HipTracer
    return HipTracer(w, h).init()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def volume(t, keyed, d, m, origin=ORIGIN, shape=SHAPE):
    t.set_volume_layout(keyed)
    t.volume_create(origin, shape)
    t.volume_upload(d, m)


def snapshot_equals(t, labels, records, tag):
    """The snapshot's two arrays, fetched in two pieces each, are the reference's byte for byte."""
    n, k = len(labels), len(records)
    got = np.concatenate([t.volume_labels_download(0, n // 3), t.volume_labels_download(n // 3, n - n // 3)])
    assert got.tobytes() == labels.tobytes(), (tag, "labels", int((got != labels).sum()), n)
    rec = np.concatenate([t.volume_components_download(0, k // 2), t.volume_components_download(k // 2, k - k // 2)])
    assert rec.tobytes() == records.tobytes(), (tag, "records", k)


def labelled_equals(t, d, lo, hi, tag, expected=None, origin=ORIGIN):
    labels, records = expected if expected is not None else R.label(d, origin, lo, hi)
    got = t.volume_label_components(lo, hi)
    assert got == (len(records), int(records["n_voxels"].sum())), (tag, got)
    snapshot_equals(t, labels, records, tag)
    return labels, records


# ---- the label array and the records ------------------------------------------------------------------------------------------------

@LAYOUTS
def test_every_case_gives_the_reference_snapshot(keyed):
    """Brick, 16- and 64-voxel borders; regions off the brick grid, of one voxel, inside one brick, with bridges outside every side; the
    long paths; the combs; checkerboard, solid box, empty and never-filled volumes; the random fills."""
    t = _tracer()
    uploaded = None
    for name, (d, m, lo, hi) in R.cases().items():
        if uploaded is not d:
            volume(t, keyed, d, m)
            uploaded = d
        labelled_equals(t, d, lo, hi, name, R.expected(name))
    t.shutdown()


@LAYOUTS
def test_regions_off_the_brick_grid_of_a_24_13_9_volume(keyed):
    """6 x 4 x 3 bricks, ragged last bricks in y and z, three tree levels: a keyed brick's index is far from its row-major one.  No corner
    of the regions is a multiple of 4."""
    origin, shape = (-7, 3, -2), (24, 13, 9)
    rng = np.random.default_rng(31)
    d = np.where(rng.random(shape[::-1]) < 0.3, rng.uniform(0.1, 2.0, shape[::-1]), 0.0).astype(np.float32)
    d[::3, ::2, ::5] = -0.5
    m = np.where(d > 0, 7, 0).astype(np.uint32)
    t = _tracer()
    volume(t, keyed, d, m, origin, shape)
    _, records = labelled_equals(t, d, None, None, "whole", origin=origin)
    assert len(records) > 5
    for lo, hi in (((1, 1, 1), (22, 11, 7)), ((5, 2, 3), (19, 10, 6)), ((17, 1, 5), (23, 13, 9)), ((2, 6, 1), (3, 7, 2))):      # box-local
        assert all(c % 4 for c in lo + hi)
        labelled_equals(t, d, tuple(o + c for o, c in zip(origin, lo)), tuple(o + c for o, c in zip(origin, hi)), (lo, hi), origin=origin)
    t.shutdown()


@LAYOUTS
def test_a_snapshot_outlives_edits_until_the_next_labelling(keyed):
    """A pillar on a slab, severed by a SUBTRACT brush: the tables match the reference on the model's arrays both times, and the first
    snapshot downloads unchanged after the edit."""
    model = DenseModel(ORIGIN, SHAPE)
    model.density[0:6, :, :] = 1.0                              # [z][y][x]: a slab over the box's floor in z ... and
    model.density[:, 0:5, :] = 1.5                              # ... the floor in y, the side the `touches` rule speaks of
    model.density[20:27, 0:60, 30:37] = 2.0                     # the pillar, 7 x 60 x 7, standing on the y floor
    model.ids[model.density > 0] = 7
    model.density[40:44, 30:34, 70:74] = np.nan                 # and something that is not filled
    t = _tracer()
    volume(t, keyed, model.density, model.ids)
    labels, records = labelled_equals(t, model.density, None, None, "whole")
    assert len(records) == 1
    centre = (ORIGIN[0] + 33.5, ORIGIN[1] + 30.5, ORIGIN[2] + 23.5)
    model.brush(centre, 8.0, 0.0, 1)
    t.volume_apply_brush(centre, 8.0, 0.0, 1)
    arrays_equal(t, model.density, model.ids, "brushed")
    snapshot_equals(t, labels, records, "the first snapshot after the edit")
    _, after = labelled_equals(t, model.density, None, None, "severed")
    assert len(after) == 2 and int((after["touches"] & 8 == 0).sum()) == 1      # the top floats
    # a region again replaces the snapshot: its size is the region's
    lo, hi = R.world((29, 20, 18), (11, 45, 13))
    labelled_equals(t, model.density, lo, hi, "region")
    with pytest.raises(BlokError):
        t.volume_labels_download(0, 11 * 45 * 13 + 1)
    t.shutdown()


# ---- capture ------------------------------------------------------------------------------------------------------------------------

def component_equals_created(t, d, m, snapshot, rec, tag, cut=False):
    """The captured model is the model model_create builds from the reference's list over the CURRENT arrays: both arrays and the info
    block, and the origin is the record's lo."""
    xyz, mm, _ = R.members(d, m, ORIGIN, snapshot, rec)
    assert len(mm) > 0, tag
    got, origin = t.volume_capture_component(int(rec["label"]), cut=cut)
    assert origin == tuple(rec["lo"].tolist()), (tag, origin)
    assert t.last_capture_voxels == len(mm), (tag, t.last_capture_voxels, len(mm))
    want = t.model_create(xyz, mm)
    assert want == got + 1, tag
    gn, gm, gi = t.model_download(got)
    wn, wm, wi = t.model_download(want)
    assert gi == wi, (tag, gi, wi)
    assert gn.tobytes() == wn.tobytes(), (tag, "nodes", gn.shape, wn.shape)
    assert gm.tobytes() == wm.tobytes(), (tag, "materials")
    if cut:
        R.clear_members(d, m, ORIGIN, snapshot, rec)
    return got


@LAYOUTS
def test_captured_components_equal_created_models(keyed, mats):
    name = "random 0.3116"
    d0, m0, lo, hi = R.cases()[name]
    labels, records = R.expected(name)
    snapshot = (labels, lo, hi)
    d, m = d0.copy(), m0.copy()
    t = _tracer()
    volume(t, keyed, d, m)
    labelled_equals(t, d, lo, hi, name, (labels, records))
    order = np.argsort(records["n_voxels"])
    largest, second = records[order[-1]], records[order[-2]]
    singles = records[records["n_voxels"] == 1]
    single = singles[len(singles) // 2]
    corner = records[records["label"] == labels[0]][0]
    assert int(labels[0]) == 0 and int(corner["touches"]) & 0b101010 == 0b101010 and int(largest["n_voxels"]) > 500
    for tag, rec in (("largest", largest), ("one voxel", single), ("corner", corner)):
        component_equals_created(t, d, m, snapshot, rec, tag)
    arrays_equal(t, d, m, "capture reads only")
    # membership is judged against the volume as it is now: an erased member is left out, a voxel filled next to the piece is not taken
    ext = [hi[a] - lo[a] for a in range(3)]
    mine = np.nonzero(labels == largest["label"])[0]
    r = int(mine[len(mine) // 2])
    gone = (lo[0] + r % ext[0], lo[1] + (r // ext[0]) % ext[1], lo[2] + r // (ext[0] * ext[1]))
    region = labels.reshape(ext[2], ext[1], ext[0])
    free = np.nonzero((region == R.EMPTY)[:, :, 1:] & (region == largest["label"])[:, :, :-1])      # an empty cell right of a member
    added = (lo[0] + int(free[2][0]) + 1, lo[1] + int(free[1][0]), lo[2] + int(free[0][0]))
    for world, ident, dens in ((gone, 0, 0.0), (added, 33, 1.0)):
        x, y, z = (world[a] - ORIGIN[a] for a in range(3))
        d[z, y, x], m[z, y, x] = dens, ident
    t.volume_set_voxels(np.array([gone, added], dtype=np.int32), [0, 33], [0.0, 1.0])
    arrays_equal(t, d, m, "edited")
    assert len(R.members(d, m, ORIGIN, snapshot, largest)[1]) == int(largest["n_voxels"]) - 1
    component_equals_created(t, d, m, snapshot, largest, "largest, one erased, one added beside it")
    # CUT: the model as before, those voxels cleared and nothing else, the tree after a rebuild
    component_equals_created(t, d, m, snapshot, largest, "cut", cut=True)
    x, y, z = (added[a] - ORIGIN[a] for a in range(3))
    assert d[z, y, x] == 1.0
    arrays_equal(t, d, m, "cut")
    tree_equal(t, d, m, ORIGIN, mats, "cut")
    # the snapshot still serves the others; the cut one has nothing left: refused, no id consumed
    component_equals_created(t, d, m, snapshot, second, "another after the cut", cut=True)
    arrays_equal(t, d, m, "second cut")
    next_id = t.model_create(np.zeros((1, 3), dtype=np.int32), np.ones(1, dtype=np.uint32))
    with pytest.raises(BlokError) as e:
        t.volume_capture_component(int(largest["label"]), cut=True)
    assert e.value.status == BLOK_ERR_UNSUPPORTED and t.last_capture_voxels == 0
    arrays_equal(t, d, m, "refused")
    assert t.model_create(np.zeros((1, 3), dtype=np.int32), np.ones(1, dtype=np.uint32)) == next_id + 1
    tree_equal(t, d, m, ORIGIN, mats, "after all")
    t.shutdown()


@LAYOUTS
def test_cut_and_carry(keyed, mats):
    """A ragged column whose top a brush has severed: the floating piece, found by `touches`, is cut out and shown as an instance at
    out_origin; every ray sees the voxel, face and material it saw in the uncut world."""
    origin, shape = (-20, -18, -14), (48, 40, 32)
    model = DenseModel(origin, shape)
    rng = np.random.default_rng(SEED)
    model.density[:, 0:3, :] = 1.0                              # ground
    for y in range(3, 34):                                      # the column: a ragged disc per layer
        zz, xx = np.indices((32, 48))
        r = 4.0 + 2.0 * rng.random()
        model.density[:, y, :][(xx - 24 - rng.integers(-1, 2)) ** 2 + (zz - 16 - rng.integers(-1, 2)) ** 2 < r * r] = 1.0
    model.ids[model.density > 0] = 1
    model.ids[model.density > 0] += (rng.integers(0, 200, model.ids.shape)[model.density > 0]).astype(np.uint32)
    model.density[:, 20:23, :] = 0.0                            # severed: three empty layers
    model.ids[:, 20:23, :] = 0
    d0, m0 = model.density.copy(), model.ids.copy()
    t = _tracer()
    volume(t, keyed, d0, m0, origin, shape)
    labels, records = labelled_equals(t, d0, None, None, "column", origin=origin)
    floating = records[records["touches"] & 8 == 0]
    assert len(records) == 2 and len(floating) == 1 and int(floating[0]["n_voxels"]) > 500
    rays, voxels, faces = face_rays(d0, origin)
    local = voxels - np.asarray(origin)
    want_material = m0[local[:, 2], local[:, 1], local[:, 0]]
    on_piece = labels.reshape(d0.shape)[local[:, 2], local[:, 1], local[:, 0]] == floating[0]["label"]
    assert len(rays) >= 500 and int(on_piece.sum()) >= 100
    t.volume_rebuild(mats)
    uncut = t.trace_rays(rays)
    piece, at = t.volume_capture_component(int(floating[0]["label"]), cut=True)
    d, m = d0.copy(), m0.copy()
    R.clear_members(d, m, origin, (labels, None, None), floating[0])
    arrays_equal(t, d, m, "cut")
    tree_equal(t, d, m, origin, mats, "cut")
    carried, _ = t.trace_rays_instanced(rays, ST.placement(at, (0, 1, 2), 0, piece))
    for hits in (uncut, carried):
        assert (hits["hit"] == 1).all()
        assert (hits["voxel"].astype(np.int64) == voxels).all()
        assert (hits["face"] == faces).all()
        assert (hits["material_id"] == want_material).all()
    t.shutdown()


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_change_nothing():
    """Every line of the contract's error list but the two that need more than 16 GiB (a volume above 2^32 cells, a region of 2^32
    cells) and BLOK_ERR_OOM; after each the previous snapshot downloads as it was and the volume is unchanged."""
    lib = _ffi.hip_lib()
    t = _tracer()
    nc, nv, out, org = C.c_uint64(7), C.c_uint64(7), C.c_uint32(77), (C.c_int32 * 3)(9, 9, 9)
    buf = np.zeros(16, dtype=np.uint32)
    rec = np.zeros(2, dtype=_ffi.COMPONENT)
    # no volume, no snapshot
    assert lib.blok_hip_volume_label_components(t._ctx, None, None, 0, C.byref(nc), C.byref(nv)) == BLOK_ERR_NO_WORLD and (nc.value, nv.value) == (0, 0)
    assert lib.blok_hip_volume_capture_component(t._ctx, 0, 0, C.byref(out), org, C.byref(nv)) == BLOK_ERR_NO_WORLD
    assert lib.blok_hip_volume_labels_download(t._ctx, _ffi.ptr(buf), 0, 0) == BLOK_ERR_INVALID_ARG
    assert lib.blok_hip_volume_components_download(t._ctx, _ffi.ptr(rec), 0, 0) == BLOK_ERR_INVALID_ARG
    name = "ragged region"
    d, m, lo, hi = R.cases()[name]
    labels, records = R.expected(name)
    volume(t, True, d, m)
    nv.value = 7
    assert lib.blok_hip_volume_capture_component(t._ctx, 0, 0, C.byref(out), org, C.byref(nv)) == BLOK_ERR_INVALID_ARG      # a volume, but no snapshot
    assert (out.value, nv.value, tuple(org)) == (77, 0, (9, 9, 9))
    labelled_equals(t, d, lo, hi, name, (labels, records))
    first_id = t.model_create(np.zeros((1, 3), dtype=np.int32), np.ones(1, dtype=np.uint32))

    def unchanged(tag):
        snapshot_equals(t, labels, records, tag)
        arrays_equal(t, d, m, tag)

    lo3, hi3 = (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi)
    for tag, status, args in (("unknown flag", BLOK_ERR_INVALID_ARG, (lo3, hi3, 1)), ("lo alone", BLOK_ERR_INVALID_ARG, (lo3, None, 0)),
                              ("hi alone", BLOK_ERR_INVALID_ARG, (None, hi3, 0)), ("lo above hi", BLOK_ERR_INVALID_ARG, (hi3, lo3, 0)),
                              ("leaves the box below", BLOK_ERR_UNSUPPORTED, ((C.c_int32 * 3)(ORIGIN[0] - 1, lo[1], lo[2]), hi3, 0)),
                              ("leaves the box above", BLOK_ERR_UNSUPPORTED, (lo3, (C.c_int32 * 3)(hi[0], hi[1], ORIGIN[2] + SHAPE[2] + 1), 0))):
        nc.value = nv.value = 7
        assert lib.blok_hip_volume_label_components(t._ctx, *args, C.byref(nc), C.byref(nv)) == status, tag
        assert (nc.value, nv.value) == (0, 0), tag
        unchanged(tag)
    # downloads
    n, k = len(labels), len(records)
    for tag, fn, out_ptr, total in (("labels", lib.blok_hip_volume_labels_download, _ffi.ptr(buf), n), ("records", lib.blok_hip_volume_components_download, _ffi.ptr(rec), k)):
        assert fn(t._ctx, out_ptr, total, 1) == BLOK_ERR_INVALID_ARG, tag
        assert fn(t._ctx, out_ptr, total + 1, 0) == BLOK_ERR_INVALID_ARG, tag
        assert fn(t._ctx, out_ptr, 1, 2 ** 64 - 1) == BLOK_ERR_INVALID_ARG, tag
        assert fn(t._ctx, None, 0, 1) == BLOK_ERR_INVALID_ARG, tag
        assert fn(t._ctx, None, total, 0) == 0 and fn(t._ctx, None, 0, 0) == 0, tag
    # capture
    empty_cell = int(np.nonzero(labels == R.EMPTY)[0][0])
    member = int(np.nonzero((labels != R.EMPTY) & (labels != np.arange(n)))[0][0])      # a voxel of a component that is not its first
    label = int(records[np.argmax(records["n_voxels"])]["label"])
    for tag, args in (("unknown flag", (label, 2, C.byref(out))), ("null output", (label, 0, None)), ("an empty cell", (empty_cell, 0, C.byref(out))),
                      ("a member that is not the first", (member, 1, C.byref(out))), ("past the region", (n, 0, C.byref(out))),
                      ("the sentinel", (0xFFFFFFFF, 0, C.byref(out)))):
        nv.value = 7
        assert lib.blok_hip_volume_capture_component(t._ctx, *args, org, C.byref(nv)) == BLOK_ERR_INVALID_ARG, tag
        assert (out.value, nv.value, tuple(org)) == (77, 0, (9, 9, 9)), tag
        unchanged(tag)
    assert t.model_create(np.zeros((1, 3), dtype=np.int32), np.ones(1, dtype=np.uint32)) == first_id + 1      # no refused call took a model id
    # NULL origin and count pointers are allowed
    assert lib.blok_hip_volume_capture_component(t._ctx, label, 0, C.byref(out), None, None) == 0 and out.value == first_id + 2
    # an empty region, and a region without filled voxels: BLOK_OK, zero counts, an empty snapshot that replaces the previous one
    z, y, x = (int(v[0]) for v in np.nonzero(~(d > 0)))
    for rlo, rhi, cells in ((lo, (hi[0], lo[1], hi[2]), 0), (*R.world((x, y, z), (1, 1, 1)), 1)):
        assert t.volume_label_components(rlo, rhi) == (0, 0)
        assert len(t.volume_components_download(0, 0)) == 0
        assert t.volume_labels_download(0, cells).tolist() == [R.EMPTY] * cells
        assert lib.blok_hip_volume_labels_download(t._ctx, _ffi.ptr(buf), 0, cells + 1) == BLOK_ERR_INVALID_ARG
        assert lib.blok_hip_volume_components_download(t._ctx, _ffi.ptr(rec), 0, 1) == BLOK_ERR_INVALID_ARG
        assert lib.blok_hip_volume_capture_component(t._ctx, 0, 0, C.byref(out), org, C.byref(nv)) == BLOK_ERR_INVALID_ARG
    # the snapshot goes with the volume
    labelled_equals(t, d, lo, hi, name, (labels, records))
    t.volume_destroy()
    assert lib.blok_hip_volume_labels_download(t._ctx, _ffi.ptr(buf), 0, 1) == BLOK_ERR_INVALID_ARG
    volume(t, False, d, m)
    labelled_equals(t, d, lo, hi, name, (labels, records))
    t.volume_create(ORIGIN, SHAPE)
    assert lib.blok_hip_volume_components_download(t._ctx, _ffi.ptr(rec), 0, 1) == BLOK_ERR_INVALID_ARG
    t.shutdown()
