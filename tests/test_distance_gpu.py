"""GPU: blok_hip_volume_distance_field / distance_info / distance_download / edit_by_distance against the numpy model of the contract
(tests/distance_reference.py, pinned in tests/test_distance_cpu.py) over volume_download(): values and info byte for byte, whole and in
pieces, in all four flag combinations and both brick layouts, on the shapes at which each pass can go wrong (test_distance_cpu.py asserts
from the model alone what makes them hard); the edits checked like check() of tests/test_volume_rebuild_gpu.py (arrays, then the rebuilt
tree) against a DenseModel that received the model's edit; the snapshot's life and independence; the error table.  Every comparison is
exact."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import distance as D
from blok_amd import stamp as S
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import distance_reference as R
from tests.conftest import SEED
from tests.test_volume_rebuild_gpu import check
from tests.volume_tree_reference import DenseModel

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
FAR = R.FAR


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def make(t, keyed, origin, shape, d=None, m=None):
    t.set_volume_layout(keyed)
    t.volume_create(origin, shape)
    if d is not None:
        t.volume_upload(d, m)
    vol = t.volume_download()
    if d is not None:
        assert vol[0].tobytes() == np.ascontiguousarray(d).tobytes() and vol[1].tobytes() == np.ascontiguousarray(m).tobytes()
    return vol


def counts(info):
    return [int(info[k][0]) for k in ("n_zero", "n_near", "n_far")]


def take(t, lo, hi, radius, flags):
    return t.volume_distance_field(lo, hi, radius, bool(flags & R.TO_EMPTY), bool(flags & R.BOX_IS_SOLID))


def field_check(t, want, lo, hi, radius, flags, pieces=True):
    """The device's field for the region equals `want` = (dist, info) of the reference; returns the downloaded values."""
    info = take(t, lo, hi, radius, flags)
    got = t.volume_distance_download()
    differ = int((got != want[0]).sum()) if got.shape == want[0].shape else -1
    print(f"region {lo}..{hi} R={radius} flags={flags}: reference {counts(want[1])}, device {counts(info)}, {differ} of {got.size} values differ")
    assert got.dtype == np.uint16 and got.shape == want[0].shape and got.tobytes() == want[0].tobytes()
    assert info.tobytes() == want[1].tobytes() == t.volume_distance_info().tobytes()
    if pieces and got.size:
        assert t.volume_distance_download(0, got.size, page=7).tobytes() == want[0].tobytes()
        assert t.volume_distance_download(got.size // 3, got.size - got.size // 3).tobytes() == want[0].ravel()[got.size // 3:].tobytes()
    return got


def cut(dist, lo, hi):
    return dist if lo is None else np.ascontiguousarray(dist[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])


# ---- the field ---------------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_field_of_the_noise_box_in_all_flag_combinations(tr, keyed):
    """13 x 10 x 7 at (-5, -3, -2): ragged last bricks on every axis; the whole box, regions off the brick grid, a one-cell region."""
    d, m = R.noise()
    vol = make(tr, keyed, R.NOISE_ORIGIN, R.NOISE_SHAPE, d, m)
    for (lo, hi), radius, flags in itertools.product(R.NOISE_REGIONS, R.NOISE_RADII, R.ALL_FLAGS):
        field_check(tr, R.field(vol[0], R.NOISE_ORIGIN, lo, hi, radius, flags), lo, hi, radius, flags)
    dense, md = R.noise(fill=0.5, seed=9)                          # half full: neighbours on every side of most cells
    vol = make(tr, keyed, R.NOISE_ORIGIN, R.NOISE_SHAPE, dense, md)
    for radius, flags in itertools.product((0, 1, 3), R.ALL_FLAGS):
        field_check(tr, R.field(vol[0], R.NOISE_ORIGIN, None, None, radius, flags), None, None, radius, flags)


@LAYOUTS
def test_field_of_the_scene_whole_and_over_regions_at_every_face(tr, keyed):
    """40 x 36 x 33 with a block, a plate, a staircase and scattered voxels, R = 8 and 16: more than one tile along y and z, sources outside
    the regions, FAR cells in both directions."""
    make(tr, keyed, R.SCENE_ORIGIN, R.SCENE_SHAPE, *R.scene())
    for lo, hi, radius, flags in R.scene_cases():
        field_check(tr, R.scene_field(lo, hi, radius, flags), lo, hi, radius, flags, pieces=lo is not None and flags == 0)


@LAYOUTS
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["along-x", "along-y", "along-z"])
def test_field_of_the_line_boxes(tr, keyed, axis):
    """600 x 5 x 3 and its permutations: R = 255 with cells 255 and 256 away from a lone source, the source outside the region, and
    sources 63, 64 and 65 apart — the seams of a 64-bit row word and of a 64-lane wave."""
    for name, sources, region in R.line_cases():
        shape, src, (lo, hi) = R.permuted(R.LINE_SHAPE, sources, region, axis)
        make(tr, keyed, (0, 0, 0), shape, *R.volume_with(shape, src))
        for radius in (255, 64):
            whole = R.from_sources(shape, src, radius)
            want = cut(whole, lo, hi)
            l = lo or (0, 0, 0)
            got = field_check(tr, (want, R.make_info((0, 0, 0), l, want.shape[::-1], radius, 0, want)), lo, hi, radius, 0, pieces=False)
            if name == "one" and radius == 255:
                z, y, x = _zyx(sources[0], axis)

                def at(k):
                    index = [z, y, x]
                    index[2 - axis] += k
                    return int(got[tuple(index)])
                assert at(255) == 65025 and at(256) == FAR and at(-255) == 65025 and at(-256) == FAR


def _zyx(source_on_x, axis):
    """[z][y][x] index of a line case's source after the permutation."""
    s = R.permuted(R.LINE_SHAPE, [source_on_x], (None, None), axis)[1][0]
    return (s[2], s[1], s[0])


@LAYOUTS
def test_field_across_the_builders_tile_seams(tr, keyed):
    """150 x 140 x 130, a lone source at eight positions next to and across the borders of the builder's tiles (blok_amd/distance.py
    exports their extents), R = 70 and 255, against the closed form.  The source is moved by set_voxels: every field reads fresh masks."""
    make(tr, keyed, (0, 0, 0), R.SEAM_SHAPE)
    previous = None
    for s in R.seam_sources(D.ROW_CELLS, D.TILE_X, D.TILE_ROWS, D.CHUNK_ROWS):
        if previous is not None:
            tr.volume_set_voxels([previous], [0], [0.0])
        tr.volume_set_voxels([s], [3], [1.0])
        previous = s
        for radius in (70, 255):
            want = R.single_source(R.SEAM_SHAPE, s, radius)
            field_check(tr, (want, R.make_info((0, 0, 0), (0, 0, 0), R.SEAM_SHAPE, radius, 0, want)), None, None, radius, 0, pieces=False)


@LAYOUTS
def test_field_of_the_extremes(tr, keyed):
    origin, shape = R.NOISE_ORIGIN, R.NOISE_SHAPE
    vol = make(tr, keyed, origin, shape)                           # empty
    for radius, flags in itertools.product((0, 3), R.ALL_FLAGS):
        got = field_check(tr, R.field(vol[0], origin, None, None, radius, flags), None, None, radius, flags)
        if flags == 0:
            assert (got == FAR).all()
        if flags & R.TO_EMPTY:
            assert (got == 0).all()
    full = np.full(shape[::-1], 1.0, np.float32), np.full(shape[::-1], 2, np.uint32)
    vol = make(tr, keyed, origin, shape, *full)
    for radius, flags in itertools.product((0, 3), R.ALL_FLAGS):
        got = field_check(tr, R.field(vol[0], origin, None, None, radius, flags), None, None, radius, flags)
        if flags == (R.TO_EMPTY | R.BOX_IS_SOLID):
            assert (got == FAR).all()
        if not flags & R.TO_EMPTY:
            assert (got == 0).all()
    # one brick filled, R larger than the box
    brick = [(x, y, z) for z in range(0, 4) for y in range(4, 8) for x in range(4, 8)]
    vol = make(tr, keyed, origin, shape, *R.volume_with(shape, brick))
    for radius in (20, 255):
        want = R.from_sources(shape, brick, radius)
        assert (want != FAR).all()
        field_check(tr, (want, R.make_info(origin, (0, 0, 0), shape, radius, 0, want)), None, None, radius, 0)
    field_check(tr, R.field(vol[0], origin, None, None, 20, R.TO_EMPTY | R.BOX_IS_SOLID), None, None, 20, R.TO_EMPTY | R.BOX_IS_SOLID)
    # an empty region: zero counts, an empty snapshot
    info = take(tr, (0, 0, 0), (0, 3, 2), 4, 0)
    assert counts(info) == [0, 0, 0] and info["ext"][0].tolist() == [0, 3, 2] and info["lo"][0].tolist() == [0, 0, 0]
    assert tr.volume_distance_download().size == 0 and tr.volume_distance_download(0, 0).size == 0


@LAYOUTS
def test_every_field_reads_the_masks_fresh_and_an_old_snapshot_stays(tr, keyed):
    d, m = R.scene()
    make(tr, keyed, R.SCENE_ORIGIN, R.SCENE_SHAPE, d, m)
    lo, hi = R.SCENE_REGIONS[3]
    old = field_check(tr, R.scene_field(lo, hi, 8, 0), lo, hi, 8, 0, pieces=False)
    o = np.array(R.SCENE_ORIGIN)
    xyz = np.array([[30, 30, 5], [31, 30, 5], [2, 20, 30]]) + o
    model = tr.model_create(np.array([[x, y, z] for x in range(3) for y in range(2) for z in range(4)], np.int32), np.full(24, 5, np.uint32))
    edits = [lambda: tr.volume_set_voxels(xyz, [7, 7, 7], [1.0, 0.5, 2.0]),
             lambda: tr.volume_apply_brush((o[0] + 10.0, o[1] + 10.5, o[2] + 9.0), 5.5, 0.0, 1),      # SUBTRACT out of the block
             lambda: tr.volume_stamp_models(S.placement((int(o[0]) + 30, int(o[1]) + 3, int(o[2]) + 27), model=model), _ffi.STAMP_SET, 1.25)]
    for i, edit in enumerate(edits):
        edit()
        assert tr.volume_distance_download().tobytes() == old.tobytes(), "an edit touched the snapshot"
        now = tr.volume_download()
        flags = R.ALL_FLAGS[i]
        got = field_check(tr, R.field(now[0], R.SCENE_ORIGIN, None, None, 8, flags), None, None, 8, flags, pieces=False)
        assert got.tobytes() != R.scene_field(None, None, 8, flags)[0].tobytes(), "the edit changed nothing the field sees"
        old = got
    tr.model_destroy(model)


@LAYOUTS
def test_the_snapshots_are_independent_of_each_other(tr, keyed):
    make(tr, keyed, R.SCENE_ORIGIN, R.SCENE_SHAPE, *R.scene())
    before = tr.volume_download()
    quads = tr.volume_extract_quads()
    n_components, _ = tr.volume_label_components()
    labels = tr.volume_labels_download(0, int(np.prod(R.SCENE_SHAPE)))
    records = tr.volume_components_download(0, n_components)
    tr.volume_encode_bricks()
    bricks = tr.volume_bricks_download()
    lo, hi = R.SCENE_REGIONS[2]
    dist = field_check(tr, R.scene_field(lo, hi, 8, 0), lo, hi, 8, 0, pieces=False)
    # the field call left the others as they were, and the volume too
    assert tr.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes()
    assert tr.volume_labels_download(0, len(labels)).tobytes() == labels.tobytes()
    assert n_components > 1 and tr.volume_components_download(0, n_components).tobytes() == records.tobytes()
    again = tr.volume_bricks_download()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, bricks))
    after = tr.volume_download()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # ... and theirs leave the field
    tr.volume_extract_quads(lo, hi)
    tr.volume_label_components(lo, hi)
    tr.volume_encode_bricks(lo, hi, filled_only=True)
    assert tr.volume_distance_download().tobytes() == dist.tobytes() and tr.volume_distance_info().tobytes() == R.scene_field(lo, hi, 8, 0)[1].tobytes()


def test_the_snapshot_dies_with_the_volume(tr):
    d, m = R.noise()
    make(tr, True, R.NOISE_ORIGIN, R.NOISE_SHAPE, d, m)

    def gone(status, fn, *a):
        with pytest.raises(BlokError) as e:
            fn(*a)
        assert e.value.status == status

    gone(BLOK_ERR_INVALID_ARG, tr.volume_distance_info)           # none taken yet in this volume
    take(tr, None, None, 2, 0)
    tr.volume_create(R.NOISE_ORIGIN, R.NOISE_SHAPE)               # a new volume
    gone(BLOK_ERR_INVALID_ARG, tr.volume_distance_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_distance_download, 0, 0)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.GROW, 1)
    take(tr, None, None, 2, 0)
    tr.volume_destroy()
    gone(BLOK_ERR_INVALID_ARG, tr.volume_distance_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_distance_download, 0, 0)
    gone(BLOK_ERR_NO_WORLD, tr.volume_edit_by_distance, D.GROW, 1)
    gone(BLOK_ERR_NO_WORLD, take, tr, None, None, 2, 0)


# ---- the edits ---------------------------------------------------------------------------------------------------------------------------------
D2 = (1, 2, 3, 9, 16)
# regions that end on 4-voxel and 16-voxel boundaries and on the box's faces (world voxels; the scene's origin is (3, -8, 10))
EDIT_REGIONS = [(None, None), ((3, -8, 10), (23, 8, 26)), ((7, -4, 14), (43, 28, 43)), ((4, -7, 11), (24, 12, 30)), ((19, 8, 26), (35, 24, 42))]


def scene_pair(tr, keyed):
    d, m = R.scene()
    make(tr, keyed, R.SCENE_ORIGIN, R.SCENE_SHAPE, d, m)
    model = DenseModel(R.SCENE_ORIGIN, R.SCENE_SHAPE)
    model.upload(d, m)
    return model


def edit_check(tr, model, mats, tag, lo, hi, op, d2, density=1.0, material=0, radius=None):
    """A fresh field of the region, the edit on the device and the model's edit on the DenseModel, then check()."""
    radius = int(np.ceil(np.sqrt(d2))) if radius is None else radius
    flags = 0 if op == D.GROW else R.TO_EMPTY
    want = R.field(model.density, model.origin, lo, hi, radius, flags)
    field_check(tr, want, lo, hi, radius, flags, pieces=False)
    n = tr.volume_edit_by_distance(op, d2, density, material)
    n_model = R.edit(model.density, model.ids, *want, op, d2, density, material, origin=model.origin)
    print(f"{tag}: device wrote {n}, model {n_model}")
    assert n == n_model, tag
    check(tr, model, tag, mats)
    return n


@LAYOUTS
@pytest.mark.parametrize("op", [D.GROW, D.SHRINK, D.HOLLOW], ids=["grow", "shrink", "hollow"])
def test_edits_on_the_scene(tr, mats, keyed, op):
    model = scene_pair(tr, keyed)
    check(tr, model, "uploaded", mats)
    total = 0
    for i, d2 in enumerate(D2[::-1] if op == D.HOLLOW else D2):      # (a HOLLOW leaves nothing for a later one at a larger threshold)
        lo, hi = EDIT_REGIONS[(i + op) % len(EDIT_REGIONS)]
        total += edit_check(tr, model, mats, f"op {op} d2 {d2} region {lo}..{hi}", lo, hi, op, d2, 0.75, 6)      # GROW writes a second material
    assert total > 0
    # the whole box at the largest threshold, with a radius above what d2 needs
    edit_check(tr, model, mats, f"op {op} whole", None, None, op, 16 if op != D.HOLLOW else 2, 1.5, 5, radius=6)      # (may find nothing left to write)


@LAYOUTS
def test_edits_judge_the_cells_as_they_are_now(tr, mats, keyed):
    model = scene_pair(tr, keyed)
    lo, hi = EDIT_REGIONS[3]
    o = np.array(R.SCENE_ORIGIN)
    for op, flags in ((D.GROW, 0), (D.HOLLOW, R.TO_EMPTY), (D.SHRINK, R.TO_EMPTY)):
        want = R.field(model.density, model.origin, lo, hi, 3, flags)
        field_check(tr, want, lo, hi, 3, flags, pieces=False)
        # between the field and the edit: cells next to the block are filled, cells of the block's skin and of its middle are cleared
        xyz = np.array([[19, 5, 5], [19, 6, 5], [18, 5, 5], [18, 6, 6], [9, 9, 9], [10, 9, 9]]) + o
        ids, dens = [8, 8, 0, 0, 0, 8], [2.5, 2.5, 0.0, 0.0, 0.0, 3.0]
        tr.volume_set_voxels(xyz, ids, dens)
        model.set_voxels(xyz, ids, dens)
        n = tr.volume_edit_by_distance(op, 4, 1.25, 6)
        assert n == R.edit(model.density, model.ids, *want, op, 4, 1.25, 6, origin=model.origin) > 0
        check(tr, model, f"now rule, op {op}", mats)
        assert tr.volume_distance_download().tobytes() == want[0].tobytes(), "the edit updated the snapshot"


@LAYOUTS
def test_an_id_written_under_an_unchanged_mask_shows_in_the_rebuilt_materials(tr, mats, keyed):
    """Between two rebuilds a SHRINK takes the block's skin off and a GROW puts it back with another id: the bricks inside the block's faces
    carry the mask of the last build, and only their dirty flags say that their ids must be gathered again."""
    model = scene_pair(tr, keyed)
    before = check(tr, model, "uploaded", mats)[1]
    lo, hi = (3, -8, 10), (23, 12, 30)                             # the block and a cell around it
    for op, flags, material in ((D.SHRINK, R.TO_EMPTY, 0), (D.GROW, 0, 6)):
        want = R.field(model.density, model.origin, lo, hi, 1, flags)
        field_check(tr, want, lo, hi, 1, flags, pieces=False)
        n = tr.volume_edit_by_distance(op, 1, 1.0, material)
        assert n == R.edit(model.density, model.ids, *want, op, 1, 1.0, material, origin=model.origin) > 0
    assert int((model.ids[1:19, 1:19, 1:19] == 6).sum()) > 1000     # the faces came back; edges and corners do not (an opening by the 6-neighbourhood)
    after = check(tr, model, "skin replaced", mats)[1]
    assert int((after == 6).sum()) > 1000 and int((before == 6).sum()) == 0


@LAYOUTS
def test_an_edit_on_an_empty_snapshot_writes_nothing(tr, mats, keyed):
    model = scene_pair(tr, keyed)
    for op, to_empty in ((D.GROW, False), (D.SHRINK, True), (D.HOLLOW, True)):
        info = tr.volume_distance_field((10, 0, 20), (10, 5, 25), 4, to_empty)
        assert counts(info) == [0, 0, 0]
        assert tr.volume_edit_by_distance(op, 9, 1.0, 3) == 0
    check(tr, model, "empty snapshot", mats)


# ---- the error table -------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_error_table_leaves_the_volume_and_the_snapshot_as_they_were(tr, keyed):
    d, m = R.noise(fill=0.3)
    o = R.NOISE_ORIGIN
    make(tr, keyed, o, R.NOISE_SHAPE, d, m)
    lib, ctx = tr._lib, tr._ctx
    import ctypes as C
    vec = lambda v: (C.c_int32 * 3)(*v)
    filled = R.field(d, o, None, None, 3, 0)
    field_check(tr, filled, None, None, 3, 0)

    def unchanged(want):
        now = tr.volume_download()
        assert now[0].tobytes() == d.tobytes() and now[1].tobytes() == m.tobytes()
        assert tr.volume_distance_download().tobytes() == want[0].tobytes() and tr.volume_distance_info().tobytes() == want[1].tobytes()

    def refused(status, fn, *a, **k):
        with pytest.raises(BlokError) as e:
            fn(*a, **k)
        assert e.value.status == status, (a, k)

    refused(BLOK_ERR_INVALID_ARG, tr.volume_distance_field, None, None, 256)                               # max_radius above 255
    refused(BLOK_ERR_INVALID_ARG, tr.volume_distance_field, (0, 2, 0), (1, 1, 1), 2)                       # lo above hi
    refused(BLOK_ERR_UNSUPPORTED, tr.volume_distance_field, (-6, 0, 0), (1, 1, 1), 2)                      # a region that leaves the box
    refused(BLOK_ERR_UNSUPPORTED, tr.volume_distance_field, (0, 0, 0), (1, 1, 6), 2)
    assert lib.blok_hip_volume_distance_field(ctx, None, None, 2, 4, None) == BLOK_ERR_INVALID_ARG        # unknown flag bits
    assert lib.blok_hip_volume_distance_field(ctx, vec((0, 0, 0)), None, 2, 0, None) == BLOK_ERR_INVALID_ARG      # exactly one region pointer
    assert lib.blok_hip_volume_distance_field(ctx, None, vec((1, 1, 1)), 2, 0, None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_hip_volume_distance_info(ctx, None) == BLOK_ERR_INVALID_ARG
    n = filled[0].size
    refused(BLOK_ERR_INVALID_ARG, tr.volume_distance_download, n, 1)                                       # a range past the end
    refused(BLOK_ERR_INVALID_ARG, tr.volume_distance_download, 1, n)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_distance_download, n + 1, 0)
    assert lib.blok_hip_volume_distance_download(ctx, None, 0, 1) == BLOK_ERR_INVALID_ARG                  # a NULL array with count > 0
    assert tr.volume_distance_download(n, 0).size == 0
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, 3, 1)                                        # an unknown op
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, -1, 1)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.SHRINK, 1)                                 # an op that needs the other kind of field
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.HOLLOW, 1)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.GROW, 10)                                  # d2 above R^2
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.GROW, 1, bad)                          # GROW needs a finite density > 0
    unchanged(filled)
    empty = R.field(d, o, None, None, 3, R.TO_EMPTY | R.BOX_IS_SOLID)
    field_check(tr, empty, None, None, 3, R.TO_EMPTY | R.BOX_IS_SOLID)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.GROW, 1)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.HOLLOW, 10)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_distance, D.SHRINK, 10)
    unchanged(empty)
    assert lib.blok_hip_volume_distance_field(ctx, None, None, 3, 0, None) == 0                            # out_info may be NULL
    assert tr.volume_distance_info().tobytes() == filled[1].tobytes()
    out = C.c_uint64(99)
    assert lib.blok_hip_volume_edit_by_distance(ctx, D.GROW, 0, C.c_float(1.0), 0, None) == 0              # out_n_voxels may be NULL; d2 = 0 writes nothing
    assert lib.blok_hip_volume_edit_by_distance(ctx, D.GROW, 0, C.c_float(1.0), 0, C.byref(out)) == 0 and out.value == 0
    unchanged(filled)
