"""GPU: blok_hip_volume_flood_field / flood_info / flood_download / edit_by_flood against the numpy model of the contract
(tests/flood_reference.py, pinned in tests/test_flood_cpu.py) over volume_download(): values and info byte for byte, whole and in pieces of
7, in every mode and both brick layouts, on the shapes at which the rounds can go wrong (test_flood_cpu.py asserts from the model alone what
makes them hard); the edits checked like check() of tests/test_volume_rebuild_gpu.py (arrays, then the rebuilt tree) against a DenseModel
that received the model's edit; the snapshot's life and independence; the error table.  Every comparison is exact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import flood as F
from blok_amd import stamp as S
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import flood_reference as R
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
    return [int(info[k][0]) for k in ("farthest", "n_seed", "n_reached", "n_unreached")]


def field_check(t, want, lo, hi, seeds, K, flags, material=0, pieces=True, tag=""):
    """The device's field equals `want` = (steps, info) of the reference; returns the downloaded values."""
    info = t.volume_flood_field(lo, hi, seeds, K, flags, material)
    got = t.volume_flood_download()
    differ = int((got != want[0]).sum()) if got.shape == want[0].shape else -1
    print(f"{tag} region {lo}..{hi} K={K} flags={flags}: reference {counts(want[1])}, device {counts(info)}, {differ} of {got.size} values differ")
    assert got.dtype == np.uint16 and got.shape == want[0].shape and got.tobytes() == want[0].tobytes()
    assert info.tobytes() == want[1].tobytes() == t.volume_flood_info().tobytes()
    if pieces and got.size:
        assert t.volume_flood_download(0, got.size, page=7).tobytes() == want[0].tobytes()
        assert t.volume_flood_download(got.size // 3, got.size - got.size // 3).tobytes() == want[0].ravel()[got.size // 3:].tobytes()
    return got


def case_check(t, keyed, case, uploaded=None, pieces=True):
    if uploaded is None or uploaded[0] is not case["d"]:
        make(t, keyed, case["origin"], case["shape"], case["d"], case["m"])
    return field_check(t, R.model_of(case), case["lo"], case["hi"], case["seeds"], case["K"], case["flags"], case["material"], pieces, case["name"])


# ---- the field ---------------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_field_of_the_noise_box_in_all_modes(tr, keyed):
    """13 x 10 x 7 at (-5, -3, -2), 45 %, 30 % and 90 % passable: through empty, through filled, SAME_MATERIAL with three ids; the whole box,
    regions off the brick grid, a one-cell region; listed seeds (one impassable, one twice), each SEED_FACE bit alone, all six."""
    uploaded = None
    for i, case in enumerate(R.noise_cases()):
        case_check(tr, keyed, case, uploaded, pieces=i % 5 == 0)
        uploaded = (case["d"],)


HARD = R.hard_cases()


@LAYOUTS
@pytest.mark.parametrize("case", HARD, ids=[c["name"].replace(" ", "-") for c in HARD])
def test_field_of_the_hard_cases(tr, keyed, case):
    """The maze (a cell first written through few bricks and lowered later), the one-brick snake (20 in-brick sweeps), tunnels whose only
    route crosses a brick face in each of the six directions, 600 x 5 x 3 line boxes at the caps 255 and 599, empty and full volumes, no
    seeds, K = 0."""
    got = case_check(tr, keyed, case, pieces=case["d"].size < 5000)
    if case["name"].startswith("line box"):
        K = case["K"]
        assert got.tobytes() == R.manhattan(case["shape"], case["seeds"][0], K).tobytes()
        assert (got == K).any() and int((got == FAR).sum()) > 0, "cells at exactly K and cells beyond it both exist"


@LAYOUTS
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["along-x", "along-y", "along-z"])
def test_field_of_the_long_corridor(tr, keyed, axis):
    """16384 x 5 x 3, filled but for its centre line, the seed at one end, K = 65534: farthest = 16383 over 4096 bricks in a row, some 4100
    rounds of a brick or two."""
    case = R.corridor(axis)
    got = case_check(tr, keyed, case, pieces=False)
    assert int(R.model_of(case)[1]["farthest"][0]) == 16383 and int(got[got != FAR].max()) == 16383


@LAYOUTS
def test_every_field_reads_the_volume_fresh_and_an_old_snapshot_stays(tr, keyed):
    d, m = R.scene()
    o = R.SCENE_ORIGIN
    make(tr, keyed, o, R.SCENE_SHAPE, d, m)
    seed = [R.world((0, 0, 0))]
    old = field_check(tr, R.field(d, m, o, None, None, seed, 200, 0), None, None, seed, 200, 0, pieces=False)
    xyz = np.array([R.HOLE, (1, 1, 1), (30, 30, 5)]) + np.array(o)     # the hole is plugged: the holed box's inside becomes a cavity
    model = tr.model_create(np.array([[x, y, z] for x in range(3) for y in range(2) for z in range(4)], np.int32), np.full(24, 5, np.uint32))
    edits = [lambda: tr.volume_set_voxels(xyz, [7, 7, 7], [1.0, 0.5, 2.0]),
             lambda: tr.volume_apply_brush((o[0] + 7.0, o[1] + 6.5, o[2] + 4.5), 3.5, 0.0, 1),      # SUBTRACT opens the closed box
             lambda: tr.volume_stamp_models(S.placement((o[0] + 30, o[1] + 3, o[2] + 27), model=model), _ffi.STAMP_SET, 1.25)]
    for i, edit in enumerate(edits):
        edit()
        assert tr.volume_flood_download().tobytes() == old.tobytes(), "an edit touched the snapshot"
        now = tr.volume_download()
        flags = (0, 0, R.THROUGH_FILLED)[i]
        start = seed if i < 2 else [(o[0] + 30, o[1] + 3, o[2] + 27)]
        got = field_check(tr, R.field(now[0], now[1], o, None, None, start, 200, flags), None, None, start, 200, flags, pieces=False)
        assert got.tobytes() != R.field(d, m, o, None, None, start, 200, flags)[0].tobytes(), "the edit changed nothing the field sees"
        old = got
    tr.model_destroy(model)


@LAYOUTS
def test_the_snapshots_are_independent_of_each_other(tr, keyed):
    d, m = R.scene()
    o = R.SCENE_ORIGIN
    make(tr, keyed, o, R.SCENE_SHAPE, d, m)
    before = tr.volume_download()
    quads = tr.volume_extract_quads()
    n_components, _ = tr.volume_label_components()
    labels = tr.volume_labels_download(0, int(np.prod(R.SCENE_SHAPE)))
    records = tr.volume_components_download(0, n_components)
    tr.volume_encode_bricks()
    bricks = tr.volume_bricks_download()
    tr.volume_distance_field(None, None, 4)
    dist = tr.volume_distance_download()
    lo, hi = R.world((4, 4, 4)), R.world((40, 36, 33))
    want = R.field(d, m, o, lo, hi, None, 50, R.ALL_FACES)
    steps = field_check(tr, want, lo, hi, None, 50, R.ALL_FACES, pieces=False)
    # the flood left the others as they were, and the volume too
    assert tr.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes()
    assert tr.volume_labels_download(0, len(labels)).tobytes() == labels.tobytes()
    assert n_components > 1 and tr.volume_components_download(0, n_components).tobytes() == records.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tr.volume_bricks_download(), bricks))
    assert tr.volume_distance_download().tobytes() == dist.tobytes()
    after = tr.volume_download()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # ... and theirs leave the flood
    tr.volume_extract_quads(lo, hi)
    tr.volume_label_components(lo, hi)
    tr.volume_encode_bricks(lo, hi, filled_only=True)
    tr.volume_distance_field(lo, hi, 3, True)
    assert tr.volume_flood_download().tobytes() == steps.tobytes() and tr.volume_flood_info().tobytes() == want[1].tobytes()


def test_the_snapshot_dies_with_the_volume(tr):
    d, m = R.noise()
    make(tr, True, R.NOISE_ORIGIN, R.NOISE_SHAPE, d, m)

    def gone(status, fn, *a):
        with pytest.raises(BlokError) as e:
            fn(*a)
        assert e.value.status == status

    gone(BLOK_ERR_INVALID_ARG, tr.volume_flood_info)              # none taken yet in this volume
    tr.volume_flood_field(None, None, None, 2, R.ALL_FACES)
    tr.volume_create(R.NOISE_ORIGIN, R.NOISE_SHAPE)               # a new volume
    gone(BLOK_ERR_INVALID_ARG, tr.volume_flood_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_flood_download, 0, 0)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.FILL, 1)
    tr.volume_flood_field(None, None, None, 2, R.ALL_FACES)
    tr.volume_destroy()
    gone(BLOK_ERR_INVALID_ARG, tr.volume_flood_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_flood_download, 0, 0)
    gone(BLOK_ERR_NO_WORLD, tr.volume_edit_by_flood, F.FILL, 1)
    gone(BLOK_ERR_NO_WORLD, tr.volume_flood_field, None, None, None, 2, R.ALL_FACES)


# ---- the edits ---------------------------------------------------------------------------------------------------------------------------------
# regions that end on 4-voxel and 16-voxel boundaries and on the box's faces (world voxels; the scene's origin is (3, -8, 10))
EDIT_REGIONS = [(None, None), ((3, -8, 10), (23, 8, 26)), ((7, -4, 14), (43, 28, 43)), ((4, -7, 11), (35, 24, 42)), ((3, -8, 10), (43, 28, 26))]


def scene_pair(tr, keyed):
    d, m = R.scene()
    make(tr, keyed, R.SCENE_ORIGIN, R.SCENE_SHAPE, d, m)
    model = DenseModel(R.SCENE_ORIGIN, R.SCENE_SHAPE)
    model.upload(d, m)
    return model


def edit_check(tr, model, mats, tag, lo, hi, seeds, K, flags, flood_material, op, d, density=1.0, material=0):
    """A fresh field of the region, the edit on the device and the model's edit on the DenseModel, then check()."""
    want = R.field(model.density, model.ids, model.origin, lo, hi, seeds, K, flags, flood_material)
    field_check(tr, want, lo, hi, seeds, K, flags, flood_material, pieces=False, tag=tag)
    n = tr.volume_edit_by_flood(op, d, density, material)
    n_model = R.edit(model.density, model.ids, *want, op, d, density, material, origin=model.origin)
    print(f"{tag}: device wrote {n}, model {n_model}")
    assert n == n_model, tag
    check(tr, model, tag, mats)
    return n, want


@LAYOUTS
def test_fill_unreached_seals_exactly_the_closed_box(tr, mats, keyed):
    model = scene_pair(tr, keyed)
    check(tr, model, "uploaded", mats)
    n, want = edit_check(tr, model, mats, "seal", None, None, None, R.MAX_STEPS, R.ALL_FACES, 0, F.FILL_UNREACHED, 0, 0.75, 6)
    assert int(want[1]["farthest"][0]) < R.MAX_STEPS, "the flood ended on its own"
    assert n == R.CLOSED_INSIDE == int(want[1]["n_unreached"][0])
    (x0, y0, z0), (x1, y1, z1) = R.CLOSED
    assert (model.ids[z0 + 1:z1 - 1, y0 + 1:y1 - 1, x0 + 1:x1 - 1] == 6).all() and int((model.ids == 6).sum()) == n
    # over regions: what the region's faces do not reach is sealed, the holed box's inside included once the region cuts its hole off
    for i, (lo, hi) in enumerate(EDIT_REGIONS[1:]):
        edit_check(tr, model, mats, f"seal region {i}", lo, hi, None, R.MAX_STEPS, R.ALL_FACES, 0, F.FILL_UNREACHED, 0, 1.5, 7 + i)


@LAYOUTS
def test_fill_pours_up_to_the_regions_top_and_plugs(tr, mats, keyed):
    model = scene_pair(tr, keyed)
    total = 0
    # water poured through the hole, up to three cells below it: the region's top is the water level
    inside = R.world((R.HOLE[0], R.HOLE[1], R.HOLED[0][2] + 1))
    lo, hi = R.world((0, 0, 0)), R.world((40, 36, R.HOLE[2] - 3))
    total += edit_check(tr, model, mats, "pour", lo, hi, [inside], R.MAX_STEPS, 0, 0, F.FILL, R.MAX_STEPS, 0.5, 9)[0]
    # a plug of three steps around the hole; then steps from three faces over the other regions
    total += edit_check(tr, model, mats, "plug", None, None, [R.world(R.HOLE)], 40, 0, 0, F.FILL, 3, 2.0, 8)[0]
    for i, (lo, hi) in enumerate(EDIT_REGIONS[1:]):
        total += edit_check(tr, model, mats, f"fill region {i}", lo, hi, None, 6, R.seed_face(i) | R.seed_face(5), 0, F.FILL, 2 + i, 1.25, 10 + i)[0]
    assert total > 1000


@LAYOUTS
def test_paint_and_clear_follow_the_material(tr, mats, keyed):
    model = scene_pair(tr, keyed)
    before = check(tr, model, "uploaded", mats)[1]
    a, b = R.world(R.BLOCK_A[0]), R.world(R.BLOCK_B[0])
    # the paint bucket on block A alone (SAME_MATERIAL), between two rebuilds: no mask changes, the material array does
    n, _ = edit_check(tr, model, mats, "paint A", None, None, [a], R.MAX_STEPS, R.THROUGH_FILLED | R.SAME_MATERIAL, 3, F.PAINT, R.MAX_STEPS, 9.0, 11)
    size = lambda blk: int(np.prod([blk[1][k] - blk[0][k] for k in range(3)]))
    assert n == size(R.BLOCK_A) and int((model.ids == 11).sum()) == n and int((model.ids == 4).sum()) == size(R.BLOCK_B)
    after = check(tr, model, "painted", mats)[1]
    assert int((after == 11).sum()) == n and int((before == 11).sum()) == 0
    assert (model.density[model.ids == 11] == np.float32(0.5)).all(), "PAINT left the densities"
    # through everything filled the two touching blocks are one piece: paint within 12 steps over regions, then clear within 7
    for i, (lo, hi) in enumerate(EDIT_REGIONS):
        if i == 1:                                                # (this region does not hold block B's corner)
            continue
        edit_check(tr, model, mats, f"paint region {i}", lo, hi, [b], 20, R.THROUGH_FILLED, 0, F.PAINT, 12, 1.0, 12 + i)
    n, _ = edit_check(tr, model, mats, "clear", None, None, [b], 30, R.THROUGH_FILLED, 0, F.CLEAR, 7, 1.0, 5)
    assert n > 100 and model.ids[R.BLOCK_B[0][2], R.BLOCK_B[0][1], R.BLOCK_B[0][0]] == 0


@LAYOUTS
def test_edits_judge_the_cells_as_they_are_now(tr, mats, keyed):
    model = scene_pair(tr, keyed)
    o = np.array(R.SCENE_ORIGIN)
    a = R.world(tuple(c - 1 for c in R.BLOCK_A[1]))                # block A's far corner: the near one is cleared below
    for op, flags, seeds in ((F.FILL, R.ALL_FACES, None), (F.FILL_UNREACHED, R.ALL_FACES, None), (F.PAINT, R.THROUGH_FILLED, [a]), (F.CLEAR, R.THROUGH_FILLED, [a])):
        want = R.field(model.density, model.ids, model.origin, None, None, seeds, 9, flags)
        field_check(tr, want, None, None, seeds, 9, flags, pieces=False)
        # between the field and the edit: cells near the faces and in the closed box are filled, cells of block A are cleared
        xyz = np.array([[0, 0, 0], [1, 0, 0], [5, 5, 5], [6, 5, 5], R.BLOCK_A[0], [6, 19, 15], [1, 1, 0]]) + o
        ids, dens = [8, 8, 8, 8, 0, 0, 0], [2.5, 2.5, 1.0, 1.0, 0.0, 0.0, 0.0]
        tr.volume_set_voxels(xyz, ids, dens)
        model.set_voxels(xyz, ids, dens)
        n = tr.volume_edit_by_flood(op, 4, 1.25, 6)
        assert n == R.edit(model.density, model.ids, *want, op, 4, 1.25, 6, origin=model.origin) > 0
        check(tr, model, f"now rule, op {op}", mats)
        assert tr.volume_flood_download().tobytes() == want[0].tobytes(), "the edit updated the snapshot"


@LAYOUTS
def test_an_edit_on_an_empty_snapshot_writes_nothing(tr, mats, keyed):
    model = scene_pair(tr, keyed)
    for op, flags in ((F.FILL, 0), (F.FILL_UNREACHED, 0), (F.PAINT, R.THROUGH_FILLED), (F.CLEAR, R.THROUGH_FILLED)):
        info = tr.volume_flood_field((10, 0, 20), (10, 5, 25), None, 4, flags | R.ALL_FACES)
        assert counts(info) == [0, 0, 0, 0] and info["ext"][0].tolist() == [0, 5, 5]
        assert tr.volume_flood_download().size == 0 and tr.volume_flood_download(0, 0).size == 0
        assert tr.volume_edit_by_flood(op, 3, 1.0, 3) == 0
    check(tr, model, "empty snapshot", mats)


# ---- the error table -------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_error_table_leaves_the_volume_and_the_snapshot_as_they_were(tr, keyed):
    d, m = R.noise()
    o = R.NOISE_ORIGIN
    make(tr, keyed, o, R.NOISE_SHAPE, d, m)
    lib, ctx = tr._lib, tr._ctx
    vec = lambda v: (C.c_int32 * 3)(*v)
    seeds = R.picked_seeds(d, m, o, None, None, 0, 0)
    empty = R.field(d, m, o, None, None, seeds, 3, 0)
    field_check(tr, empty, None, None, seeds, 3, 0)

    def unchanged(want):
        now = tr.volume_download()
        assert now[0].tobytes() == d.tobytes() and now[1].tobytes() == m.tobytes()
        assert tr.volume_flood_download().tobytes() == want[0].tobytes() and tr.volume_flood_info().tobytes() == want[1].tobytes()

    def refused(status, fn, *a, **k):
        with pytest.raises(BlokError) as e:
            fn(*a, **k)
        assert e.value.status == status, (a, k)
        return str(e.value)

    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_field, None, None, seeds, 65535)                        # max_steps above 65534
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_field, None, None, seeds, 3, R.SAME_MATERIAL)           # SAME_MATERIAL without THROUGH_FILLED
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_field, None, None, seeds, 3, 4)                         # unknown flag bits
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_field, None, None, seeds, 3, 1 << 14)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_field, (0, 2, 0), (1, 1, 1), None, 2)                   # lo above hi
    refused(BLOK_ERR_UNSUPPORTED, tr.volume_flood_field, (-6, 0, 0), (1, 1, 1), None, 2)                  # a region that leaves the box
    refused(BLOK_ERR_UNSUPPORTED, tr.volume_flood_field, (0, 0, 0), (1, 1, 6), None, 2)
    text = refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_field, None, None, [seeds[0], (8, 0, 0), (9, 9, 9)], 2)      # a seed outside the box ...
    assert "seed 1 " in text, text                                # ... named: the first one
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_field, (-4, -2, -1), (7, 6, 4), [(-5, 0, 0)], 2)        # ... and one inside the box, outside the region
    assert lib.blok_hip_volume_flood_field(ctx, None, None, None, 1, 2, 0, 0, None) == BLOK_ERR_INVALID_ARG      # a NULL seed array with n_seeds > 0
    assert lib.blok_hip_volume_flood_field(ctx, vec((0, 0, 0)), None, None, 0, 2, 0, 0, None) == BLOK_ERR_INVALID_ARG      # exactly one region pointer
    assert lib.blok_hip_volume_flood_field(ctx, None, vec((1, 1, 1)), None, 0, 2, 0, 0, None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_hip_volume_flood_info(ctx, None) == BLOK_ERR_INVALID_ARG
    n = empty[0].size
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_download, n, 1)                                         # a range past the end
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_download, 1, n)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_flood_download, n + 1, 0)
    assert lib.blok_hip_volume_flood_download(ctx, None, 0, 1) == BLOK_ERR_INVALID_ARG                    # a NULL array with count > 0
    assert tr.volume_flood_download(n, 0).size == 0
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, 4, 1)                                          # an unknown op
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, -1, 1)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.PAINT, 1)                                    # an op on the wrong kind of field
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.CLEAR, 1)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.FILL, 4)                                     # d above the snapshot's max_steps
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.FILL, 1, bad)                            # the FILL ops need a finite density > 0
        refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.FILL_UNREACHED, 1, bad)
    unchanged(empty)
    filled = R.field(d, m, o, None, None, None, 3, R.THROUGH_FILLED | R.seed_face(2))
    field_check(tr, filled, None, None, None, 3, R.THROUGH_FILLED | R.seed_face(2))
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.FILL, 1)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.FILL_UNREACHED, 1)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.PAINT, 4)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_edit_by_flood, F.CLEAR, 4)
    unchanged(filled)
    xyz = np.ascontiguousarray(seeds, dtype=np.int32)
    assert lib.blok_hip_volume_flood_field(ctx, None, None, _ffi.ptr(xyz), len(xyz), 3, 0, 0, None) == 0  # out_info may be NULL
    assert tr.volume_flood_info().tobytes() == empty[1].tobytes()
    out = C.c_uint64(99)
    assert lib.blok_hip_volume_edit_by_flood(ctx, F.PAINT, 0, C.c_float(1.0), 0, C.byref(out)) == BLOK_ERR_INVALID_ARG and out.value == 0
    unchanged(empty)
