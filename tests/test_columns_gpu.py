"""GPU: blok_hip_volume_column_field / columns_info / columns_download and blok_hip_volume_scatter_models / scatter_info /
scatter_download / scatter_device against the numpy model of the contract (tests/columns_reference.py, pinned in tests/test_columns_cpu.py)
over volume_download(): planes, tables and infos byte for byte, whole and in pieces, along all three axes in both directions and both brick
layouts, on the shapes at which the walk over the bricks can go wrong (test_columns_cpu.py asserts from the model alone what makes them
hard); the snapshot's life and independence; the error tables; and the table traced where it lies and stamped.  Every comparison is
exact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import columns_reference as R
from tests import limit_cases as LC
from tests import stamp_reference as SR
from tests.conftest import SEED
from tests.test_volume_rebuild_gpu import check
from tests.volume_tree_reference import DenseModel

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


@pytest.fixture(scope="module")
def scene():
    return R.scene()


def make(t, keyed, origin, shape, d=None, m=None):
    t.set_volume_layout(keyed)
    t.volume_create(origin, shape)
    if d is not None:
        t.volume_upload(d, m)
    return t.volume_download()


def counts(info):
    return [int(info[k][0]) for k in ("n_columns", "n_hit", "min_top", "max_top")]


def field_check(t, want, lo, hi, axis, flags, pieces=True, tag=""):
    """The device's field equals `want` = (top, material, info) of the reference; returns the downloaded planes."""
    info = t.volume_column_field(lo, hi, axis, flags)
    top, material = t.volume_columns_download(0), t.volume_columns_download(1)
    differ = int((top != want[0]).sum()) if top.shape == want[0].shape else -1
    print(f"{tag} region {lo}..{hi} axis {axis} flags {flags}: reference {counts(want[2])}, device {counts(info)}, {differ} of {top.size} tops differ")
    assert top.dtype == np.uint16 and material.dtype == np.uint32
    assert top.tobytes() == want[0].tobytes() and material.tobytes() == want[1].tobytes()
    assert info.tobytes() == want[2].tobytes() == t.volume_columns_info().tobytes()
    n = top.size
    if pieces and n:
        for plane in (0, 1):
            assert t.volume_columns_download(plane, 0, n, page=7).tobytes() == want[plane].tobytes()
            assert t.volume_columns_download(plane, n // 3, n - n // 3).tobytes() == want[plane][n // 3:].tobytes()
    return top, material


def case_check(t, keyed, c, uploaded=None, pieces=True):
    if uploaded is not c["d"]:
        make(t, keyed, c["origin"], c["shape"], c["d"], c["m"])
    return field_check(t, R.model_of(c), c["lo"], c["hi"], c["axis"], c["flags"], pieces, c["name"])


# ---- the field ---------------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_field_of_the_noise_box(tr, keyed):
    """13 x 10 x 7 at (-5, -3, -2), fill 0.05 (mostly NONE) and 0.5 (early hits): the whole box, regions off the brick grid, a one-cell
    region, an empty region; three axes, both directions."""
    uploaded = None
    for i, c in enumerate(R.noise_cases()):
        case_check(tr, keyed, c, uploaded, pieces=i % 4 == 0)
        uploaded = c["d"]
        if c["hi"] == (0, 4, 4):
            assert tr.volume_columns_download(0).size == 0 and tr.volume_columns_download(1, 0, 0).size == 0


@LAYOUTS
def test_field_of_the_hard_cases(tr, keyed):
    """Regions that cut their first and last brick, with tops in both and columns without any (test_columns_cpu.py)."""
    uploaded = None
    for c in R.hard_cases():
        case_check(tr, keyed, c, uploaded)
        uploaded = c["d"]


@LAYOUTS
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["along-x", "along-y", "along-z"])
def test_field_at_the_seams_of_the_brick_groups(tr, keyed, axis):
    """5 x 300 x 6 and its permutations: one filled cell per column at travel positions 0, 1, 3, 4, 63, 64, 255, 256, 298, 299 — the seams
    of a brick and of groups of 4, 16 and 64 bricks — in both directions, over the whole box and over cells 1 .. 298."""
    uploaded = None
    for c in R.seam_cases():
        if c["axis"] == axis:
            top, _ = case_check(tr, keyed, c, uploaded)
            uploaded = c["d"]
            if c["lo"] is None:
                assert sorted(top[top != R.NONE].tolist()) == sorted(R.SEAMS)


@LAYOUTS
@pytest.mark.parametrize("long_axis", [0, 1, 2], ids=["long-x", "long-y", "long-z"])
def test_field_of_the_staircase_across_waves(tr, keyed, long_axis):
    """300 x 5 x 5 and its permutations: more than 64 and more than 256 columns side by side, the surface stepping at 63, 64, 65, 255, 256."""
    uploaded = None
    for c in R.stair_cases():
        if c["name"].startswith(f"stairs long {long_axis} "):
            case_check(tr, keyed, c, uploaded, pieces=False)
            uploaded = c["d"]


@LAYOUTS
@pytest.mark.parametrize("which", ["LOW", "HIGH"])
def test_field_in_the_limit_boxes(tr, keyed, which):
    uploaded = None
    for axis in range(3):
        for flags in (0, R.FROM_LOW):
            c = R.limit_case(which, axis, flags)
            if uploaded is not None:
                c["d"] = uploaded                                # (the same arrays: one upload)
            case_check(tr, keyed, c, uploaded, pieces=False)
            uploaded = c["d"]


@pytest.mark.parametrize("box", LC.LONG_BOXES, ids=LC.LONG_IDS)
def test_field_along_16384_cells(tr, box):
    """The closed form of columns_reference.long_expected (pinned to the model at 600 cells in test_columns_cpu.py): tops at cell 0 and at
    cell 16383, 4096 bricks to a column."""
    d, m = R.long_fill(box)
    make(tr, True, box.origin, box.shape, d, m)
    for flags in (0, R.FROM_LOW):
        want = R.long_expected(box, flags)
        info = tr.volume_column_field(None, None, box.axis, flags)
        assert tr.volume_columns_download(0).tobytes() == want[0].tobytes() and tr.volume_columns_download(1).tobytes() == want[1].tobytes()
        hit = want[0][want[0] != R.NONE]
        assert counts(info) == [want[0].size, hit.size, int(hit.min()), int(hit.max())]


@LAYOUTS
def test_the_material_plane_reads_the_ids_as_they_are_now(tr, keyed, scene):
    """volume_set_voxels changes ids under an unchanged mask: the next field sees them without a rebuild."""
    d, m = scene
    o = R.SCENE_ORIGIN
    make(tr, keyed, o, R.SCENE_SHAPE, d, m)
    before = field_check(tr, R.field(d, m, o, None, None, 1, 0), None, None, 1, 0, pieces=False)
    xz = [(3, 4), (50, 20), (95, 79)]
    top = before[0].reshape(R.SCENE_SHAPE[2], R.SCENE_SHAPE[0])
    xyz = np.array([(o[0] + x, o[1] + int(top[z, x]), o[2] + z) for x, z in xz])
    tr.volume_set_voxels(xyz, [201, 202, 203], [1.0, 1.0, 1.0])
    now = tr.volume_download()
    assert ((now[0] > 0) == (d > 0)).all(), "the masks are unchanged"
    after = field_check(tr, R.field(now[0], now[1], o, None, None, 1, 0), None, None, 1, 0, pieces=False)
    assert after[0].tobytes() == before[0].tobytes() and [int(after[1].reshape(top.shape)[z, x]) for x, z in xz] == [201, 202, 203]


@LAYOUTS
def test_the_snapshot_stays_under_edits_and_the_next_field_replaces_it(tr, keyed, scene):
    d, m = scene
    o = R.SCENE_ORIGIN
    make(tr, keyed, o, R.SCENE_SHAPE, d, m)
    want = R.field(d, m, o, None, None, 1, 0)
    old = field_check(tr, want, None, None, 1, 0, pieces=False)
    tr.volume_apply_brush((o[0] + 30.0, o[1] + 16.0, o[2] + 20.0), 5.5, 1.0, 0)          # ADD: a mound on the ground
    assert tr.volume_columns_download(0).tobytes() == old[0].tobytes() and tr.volume_columns_download(1).tobytes() == old[1].tobytes(), "an edit touched the snapshot"
    assert tr.volume_columns_info().tobytes() == want[2].tobytes()
    now = tr.volume_download()
    new = field_check(tr, R.field(now[0], now[1], o, None, None, 1, 0), None, None, 1, 0, pieces=False)
    assert new[0].tobytes() != old[0].tobytes(), "the brush changed nothing the field sees"
    lo, hi = (o[0] + 5, o[1] + 3, o[2] + 9), (o[0] + 70, o[1] + 33, o[2] + 61)
    field_check(tr, R.field(now[0], now[1], o, lo, hi, 2, R.FROM_LOW), lo, hi, 2, R.FROM_LOW, pieces=False)      # replaced: another region, axis and direction


@LAYOUTS
def test_the_snapshots_are_independent_of_each_other(tr, keyed, scene):
    d, m = scene
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
    tr.volume_flood_field(None, None, None, 50, _ffi.flood_seed_face(2))
    flood = tr.volume_flood_download()
    lo, hi = (o[0] + 4, o[1] + 4, o[2] + 4), (o[0] + 90, o[1] + 36, o[2] + 77)
    want = R.field(d, m, o, lo, hi, 1, 0)
    planes = field_check(tr, want, lo, hi, 1, 0, pieces=False)
    tr.volume_scatter_models(R.scene_params(), R.entries(R.ENTRIES3))
    table = tr.volume_scatter_download()
    # the field and the scatter left the others as they were, and the volume too
    assert tr.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes()
    assert tr.volume_labels_download(0, len(labels)).tobytes() == labels.tobytes()
    assert n_components > 1 and tr.volume_components_download(0, n_components).tobytes() == records.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tr.volume_bricks_download(), bricks))
    assert tr.volume_distance_download().tobytes() == dist.tobytes() and tr.volume_flood_download().tobytes() == flood.tobytes()
    after = tr.volume_download()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # ... and theirs leave the field and the table
    tr.volume_extract_quads(lo, hi)
    tr.volume_label_components(lo, hi)
    tr.volume_encode_bricks(lo, hi, filled_only=True)
    tr.volume_distance_field(lo, hi, 3, True)
    tr.volume_flood_field(lo, hi, None, 9, _ffi.flood_seed_face(3))
    assert tr.volume_columns_download(0).tobytes() == planes[0].tobytes() and tr.volume_columns_download(1).tobytes() == planes[1].tobytes()
    assert tr.volume_columns_info().tobytes() == want[2].tobytes()
    assert len(table) > 0 and tr.volume_scatter_download().tobytes() == table.tobytes()


def gone(status, fn, *a):
    with pytest.raises(BlokError) as e:
        fn(*a)
    assert e.value.status == status


def test_the_snapshot_and_the_table_die_with_the_volume_and_the_table_with_the_field(tr, scene):
    d, m = scene
    make(tr, True, R.SCENE_ORIGIN, R.SCENE_SHAPE, d, m)
    p, ent = R.scene_params(), R.entries(R.ENTRIES3)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_info)            # none taken yet in this volume
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_models, p, ent)
    tr.volume_column_field()
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_info)            # a field, but no table yet
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_device)
    tr.volume_scatter_models(p, ent)
    assert tr.volume_scatter_device()[1] == int(tr.volume_scatter_info()["n_placed"][0]) > 0
    tr.volume_column_field()                                      # a new field frees the table
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_download, 0, 0)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_device)
    tr.volume_scatter_models(p, ent)
    tr.volume_create(R.SCENE_ORIGIN, R.SCENE_SHAPE)               # a new volume frees both
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_download, 0, 0, 0)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_models, p, ent)
    tr.volume_column_field()
    tr.volume_scatter_models(p, ent)
    tr.volume_destroy()
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_info)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_download, 0, 0)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_models, p, ent)
    gone(BLOK_ERR_NO_WORLD, tr.volume_column_field)


@LAYOUTS
def test_field_error_table_leaves_the_volume_and_the_snapshot_as_they_were(tr, keyed):
    d, m = R.noise(0.5)
    o = R.NOISE_ORIGIN
    make(tr, keyed, o, R.NOISE_SHAPE, d, m)
    lib, ctx = tr._lib, tr._ctx
    vec = lambda v: (C.c_int32 * 3)(*v)
    want = R.field(d, m, o, None, None, 2, R.FROM_LOW)
    field_check(tr, want, None, None, 2, R.FROM_LOW)

    def unchanged():
        now = tr.volume_download()
        assert now[0].tobytes() == d.tobytes() and now[1].tobytes() == m.tobytes()
        assert tr.volume_columns_download(0).tobytes() == want[0].tobytes() and tr.volume_columns_download(1).tobytes() == want[1].tobytes()
        assert tr.volume_columns_info().tobytes() == want[2].tobytes()

    gone(BLOK_ERR_INVALID_ARG, tr.volume_column_field, None, None, 3)                                     # axis above 2
    gone(BLOK_ERR_INVALID_ARG, tr.volume_column_field, None, None, 1, 2)                                  # unknown flag bits
    gone(BLOK_ERR_INVALID_ARG, tr.volume_column_field, None, None, 1, 1 << 20)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_column_field, (0, 2, 0), (1, 1, 1))                              # lo above hi
    gone(BLOK_ERR_UNSUPPORTED, tr.volume_column_field, (-6, 0, 0), (1, 1, 1))                             # a region that leaves the box
    gone(BLOK_ERR_UNSUPPORTED, tr.volume_column_field, (0, 0, 0), (1, 1, 6))
    assert lib.blok_hip_volume_column_field(ctx, vec((0, 0, 0)), None, 1, 0, None) == BLOK_ERR_INVALID_ARG      # exactly one region pointer
    assert lib.blok_hip_volume_column_field(ctx, None, vec((1, 1, 1)), 1, 0, None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_hip_volume_columns_info(ctx, None) == BLOK_ERR_INVALID_ARG
    n = want[0].size
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_download, 0, n, 1)                                       # a range past the end
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_download, 1, 1, n)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_download, 0, n + 1, 0)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_columns_download, 2, 0, 1)                                       # plane above 1
    assert lib.blok_hip_volume_columns_download(ctx, 0, None, 0, 1) == BLOK_ERR_INVALID_ARG               # a NULL array with count > 0
    assert lib.blok_hip_volume_columns_download(ctx, 1, None, 0, 1) == BLOK_ERR_INVALID_ARG
    assert tr.volume_columns_download(0, n, 0).size == 0
    unchanged()
    assert lib.blok_hip_volume_column_field(ctx, None, None, 2, R.FROM_LOW, None) == 0                    # out_info may be NULL
    unchanged()


# ---- scatter ----------------------------------------------------------------------------------------------------------------------------------
def scatter_check(t, field, p, ent, pieces=True, tag=""):
    """The device's table and info equal the reference's over `field` (the reference's field of the current snapshot)."""
    want = R.scatter(*field, p, ent)
    info = t.volume_scatter_models(p, ent)
    table = t.volume_scatter_download()
    print(f"{tag}: reference {want[1][0]}, device {info[0]}")
    assert table.dtype == _ffi.INSTANCE and table.tobytes() == want[0].tobytes()
    assert info.tobytes() == want[1].tobytes() == t.volume_scatter_info().tobytes()
    address, n = t.volume_scatter_device()
    assert n == len(table) and (address != 0) == (n > 0)
    if pieces and n:
        assert t.volume_scatter_download(0, n, page=7).tobytes() == want[0].tobytes()
        assert t.volume_scatter_download(n // 3, n - n // 3).tobytes() == want[0][n // 3:].tobytes()
    return table


@LAYOUTS
def test_scatter_over_the_scene(tr, keyed, scene):
    """The main cases (every test rejects something, every entry and orientation placed: test_columns_cpu.py), then cell_log2 x radius x
    probability, a region off the cell grid, 1 and 16 entries, the empty table, a table that replaces a longer one."""
    d, m = scene
    o = R.SCENE_ORIGIN
    make(tr, keyed, o, R.SCENE_SHAPE, d, m)
    taken = "nothing yet"
    lengths = []
    for i, (name, lo, hi, p, ent) in enumerate(R.main_scatter_cases() + R.sweep_scatter_cases()):
        if taken != (lo, hi):
            field = field_check(tr, R.field(d, m, o, lo, hi, 1, 0), lo, hi, 1, 0, pieces=False)
            field = (*field, tr.volume_columns_info())
            taken = (lo, hi)
        lengths.append(len(scatter_check(tr, field, p, ent, pieces=i < 4, tag=name)))
    assert 0 in lengths, "the empty table"
    assert any(b < a for a, b in zip(lengths, lengths[1:]) if b > 0), "a table that replaces a longer one"
    # an empty field: an empty table
    lo, hi = (o[0], o[1], o[2] + 20), (o[0], o[1] + 5, o[2] + 25)
    field = field_check(tr, R.field(d, m, o, lo, hi, 1, 0), lo, hi, 1, 0, pieces=False)
    assert len(scatter_check(tr, (*field, tr.volume_columns_info()), R.scene_params(), R.entries(R.ENTRIES3))) == 0


def test_scatter_error_table_leaves_the_previous_table(tr, scene):
    d, m = scene
    o = R.SCENE_ORIGIN
    make(tr, True, o, R.SCENE_SHAPE, d, m)
    field = R.field(d, m, o, None, None, 1, 0)
    tr.volume_column_field()
    p, ent = R.scene_params(), R.entries(R.ENTRIES3)
    table = scatter_check(tr, field, p, ent, pieces=False)
    info = tr.volume_scatter_info()
    lib, ctx = tr._lib, tr._ctx

    def refused(pp=p, e=ent):
        gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_models, pp, e)
        assert tr.volume_scatter_download().tobytes() == table.tobytes() and tr.volume_scatter_info().tobytes() == info.tobytes()

    refused(R.scene_params(flags=8))                                               # unknown flag bits
    bad = R.scene_params(); bad["reserved"][0][0] = 7
    refused(bad)                                                                   # a non-zero reserved word
    refused(R.scene_params(cell_log2=9))
    refused(R.scene_params(probability=65537))
    refused(R.scene_params(radius=9))
    refused(R.scene_params(max_rise=0x10000))
    refused(R.scene_params(min_y=5, max_y=4))
    refused(e=ent[:0])                                                             # no entries
    refused(e=R.entries([R.ENTRIES3[0]] * 17))
    refused(e=R.entries([(0, 0, (0, 0, 0), 0)]))                                   # a zero weight
    refused(e=R.entries([(0, 65536, (0, 0, 0), 0)]))
    assert lib.blok_hip_volume_scatter_models(ctx, None, _ffi.ptr(ent), 3, None) == BLOK_ERR_INVALID_ARG      # NULL pointers
    assert lib.blok_hip_volume_scatter_models(ctx, _ffi.ptr(p), None, 3, None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_hip_volume_scatter_info(ctx, None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_hip_volume_scatter_device(ctx, None, None) == BLOK_ERR_INVALID_ARG
    n = len(table)
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_download, n, 1)                   # a range past the end
    gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_download, n + 1, 0)
    assert lib.blok_hip_volume_scatter_download(ctx, None, 0, 1) == BLOK_ERR_INVALID_ARG
    assert tr.volume_scatter_download(n, 0).size == 0
    assert tr.volume_scatter_download().tobytes() == table.tobytes() and tr.volume_scatter_info().tobytes() == info.tobytes()      # (nothing above touched the table)
    assert lib.blok_hip_volume_scatter_models(ctx, _ffi.ptr(p), _ffi.ptr(ent), 3, None) == 0      # out_info may be NULL
    assert tr.volume_scatter_download().tobytes() == table.tobytes()
    # a snapshot along another axis or from the low end: refused (and that field freed the table)
    for axis, flags in ((0, 0), (2, 0), (1, R.FROM_LOW)):
        tr.volume_column_field(None, None, axis, flags)
        gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_models, p, ent)
        gone(BLOK_ERR_INVALID_ARG, tr.volume_scatter_info)


# ---- end to end: the table traced where it lies, and stamped -----------------------------------------------------------------------------------
def two_models():
    tree = np.array([(0, y, 0) for y in range(4)] + [(x, 3, z) for x in (-1, 0, 1) for z in (-1, 0, 1) if (x, z) != (0, 0)] + [(1, 4, 0)], np.int32)
    rock = np.array([(x, y, z) for x in range(3) for y in range(2) for z in range(4) if (x + y + z) % 3], np.int32)
    return (tree, (20 + np.arange(len(tree))).astype(np.uint32)), (rock, (60 + np.arange(len(rock))).astype(np.uint32))


def test_the_table_traces_where_it_lies_and_stamps(tr, mats, scene):
    import torch
    d, m = scene
    o = R.SCENE_ORIGIN
    make(tr, True, o, R.SCENE_SHAPE, d, m)
    model = DenseModel(o, R.SCENE_SHAPE)
    model.upload(d, m)
    check(tr, model, "uploaded", mats)                              # (installs the world the frames are traced over)
    models = two_models()
    ids = [tr.model_create(*mm) for mm in models]
    rows = [(ids[0], 5, (0, 0, 0), 0), (ids[1], 2, (1, 0, 2), 1), (ids[0], 1, (-1, 2, 0), -2)]
    p, ent = R.scene_params(cell_log2=2, radius=1, probability=65536), R.entries(rows)
    tr.volume_column_field()
    table = scatter_check(tr, R.field(d, m, o, None, None, 1, 0), p, ent, pieces=False)
    assert len(table) > 20
    assert tr._lib.blok_hip_check_instances(tr._ctx, _ffi.ptr(table), len(table)) == 0, "the caller's check of the downloaded table"
    # traced from where it lies == traced from the downloaded table
    cam = W.camera_look_at((o[0] + 48.0, o[1] + 70.0, o[2] - 30.0), (o[0] + 40.0, o[1] + 14.0, o[2] + 30.0), 60.0, tr.width, tr.height)
    want_hits, want_ids, want_rgba = tr.trace_primary_instanced(cam, table)
    address, n = tr.volume_scatter_device()
    px = tr.width * tr.height
    hits = torch.zeros((px, 4), dtype=torch.int32, device="cuda")
    rgba = torch.zeros(px, dtype=torch.int32, device="cuda")
    inst = torch.zeros(px, dtype=torch.int32, device="cuda")
    tr.trace_primary_instanced_device(cam, address, n, hits.data_ptr(), rgba.data_ptr(), inst.data_ptr())
    torch.cuda.synchronize()
    got_ids = inst.cpu().numpy().view(np.uint32)
    assert hits.cpu().numpy().tobytes() == want_hits.tobytes() and got_ids.tobytes() == want_ids.tobytes()
    assert rgba.cpu().numpy().tobytes() == want_rgba.tobytes()
    assert int((got_ids != _ffi.INSTANCE_NONE).sum()) > 50 and len(set(got_ids.tolist())) > 5, "the frame shows scattered models"
    # stamped: the arrays stamp_reference predicts, then the rebuilt tree
    n_written = tr.volume_stamp_models(table, _ffi.STAMP_SET, 1.25)
    n_model = 0
    for rec in table:
        which = ids.index(int(rec["model"]))
        n_model += SR.stamp(model.density, model.ids, o, *models[which], (tuple(int(v) for v in rec["offset"]), tuple(int(a) for a in rec["axis"]), int(rec["flip"])),
                            SR.SET, 1.25)
    assert n_written == n_model > 0
    check(tr, model, "stamped", mats)
    for i in ids:
        tr.model_destroy(i)
