"""GPU: blok_hip_volume_scroll against the numpy model of the contract (tests/scroll_reference.py), in both brick layouts where the shape
allows.  Every comparison is exact.  After a scroll the download is the model's move of the previous download, the info is the model's,
and PLAN_ONLY said so beforehand and changed nothing; what lies above the dense arrays — masks, occupancy words, dirty flags — is checked
through what reads it: the rebuilt tree against an independent build, the column field and the components (which read the masks with no
rebuild in between), and frames against a volume created where the box now is.  The snapshots follow the box or are dropped."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import columns_reference as CR
from tests import components_reference as KR
from tests import distance_reference as DR
from tests import flood_reference as FR
from tests import limit_cases as LC
from tests import scroll_reference as R
from tests import terrain_cases as TC
from tests.conftest import SEED
from tests.test_volume_rebuild_gpu import Pair, check
from tests.volume_tree_reference import DenseModel

pytestmark = pytest.mark.gpu

FW, FH = 96, 64
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
BOXES = pytest.mark.parametrize("box", [R.SMALL, R.MID], ids=["13x10x7", "72x40x24"])


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(FW, FH).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def make(tr, keyed, origin, dims, d=None, m=None):
    tr.set_volume_layout(keyed)
    tr.volume_create(origin, dims, 128, 1.0)
    if d is not None:
        tr.volume_upload(d, m)


def add(origin, delta):
    return tuple(o + s for o, s in zip(origin, delta))


def same_arrays(got, want, tag):
    assert got[0].tobytes() == want[0].tobytes(), (tag, "density")
    assert got[1].tobytes() == want[1].tobytes(), (tag, "ids")


def scroll_checked(tr, d, m, origin, delta, download_before=True):
    """One scroll of a volume that holds (d, m) at `origin`, with the contract's checks; returns the model's arrays and the new origin."""
    want = R.info(d, m, origin, delta)
    planned = tr.volume_scroll(delta, plan_only=True)
    assert planned.tobytes() == want.tobytes(), (delta, "plan", planned, want)
    assert tr.volume_scroll((0, 0, 0)).tobytes() == R.info(d, m, origin, (0, 0, 0)).tobytes(), (delta, "the plan moved the box")
    if download_before:
        same_arrays(tr.volume_download(), (d, m), (delta, "the plan wrote"))
    got = tr.volume_scroll(delta)
    assert got.tobytes() == want.tobytes(), (delta, "info", got, want)
    moved = R.scroll(d, m, delta)
    same_arrays(tr.volume_download(), moved, delta)
    return moved[0], moved[1], add(origin, delta)


def columns_equal(tr, d, m, origin, tag):
    """The column field of the whole box along every axis, from the masks as the scroll left them, against the model of the arrays."""
    for axis in range(3):
        top, material, info = CR.field(d, m, origin, None, None, axis, 0)
        got = tr.volume_column_field(None, None, axis, 0)
        assert got.tobytes() == info.tobytes(), (tag, axis, got, info)
        assert tr.volume_columns_download(0).tobytes() == top.tobytes(), (tag, axis, "tops")
        assert tr.volume_columns_download(1).tobytes() == material.tobytes(), (tag, axis, "materials")


def components_equal(tr, d, origin, tag):
    labels, records = KR.label(d, origin)
    n, voxels = tr.volume_label_components()
    assert (n, voxels) == (len(records), int(records["n_voxels"].sum())), tag
    assert tr.volume_labels_download(0, labels.size).tobytes() == labels.tobytes(), (tag, "labels")
    assert tr.volume_components_download(0, n).tobytes() == records.tobytes(), (tag, "records")


# ---- the move -----------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@BOXES
def test_every_delta_moves_the_world_cells_and_the_masks(tr, keyed, box):
    dims, origin = box
    d0, m0 = R.noise(dims)
    make(tr, keyed, origin, dims)
    for delta in R.deltas(box):
        tr.volume_upload(d0, m0)
        d, m, origin = scroll_checked(tr, d0, m0, origin, delta)
        columns_equal(tr, d, m, origin, delta)
        if box == R.SMALL:
            components_equal(tr, d, origin, delta)


@LAYOUTS
@pytest.mark.parametrize("which", ["LOW", "HIGH"])
def test_limit_boxes_scroll_off_the_lattices_end_and_back_onto_it(tr, keyed, which):
    dims = LC.SHAPE
    origin = LC.limit_origin(which, dims)
    sign = 1 if which == "LOW" else -1
    d, m = R.noise(dims, seed=9)
    make(tr, keyed, origin, dims, d, m)
    for delta in ((4 * sign, 0, 0), (0, 8 * sign, 4 * sign), (-4 * sign, 0, 0), (0, -8 * sign, -4 * sign)):
        d, m, origin = scroll_checked(tr, d, m, origin, delta, download_before=False)
    assert origin == LC.limit_origin(which, dims)              # it ends exactly on the lattice's end again: fine; one brick further is refused
    columns_equal(tr, d, m, origin, which)
    for a in range(3):
        delta = [0, 0, 0]
        delta[a] = -4 * sign
        for plan_only in (True, False):
            with pytest.raises(BlokError) as e:
                tr.volume_scroll(delta, plan_only)
            assert e.value.status == R.UNSUPPORTED
    same_arrays(tr.volume_download(), (d, m), "refused")


@pytest.mark.parametrize("box", LC.LONG_BOXES, ids=LC.LONG_IDS)
def test_long_boxes_scroll_along_their_long_axis(tr, mats, box):
    d, m = LC.sparse_fill(box)
    origin = box.origin
    make(tr, True, origin, box.shape, d, m)
    for step in (8192, LC.L - 4):
        delta = [0, 0, 0]
        delta[box.axis] = step if origin[box.axis] + LC.L + step <= R.LATTICE_HI else -step      # towards the inside of the lattice
        assert origin[box.axis] + delta[box.axis] >= R.LATTICE_LO
        d, m, origin = scroll_checked(tr, d, m, origin, tuple(delta), download_before=False)
        model = DenseModel(origin, box.shape)
        model.upload(d, m)
        check(tr, model, (box.name, step), mats)
        assert 0 < int(R.filled(d).sum())
        delta[box.axis] = -delta[box.axis]                         # and back: what left is gone
        d, m, origin = scroll_checked(tr, d, m, origin, tuple(delta), download_before=False)
        tr.volume_upload(*LC.sparse_fill(box))
        d, m = LC.sparse_fill(box)


# ---- masks and everything above them: the rebuilt tree ----------------------------------------------------------------------------------------
def moved_model(model, delta):
    out = DenseModel(add(model.origin, delta), model.shape_xyz)
    out.upload(*R.scroll(model.density, model.ids, delta))
    return out


@LAYOUTS
@BOXES
def test_rebuilds_around_scrolls_equal_an_independent_build(tr, mats, keyed, box):
    dims, origin = box
    p = Pair(tr, origin, dims, keyed, mats)
    p.upload(*R.noise(dims))
    p.check("uploaded")                                        # the rebuild that arms the stale-id path: every brick has a place in this build's ids
    centre = [o + n / 2 for o, n in zip(origin, dims)]
    p.brush(centre, 2.5, 0.8, 0)
    tr.volume_scroll((-4, 0, 4))
    p.model = moved_model(p.model, (-4, 0, 4))
    p.check("scrolled behind a rebuild and a brush")
    info = tr.volume_scroll((8, -4, 0))                        # again, with no rebuild in between, and edits inside what came into view
    p.model = moved_model(p.model, (8, -4, 0))
    lo, hi = (np.array(c) for c in R.plan(add(origin, (-4, 0, 4)), dims, (8, -4, 0))["exposed"][-1])      # the x slab, 8 cells thick
    assert info["n_exposed"][0] == 2 and tuple(info["exposed"][0, 1]["lo"]) == tuple(lo)
    corners = [[x, y, z] for z in (lo[2], hi[2] - 1) for y in (lo[1], hi[1] - 1) for x in (lo[0], hi[0] - 1)]
    p.set_voxels(corners, np.arange(31, 39), np.linspace(0.5, 1.2, 8))
    p.brush([lo[0] + 4.0, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2], 2.5, 0.9, 0)
    p.check("edited inside an exposed box")
    tr.volume_scroll(R.GONE[box])
    p.model = moved_model(p.model, R.GONE[box])
    p.check("everything left")


# ---- frames -----------------------------------------------------------------------------------------------------------------------------------
def frames(tr, cam):
    hits = tr.draw_frame(cam)
    planes = tr.trace_paths(cam, spp=2, max_bounces=2, frame_index=3)
    return hits.tobytes(), {k: v.tobytes() for k, v in planes.items()}


@LAYOUTS
def test_frames_show_the_old_world_until_the_rebuild_then_the_moved_one(tr, mats, keyed):
    dims, origin = R.MID
    d, m = R.noise(dims)
    m = np.where(R.filled(d), 1 + m % 200, m).astype(np.uint32)
    delta = (8, -4, 4)
    centre = [o + n / 2 for o, n in zip(origin, dims)]
    cam = W.camera_look_at([centre[0] + 20.0, centre[1] + 70.0, centre[2] + 35.0], centre, 60.0, FW, FH)
    make(tr, keyed, origin, dims, d, m)
    tr.volume_rebuild(mats)
    tr.draw_frame(cam)
    at_rest = tr.draw_frame(cam)                               # the second frame of a view at rest
    assert int(at_rest["hit"].astype(bool).sum()) > 0
    tr.volume_scroll(delta)
    assert tr.draw_frame(cam).tobytes() == at_rest.tobytes(), "the installed world changed before the rebuild"
    tr.volume_rebuild(mats)
    got = frames(tr, cam)
    make(tr, keyed, add(origin, delta), dims, *R.scroll(d, m, delta))
    tr.volume_rebuild(mats)
    want = frames(tr, cam)
    assert got[0] == want[0], "first hits"
    for k in want[1]:
        assert got[1][k] == want[1][k], k
    assert got[0] != at_rest.tobytes(), "the camera sees what left"


# ---- the terrain seam -------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_terrain_generated_into_the_exposed_boxes_is_seamless(tr, keyed):
    dims, origin, delta = (64, 48, 64), (-40, -44, 16), (8, 0, -12)
    params, _ = TC.params()
    make(tr, keyed, origin, dims)
    assert tr.volume_generate_terrain(params) > 0
    info = tr.volume_scroll(delta)
    assert info["n_exposed"][0] == 2 and 0 < info["n_filled_kept"][0] < info["n_filled_before"][0]
    from blok_amd import scroll as S
    for lo, hi in S.boxes(info, "exposed"):
        tr.volume_generate_terrain(params, lo, hi)
    got = tr.volume_download()
    columns = (tr.volume_column_field().tobytes(), tr.volume_columns_download(0).tobytes(), tr.volume_columns_download(1).tobytes())
    make(tr, keyed, add(origin, delta), dims)
    tr.volume_generate_terrain(params)
    same_arrays(got, tr.volume_download(), "a fresh box generated whole")
    assert columns == (tr.volume_column_field().tobytes(), tr.volume_columns_download(0).tobytes(), tr.volume_columns_download(1).tobytes())


# ---- snapshots ------------------------------------------------------------------------------------------------------------------------------
STAYS, CUTS = (8, -4, 4), (24, 0, 0)                            # for the region below in the MID box: wholly inside afterwards / cut by the new box
REGION_LO, REGION_HI = (0, 12, -8), (20, 30, 6)               # world voxels


def no_snapshot(fn, *args):
    with pytest.raises(BlokError) as e:
        fn(*args)
    assert e.value.status == R.INVALID_ARG


def snapshot_volume(tr, keyed):
    dims, origin = R.MID
    d, m = R.noise(dims, seed=21)
    make(tr, keyed, origin, dims, d, m)
    for delta in (STAYS, CUTS):
        new = add(origin, delta)
        stays = all(n <= l and h <= n + e for n, e, l, h in zip(new, dims, REGION_LO, REGION_HI))
        assert stays == (delta == STAYS)
    return d, m, origin


@LAYOUTS
def test_the_brick_stream_stays_where_it_was_taken(tr, keyed):
    d, m, origin = snapshot_volume(tr, keyed)
    tr.volume_encode_bricks(REGION_LO, REGION_HI)
    stream = [a.tobytes() for a in tr.volume_bricks_download()]
    quads = tr.volume_extract_quads(REGION_LO, REGION_HI)
    d, m, origin = scroll_checked(tr, d, m, origin, STAYS)
    cells = np.array([[x, y, z] for z in range(REGION_LO[2], REGION_HI[2]) for y in range(REGION_LO[1], REGION_HI[1]) for x in range(REGION_LO[0], REGION_HI[0])])
    tr.volume_set_voxels(cells, np.zeros(len(cells), np.uint32), np.zeros(len(cells), np.float32))
    cleared = tr.volume_download()
    l = [a - o for a, o in zip(REGION_LO, origin)]
    h = [a - o for a, o in zip(REGION_HI, origin)]
    assert not cleared[0][l[2]:h[2], l[1]:h[1], l[0]:h[0]].any()
    tr.volume_restore_bricks(None)                             # "where it was taken": the same world cells come back
    same_arrays(tr.volume_download(), (d, m), "restored")
    d, m, origin = scroll_checked(tr, d, m, origin, CUTS)
    with pytest.raises(BlokError) as e:
        tr.volume_restore_bricks(None)
    assert e.value.status == R.UNSUPPORTED
    same_arrays(tr.volume_download(), (d, m), "a refused restore wrote")
    assert [a.tobytes() for a in tr.volume_bricks_download()] == stream, "the stream is kept"
    assert tr.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes(), "the quads hold no position and stay"


@LAYOUTS
def test_the_distance_field_follows_the_box_or_is_dropped(tr, keyed):
    d, m, origin = snapshot_volume(tr, keyed)
    dist, info = DR.field(d, origin, REGION_LO, REGION_HI, 3, 0)
    assert tr.volume_distance_field(REGION_LO, REGION_HI, 3).tobytes() == info.tobytes()
    d, m, origin = scroll_checked(tr, d, m, origin, STAYS)
    assert tr.volume_distance_info().tobytes() == info.tobytes() and tr.volume_distance_download().tobytes() == dist.tobytes()
    d, m = d.copy(), m.copy()
    n = DR.edit(d, m, dist, info, DR.GROW, 4, 1.25, 6, origin)
    assert n > 0 and tr.volume_edit_by_distance(DR.GROW, 4, 1.25, 6) == n
    same_arrays(tr.volume_download(), (d, m), "grown at the same world cells")
    scroll_checked(tr, d, m, origin, CUTS)
    no_snapshot(tr.volume_distance_info)
    no_snapshot(tr.volume_edit_by_distance, DR.GROW, 1)


@LAYOUTS
def test_the_flood_field_follows_the_box_or_is_dropped(tr, keyed):
    d, m, origin = snapshot_volume(tr, keyed)
    flags = FR.seed_face(2)
    steps, info = FR.field(d, m, origin, REGION_LO, REGION_HI, np.zeros((0, 3), np.int32), 12, flags)
    assert tr.volume_flood_field(REGION_LO, REGION_HI, None, 12, flags).tobytes() == info.tobytes()
    d, m, origin = scroll_checked(tr, d, m, origin, STAYS)
    assert tr.volume_flood_info().tobytes() == info.tobytes() and tr.volume_flood_download().tobytes() == np.asarray(steps, np.uint16).tobytes()
    d, m = d.copy(), m.copy()
    n = FR.edit(d, m, steps, info, FR.FILL, 3, np.float32(1.5), 9, origin)
    assert n > 0 and tr.volume_edit_by_flood(FR.FILL, 3, 1.5, 9) == n
    same_arrays(tr.volume_download(), (d, m), "filled at the same world cells")
    scroll_checked(tr, d, m, origin, CUTS)
    no_snapshot(tr.volume_flood_info)
    no_snapshot(tr.volume_edit_by_flood, FR.FILL, 1)


@LAYOUTS
def test_the_components_follow_the_box_or_are_dropped(tr, keyed):
    d, m, origin = snapshot_volume(tr, keyed)
    labels, records = KR.label(d, origin, REGION_LO, REGION_HI)
    assert tr.volume_label_components(REGION_LO, REGION_HI)[0] == len(records)
    d, m, origin = scroll_checked(tr, d, m, origin, STAYS)
    assert tr.volume_labels_download(0, labels.size).tobytes() == labels.tobytes() and tr.volume_components_download(0, len(records)).tobytes() == records.tobytes()
    big = records[int(np.argmax(records["n_voxels"]))]
    _, at = tr.volume_capture_component(int(big["label"]), cut=True)
    assert at == tuple(int(c) for c in big["lo"]) and tr.last_capture_voxels == int(big["n_voxels"])
    d, m = d.copy(), m.copy()
    KR.clear_members(d, m, origin, (labels, REGION_LO, REGION_HI), big)
    same_arrays(tr.volume_download(), (d, m), "cut at the same world cells")
    scroll_checked(tr, d, m, origin, CUTS)
    no_snapshot(tr.volume_labels_download, 0, 0)
    no_snapshot(tr.volume_capture_component, int(big["label"]))


@LAYOUTS
def test_the_columns_and_their_scatter_table_follow_the_box_or_are_dropped(tr, keyed):
    d, m, origin = snapshot_volume(tr, keyed)
    top, material, info = CR.field(d, m, origin, REGION_LO, REGION_HI, 1, 0)
    assert tr.volume_column_field(REGION_LO, REGION_HI, 1, 0).tobytes() == info.tobytes()
    p, ent = CR.params(seed=5, flags=_ffi.SCATTER_ANY_MATERIAL, cell_log2=1), CR.entries([(1, 3, (0, 0, 0), 0), (2, 1, (1, 0, 1), 1)])
    table, counts = CR.scatter(top, material, info, p, ent)
    assert len(table) > 0 and tr.volume_scatter_models(p, ent).tobytes() == counts.tobytes()
    d, m, origin = scroll_checked(tr, d, m, origin, STAYS)
    assert tr.volume_columns_info().tobytes() == info.tobytes()
    assert tr.volume_columns_download(0).tobytes() == top.tobytes() and tr.volume_columns_download(1).tobytes() == material.tobytes()
    assert tr.volume_scatter_info().tobytes() == counts.tobytes() and tr.volume_scatter_download().tobytes() == table.tobytes()
    assert tr.volume_scatter_models(p, ent).tobytes() == counts.tobytes() and tr.volume_scatter_download().tobytes() == table.tobytes()
    scroll_checked(tr, d, m, origin, CUTS)
    no_snapshot(tr.volume_columns_info)
    no_snapshot(tr.volume_scatter_info)
    no_snapshot(tr.volume_scatter_models, p, ent)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_the_error_table_leaves_the_volume_its_origin_and_the_snapshots(tr, keyed):
    d, m, origin = snapshot_volume(tr, keyed)
    dims = R.MID[0]
    distance = tr.volume_distance_field(REGION_LO, REGION_HI, 2).tobytes()
    bricks = tr.volume_encode_bricks(REGION_LO, REGION_HI).tobytes()
    columns = tr.volume_column_field(REGION_LO, REGION_HI).tobytes()
    lib, ctx = tr._lib, tr._ctx
    out = np.full(1, 0, dtype=_ffi.SCROLL_INFO)
    for delta, flags, status in R.refusals(origin, dims):
        for extra in (0, _ffi.SCROLL_PLAN_ONLY):
            if flags & _ffi.SCROLL_PLAN_ONLY and extra:
                continue
            vec = None if delta is None else (np.ctypeslib.ctypes.c_int32 * 3)(*delta)
            assert lib.blok_hip_volume_scroll(ctx, vec, flags | extra, _ffi.ptr(out)) == status, (delta, flags, extra)
            assert not out.tobytes().strip(b"\0"), "a refusal wrote the info"
        assert tr.volume_scroll((0, 0, 0))["origin"][0].tolist() == list(origin)
        same_arrays(tr.volume_download(), (d, m), (delta, flags))
        assert tr.volume_distance_info().tobytes() == distance and tr.volume_bricks_info().tobytes() == bricks and tr.volume_columns_info().tobytes() == columns
    assert lib.blok_hip_volume_scroll(ctx, (np.ctypeslib.ctypes.c_int32 * 3)(4, 0, 0), 0, None) == 0      # out_info may be NULL
    assert tr.volume_scroll((0, 0, 0))["origin"][0].tolist() == list(add(origin, (4, 0, 0)))
    tr.volume_destroy()
    with pytest.raises(BlokError) as e:
        tr.volume_scroll((4, 0, 0))
    assert e.value.status == R.NO_WORLD
