"""GPU: the mixed lives of tests/volume_life.py on the device, one HipTracer and one volume per life, in both brick layouts.  What the
families share — brick masks that seven readers read without a rebuild, edit logs pooled between two rebuilds, the incremental gather of
material ids, the snapshots that live in the context together and follow or leave a scrolled box — is crossed here: after every writer the
returned count or info and the whole download equal the model's, after every reader its snapshot or records equal the reference's in the
form the family's own test compares, at every scheduled rebuild (and at no other time) the tree equals reference_tree byte for byte, and
at the end every snapshot still held is downloaded once more and every dropped one is refused.  And behind every rebuild the shadow
rays' last-occluder map, which is kept across rebuilds and raised only where the pooled edits say they may have filled something, is held
against tests/bounds_reference.py as numbers (tests/test_sun_map_gpu.py: Verdict): valid always, tight behind a pool that holds a scroll
or an upload, and there at all exactly when the world holds a voxel; the texels a kept map would have left too low are counted and
printed.  tests/test_volume_life_cpu.py proves on the CPU that the schedules cross what they claim to cross, and that every life has
rebuilds at which a map kept as it was would be too low.  Measured on an MI355X over the six lives in both layouts: no texel more than
1.2e-5 voxel (0.05 delta) beyond its bound; behind an upload up to 3815 texels of the map held before lie below the new lower bound.

Covered now: the map the path-traced frames' shadow rays read.  Not covered: the traced frames themselves, volumes above this box, several
GPUs, timings."""
from __future__ import annotations

import time

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import affine as A
from blok_amd import scroll as S
from blok_amd import stamp as ST
from blok_amd import world as W
from tests import bounds_reference as BO
from tests import bricks_reference as BR
from tests import lod_reference as LR
from tests import shapes_reference as SHR
from tests import volume_life as VL
from tests.conftest import SEED
from tests.test_columns_gpu import field_check as columns_check
from tests.test_components_gpu import labelled_equals, snapshot_equals
from tests.test_distance_gpu import field_check as distance_check
from tests.test_flood_gpu import field_check as flood_check
from tests.test_lod_gpu import planes_of, reduce_check
from tests.test_quads_gpu import _same as same_quads
from tests.test_scroll_gpu import no_snapshot
from tests.test_stamp_gpu import arrays_equal, captured_equals_created, tree_equal
from tests.test_sun_map_gpu import Verdict
from tests.test_sweep_gpu import as_tuples
from tests.test_volume_limits_gpu import component_equals_created

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
LIVES = pytest.mark.parametrize("index", range(VL.N_LIVES))


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def terrain_params(d):
    p = _ffi.TerrainParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def placements(table, ids):
    return np.concatenate([ST.placement(*place, model=ids[name]) for name, place in table])


def same_model(t, got, xyz, mm, tag):
    """The model `got` is the model model_create builds from the reference's list."""
    want = t.model_create(xyz, mm)
    gn, gm, gi = t.model_download(got)
    wn, wm, wi = t.model_download(want)
    assert gi == wi and gn.tobytes() == wn.tobytes() and gm.tobytes() == wm.tobytes(), (tag, gi, wi)


def scatter_equals(t, table, counts, tag):
    assert t.volume_scatter_info().tobytes() == counts.tobytes() and t.volume_scatter_download().tobytes() == table.tobytes(), tag


# ---- one reader on the device, against the reference's result `want` ----------------------------------------------------------------------
def read(t, ids, family, a, want, before, tag):
    d, m, origin = before
    if family == "distance":
        distance_check(t, want, a["lo"], a["hi"], a["radius"], a["flags"], pieces=False)
    elif family == "flood":
        flood_check(t, want, a["lo"], a["hi"], a["seeds"], a["K"], a["flags"], a["material"], pieces=False, tag=tag)
    elif family == "columns":
        columns_check(t, want[:3], a["lo"], a["hi"], a["axis"], a["flags"], pieces=False, tag=tag)
        if len(want) == 5:
            assert t.volume_scatter_models(*VL.SCATTER).tobytes() == want[4].tobytes(), tag
            scatter_equals(t, want[3], want[4], tag)
    elif family == "lod":
        reduce_check(t, want, a["lo"], a["hi"], a["levels"], a["flags"], pieces=False, tag=tag)
        xyz, mm = LR.model_voxels(want[0][0], 1)
        if len(mm):
            got = t.volume_lod_model(1, 1)
            assert t.last_capture_voxels == len(mm), tag
            same_model(t, got, xyz, mm, tag)
    elif family == "bricks":
        info = t.volume_encode_bricks(a["lo"], a["hi"], bool(a["flags"] & BR.FILLED_ONLY))
        assert info.tobytes() == want[0].tobytes() and BR.same_stream(t.volume_bricks_download(), want), tag
    elif family == "quads":
        got = t.volume_extract_quads(a["lo"], a["hi"], a["ignore"])
        assert (len(got), t.last_quad_faces) == (len(want[0]), want[1]) and same_quads(got, want[0]), tag
    elif family == "components":
        labelled_equals(t, d, a["lo"], a["hi"], tag, want, origin=origin)
    elif family == "sweep":
        got = as_tuples(t.volume_sweep_models(placements(a["table"], ids), a["direction"], a["max_distance"], a["flags"]))
        assert got == [tuple(w) for w in want], (tag, got, want)
    else:
        assert family == "capture"
        captured_equals_created(t, d, m, origin, a["lo"], a["hi"], tag)


# ---- one writer on the device; returns what the entry returned, in the form of the reference's result -------------------------------------
def write(t, ids, family, a, want, before, snaps, tag):
    d, m, origin = before
    if family == "upload":
        return t.volume_upload(*VL.content(a["seed"]))
    if family == "set_voxels":
        return t.volume_set_voxels(a["xyz"], a["ids"], a["density"])
    if family == "brush":
        return t.volume_apply_brush(a["centre"], a["radius"], a["value"], a["mode"])
    if family == "voxelize":
        return t.volume_voxelize_mesh(*a["mesh"], material=a["material"], density=a["density"], solid=a["solid"])
    if family == "terrain":
        return t.volume_generate_terrain(terrain_params(a["params"]), a["lo"], a["hi"])
    if family == "stamp_models":
        return t.volume_stamp_models(placements(a["table"], ids), a["mode"], a["value"])
    if family == "stamp_affine":
        records = np.concatenate([A.from_matrix(forward, ids[name]) for name, forward in a["table"]])
        return t.volume_stamp_affine(records, a["lo"], a["hi"], a["mode"], a["value"])
    if family == "apply_shapes":
        return t.volume_apply_shapes(SHR.record(a["shapes"]))
    if family == "capture_cut":
        captured_equals_created(t, d, m, origin, a["lo"], a["hi"], tag, cut=True)
        return want
    if family == "component_cut":
        labels, records = snaps["components"]["want"]
        region = snaps["components"]["args"]
        rec = records[records["label"] == a["label"]][0]
        component_equals_created(t, d.copy(), m.copy(), origin, (labels, region["lo"], region["hi"]), rec, tag, cut=True)
        return want
    if family == "restore":
        if a.get("stream") is None:
            return t.volume_restore_bricks(a["dst"], a["keep_others"])
        return t.volume_decode_bricks(*a["stream"], dst_lo=a["dst"], keep_others=a["keep_others"])
    if family == "edit_by_distance":
        return t.volume_edit_by_distance(a["op"], a["d2"], a["density"], a["material"])
    if family == "edit_by_flood":
        return t.volume_edit_by_flood(a["op"], a["d"], a["density"], a["material"])
    if family == "scroll":
        info = t.volume_scroll(a["delta"])
        counts = []
        if a["terrain"] is not None:
            counts = [t.volume_generate_terrain(terrain_params(a["terrain"]), lo, hi) for lo, hi in S.boxes(info, "exposed")]
        return info, counts
    assert family == "scatter"
    counts = t.volume_scatter_models(*VL.SCATTER)
    return t.volume_scatter_download(), counts


# ---- the snapshots at the end of a life ---------------------------------------------------------------------------------------------------
NO_SNAPSHOT = {"distance": lambda t: no_snapshot(t.volume_distance_info), "flood": lambda t: no_snapshot(t.volume_flood_info),
               "columns": lambda t: (no_snapshot(t.volume_columns_info), no_snapshot(t.volume_scatter_info)),
               "components": lambda t: no_snapshot(t.volume_labels_download, 0, 0)}


def held_equals(t, kind, want, tag):
    if kind == "quads":
        assert same_quads(t.volume_quads_download(0, len(want[0])), want[0]), tag
    elif kind == "bricks":
        assert BR.same_stream(t.volume_bricks_download(), want), tag
    elif kind == "distance":
        assert t.volume_distance_info().tobytes() == want[1].tobytes() and t.volume_distance_download().tobytes() == want[0].tobytes(), tag
    elif kind == "flood":
        assert t.volume_flood_info().tobytes() == want[1].tobytes() and t.volume_flood_download().tobytes() == np.asarray(want[0], np.uint16).tobytes(), tag
    elif kind == "columns":
        assert t.volume_columns_info().tobytes() == want[2].tobytes(), tag
        assert t.volume_columns_download(0).tobytes() == want[0].tobytes() and t.volume_columns_download(1).tobytes() == want[1].tobytes(), tag
        if len(want) == 5:
            scatter_equals(t, want[3], want[4], tag)
    elif kind == "lod":
        assert t.volume_lod_info().tobytes() == want[1].tobytes(), tag
        for got, planes in zip(planes_of(t, len(want[0])), want[0]):
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, planes)), tag
    else:
        snapshot_equals(t, *want, tag)


# ---- the shadow rays' last-occluder map behind a rebuild -----------------------------------------------------------------------------------
def map_before(t):
    """(info, texels) of the map as it lies before a rebuild, or None when there is none."""
    info, texels = t.sun_map()
    return (info[0], texels) if int(info["has_map"][0]) else None


def map_holds(t, life, held, pool, tag):
    """Behind a rebuild: the map is there exactly when the world holds a voxel, valid against the model's voxels, tight when the pooled
    writers made it a new world to the map.  Prints how many texels of the map held before would now be too low."""
    n_voxels = int(t.world_stats().n_voxels)
    info = t.sun_map(want_map=False)[0]
    assert int(info["has_map"][0]) == (1 if n_voxels > 0 else 0), (tag, n_voxels)
    if not n_voxels:
        return
    with np.errstate(invalid="ignore"):
        v = Verdict(t, BO.voxels_of(life.d > 0, life.origin))
    v.report(tag)
    v.assert_valid(tag)
    if {"scroll", "upload"} & set(pool):
        v.assert_tight(tag + ": a new world to the map")
    same_frame = held is not None and all(np.array_equal(held[0][k], v.info[k]) for k in ("u", "v", "s", "u0", "v0", "texel", "nu", "nv"))
    if same_frame:
        low = int((held[1].astype(np.float64) < v.lo - v.delta).sum())
        print(f"[sun map] {tag}: behind {sorted(set(pool))}, {low} texels of the map held before the rebuild lie below the new lower bound")
    else:
        print(f"[sun map] {tag}: behind {sorted(set(pool))}, " + ("no map was held before" if held is None else "the map is laid out anew"))


@LAYOUTS
@LIVES
def test_a_life_on_the_device_equals_the_model(index, keyed, mats):
    from blok_amd.tracer import HipTracer
    t0 = time.perf_counter()
    steps = VL.schedule(index, keyed)
    t = HipTracer(64, 64).init()
    try:
        t.set_volume_layout(keyed)
        t.volume_create(VL.ORIGIN, VL.SHAPE)
        t.volume_upload(*VL.content())
        ids = {name: t.model_create(*model) for name, model in VL.MODELS.items()}
        device = 0.0
        snaps = {}
        pool = ["upload"]                                          # the writers since the last rebuild: the first finds the upload above
        for i, step, before, life, want in VL.replay(steps):
            tag = VL.label(index, i, step) + (", keyed" if keyed else ", general")
            t1 = time.perf_counter()
            if step["kind"] == "rebuild":
                held = map_before(t)
                tree_equal(t, life.d, life.m, life.origin, mats, tag)
                map_holds(t, life, held, pool, tag)
                pool = []
            elif step["kind"] == "reader":
                read(t, ids, step["family"], step["args"], want, before, tag)
            else:
                got = write(t, ids, step["family"], step["args"], want, before, snaps, tag)
                assert VL.norm(got) == VL.norm(want), f"{tag}: the entry returned {got}, the reference {want}"
                arrays_equal(t, life.d, life.m, tag)
                assert tuple(t.volume_scroll((0, 0, 0))["origin"][0].tolist()) == life.origin, tag
                pool.append(step["family"])
            device += time.perf_counter() - t1
            snaps = dict(life.snaps)
        for kind in VL.KINDS:
            tag = f"life {index}, at the end: the {kind} snapshot" + (", keyed" if keyed else ", general")
            held = life.snaps.get(kind)
            if held is VL.DROPPED:
                NO_SNAPSHOT[kind](t)
            elif held is not None:
                held_equals(t, kind, held["want"], tag)
        arrays_equal(t, life.d, life.m, f"life {index}, at the end")
        held = map_before(t)
        tree_equal(t, life.d, life.m, life.origin, mats, f"life {index}, the final rebuild")
        map_holds(t, life, held, pool, f"life {index}, the final rebuild" + (", keyed" if keyed else ", general"))
        print(f"life {index} {'keyed' if keyed else 'general'}: {len(steps)} steps, {time.perf_counter() - t0:.2f} s in all, {device:.2f} s in the device's steps")
    finally:
        t.shutdown()
