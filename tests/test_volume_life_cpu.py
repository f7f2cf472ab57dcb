"""CPU: the mixed lives of tests/volume_life.py before a GPU is involved.  The schedules meet their conditions (asserted from the schedule
and the numpy references alone): every writer family followed by every reader family with no rebuild in between and with a result the write
changed, every writer family in a pool of several families' edits before one rebuild, a rebuild behind a scroll and a later small edit,
every deferred consumer across a kept scroll and across writes into its region, every snapshot kind held with all the others, whole bricks
emptied and bricks filled in an empty 64-cell in every life, and at least two rebuilds per life at which the shadow rays' last-occluder
map, had it been kept as it was, would be too low (what tests/test_volume_life_gpu.py checks on the device can fail).  And the host builds of libblok_host.so, driven through the same lives from
the model's arrays, return what the composed references return, exactly.  The measured seconds per life are printed."""
from __future__ import annotations

import time

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import affine as A
from blok_amd import bricks as B
from blok_amd import columns as COL
from blok_amd import components as K
from blok_amd import distance as D
from blok_amd import flood as F
from blok_amd import lod as L
from blok_amd import mesh as M
from blok_amd import scroll as S
from blok_amd import shapes as SH
from blok_amd import stamp as ST
from blok_amd import sweep as SW
from blok_amd import terrain as T
from tests import bounds_reference as BO
from tests import shapes_reference as SHR
from tests import volume_life as VL

LIVES = pytest.mark.parametrize("index", range(VL.N_LIVES))
SMALL_EDITS = ("set_voxels", "brush")
MODES = ["stamp_models SET", "stamp_models KEEP", "stamp_models ERASE", "stamp_affine SET", "stamp_affine KEEP", "stamp_affine ERASE",
         "GROW", "SHRINK", "HOLLOW", "edit_by_flood FILL", "FILL_UNREACHED", "edit_by_flood PAINT", "edit_by_flood CLEAR",
         "terrain solid", "shell", "terrain additive", "voxelize surface", "voxelize solid",
         "restore_bricks in place", "restore_bricks moved off the brick grid", "decode_bricks of a host stream", "with terrain", "SET the twin"]


def region_slices(origin, lo, hi):
    return tuple(slice(lo[a] - origin[a], hi[a] - origin[a]) for a in (2, 1, 0))


@pytest.fixture(scope="module")
def facts():
    """What each life's schedule does, from one replay of each on the model: per life a dict of the conditions' evidence."""
    out = []
    for index in range(VL.N_LIVES):
        t0 = time.perf_counter()
        steps = VL.schedule(index)
        t1 = time.perf_counter()
        f = dict(pairs=set(), pooled=set(), rebuild_behind_scroll_and_edit=False, deferred={c: set() for c in VL.CONSUMERS}, all_held=False,
                 emptied=0, filled_empty_cell=0, tags=[s["tag"] for s in steps], shapes=set(), deltas=set(), steps=steps)
        pool, last_writer, since = [], None, {}
        for i, step, before, life, want in VL.replay(steps):
            tag = VL.label(index, i, step)
            if step["kind"] == "rebuild":
                if len(set(pool)) >= 2:
                    f["pooled"] |= set(pool)
                if "scroll" in pool and any(w in SMALL_EDITS for w in pool[pool.index("scroll") + 1:]):
                    f["rebuild_behind_scroll_and_edit"] = True
                pool, last_writer = [], None
            elif step["kind"] == "reader":
                if step["family"] in VL.KEEPS_A_SNAPSHOT:
                    since[step["family"]] = dict(writers=0, kept_scroll=False, written_inside=False)
                if "pair" in step or step.get("equality_only"):
                    assert last_writer is not None, f"{tag}: a rebuild lies between the writer and this reader"
                    stale = VL.norm(VL.READ[step["family"]](last_writer["before"][0], last_writer["before"][1], life.origin, **step["args"]))
                    if step.get("equality_only"):
                        assert last_writer["step"].get("ids_only") and stale == VL.norm(want), f"{tag}: ids changed under it, nothing it reads"
                    else:
                        assert step["pair"] == last_writer["step"]["family"], tag
                        assert stale != VL.norm(want), f"{tag}: condition b, the write changed nothing of what this reader returns"
                        assert not last_writer["step"].get("ids_only") or step["family"] in VL.READS_IDS, tag
                        f["pairs"].add((step["pair"], step["family"]))
            else:
                if step["family"] == "scatter":
                    state = since["columns"]
                    assert step["kind"] == "deferred" and state["writers"] >= 2, tag
                    f["deferred"]["scatter"] |= {k for k in ("kept_scroll", "written_inside") if state[k]}
                    continue
                after = (life.d, life.m)
                cells = VL.changed_cells(before[:2], after)
                assert cells.any(), f"{tag}: the writer changed nothing"
                if step.get("ids_only"):
                    assert (VL.filled(before[0]) == VL.filled(life.d)).all(), f"{tag}: not ids only"
                kind = VL.SNAPSHOT_OF.get(step["family"])
                if step["kind"] == "deferred":
                    state = since[kind]
                    assert state["writers"] >= 2, f"{tag}: a deferred consumer acts on a snapshot at least two writers old"
                    f["deferred"][step["family"]] |= {k for k in ("kept_scroll", "written_inside") if state[k]}
                for kind, state in since.items():
                    held = life.snaps.get(kind, VL.DROPPED)
                    if held is VL.DROPPED:
                        continue
                    state["writers"] += 1
                    if step["family"] == "scroll":
                        state["kept_scroll"] = True
                    elif cells[region_slices(life.origin, *life.region_of(kind))].any():
                        state["written_inside"] = True
                f["emptied"] += VL.emptied_bricks(before[0], life.d)
                f["filled_empty_cell"] += VL.bricks_in_an_empty_64_cell(before[0], life.d) if step["family"] != "scroll" else 0
                pool.append(step["family"])
                last_writer = dict(step=step, before=before)
                if step["family"] == "apply_shapes":
                    f["shapes"] |= {(s["kind"], s["op"]) for s in step["args"]["shapes"]}
                if step["family"] == "scroll":
                    f["deltas"] |= {(a, int(np.sign(c))) for a, c in enumerate(step["args"]["delta"]) if c}
            if all(life.snaps.get(k, VL.DROPPED) is not VL.DROPPED for k in VL.KINDS):
                f["all_held"] = True
        f["seconds"] = (t1 - t0, time.perf_counter() - t1)
        out.append(f)
    print("seconds per life (generate, replay):", [tuple(round(s, 2) for s in f["seconds"]) for f in out])
    return out


def test_the_box_keeps_the_properties_it_was_chosen_for():
    """Odd origin, negative in x and y; x crosses a 64-cell boundary of the keyed layout and of the 64-wide tiles; y and z end inside a
    16-cell (52 and 44 are whole bricks, not whole 16-cells); four tree levels, so the keyed layout is taken when allowed."""
    from tests.volume_tree_reference import box_levels
    assert all(o % 2 for o in VL.ORIGIN) and VL.ORIGIN[0] < 0 and VL.ORIGIN[1] < 0
    assert VL.SHAPE[0] > 64 and VL.SHAPE[1] % 16 and VL.SHAPE[2] % 16 and box_levels(VL.SHAPE) == 4
    d, m = VL.content()
    assert np.isnan(d).any() and (d < 0).any() and (d > 0).any()


def deep(x):
    if isinstance(x, dict):
        return tuple((k, deep(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(deep(v) for v in x)
    return x.tobytes() if isinstance(x, np.ndarray) else x


def test_schedules_are_deterministic_and_the_same_in_both_layouts():
    first = [deep(s) for s in VL.schedule(1, True)]
    VL._schedule.cache_clear()
    assert [deep(s) for s in VL.schedule(1, False)] == first


def test_a_every_writer_family_is_followed_by_every_reader_family(facts):
    pairs = set().union(*(f["pairs"] for f in facts))
    missing = [(w, r) for w in VL.WRITERS for r in VL.READERS if (w, r) not in pairs]
    assert not missing, missing                                   # (condition b is asserted where the pairs are collected)
    assert len(pairs) >= len(VL.WRITERS) * len(VL.READERS) == 126


def test_c_every_writer_family_pools_with_another_before_a_rebuild(facts):
    for index, f in enumerate(facts):
        assert f["pooled"] >= set(VL.WRITERS), (index, set(VL.WRITERS) - f["pooled"])


def test_d_a_rebuild_follows_a_scroll_and_a_later_small_edit(facts):
    assert all(f["rebuild_behind_scroll_and_edit"] for f in facts)


def test_e_every_deferred_consumer_crosses_a_kept_scroll_and_writes_into_its_region(facts):
    for consumer in VL.CONSUMERS:
        seen = set().union(*(f["deferred"][consumer] for f in facts))
        assert seen == {"kept_scroll", "written_inside"}, (consumer, seen)


def test_f_every_snapshot_kind_is_held_with_all_the_others(facts):
    assert all(f["all_held"] for f in facts)


def test_g_every_life_empties_whole_bricks_and_fills_an_empty_64_cell(facts):
    for index, f in enumerate(facts):
        assert f["emptied"] > 0 and f["filled_empty_cell"] > 0, (index, f["emptied"], f["filled_empty_cell"])


def test_every_mode_of_every_family_appears(facts):
    tags = [t for f in facts for t in f["tags"]]
    assert not [mode for mode in MODES if not any(mode in t for t in tags)]
    shapes = set().union(*(f["shapes"] for f in facts))
    assert {op for _, op in shapes} == set(SHR.OPS) and {kind for kind, _ in shapes} == set(SHR.KINDS)
    assert set().union(*(f["deltas"] for f in facts)) == {(a, s) for a in range(3) for s in (1, -1)}
    kinds = {s["kind"] for f in facts for s in f["steps"]}
    assert kinds == {"writer", "reader", "rebuild", "deferred"}


@LIVES
def test_h_a_kept_map_would_be_too_low_at_two_rebuilds_of_every_life(index):
    """The map is kept across rebuilds and raised only where the pooled edits say so.  In one frame (bounds_reference.sun_frame over a
    cube that holds every box the life reaches: the box drifts by at most 12 cells) the world at a rebuild is held against the world at
    the rebuild before: where the new lower bound stands above the old upper bound by more than the two deltas, a tight map of the world
    before is too low for the world after, whatever the pool was made of."""
    origin, edge = tuple(c - 16 for c in VL.ORIGIN), 256.0
    assert all(o + 12 + n <= c + edge for o, n, c in zip(VL.ORIGIN, VL.SHAPE, origin))
    info = BO.sun_frame(origin, edge)
    delta = BO.sun_delta(info, np.asarray(origin, dtype=np.float64), edge)
    hi_before, counts = None, []
    for i, step, before, life, want in VL.replay(VL.schedule(index)):
        if step["kind"] != "rebuild":
            continue
        lo, hi = BO.sun_map_bounds(BO.voxels_of(VL.filled(life.d), life.origin), info, delta)
        if hi_before is not None:
            counts.append(int((lo - delta > hi_before + delta).sum()))
        hi_before = hi
    print(f"life {index}: texels a kept map would leave too low, per rebuild after the first: {counts}")
    assert sum(1 for c in counts if c > 0) >= 2, counts


# ---- the host builds through the same lives -------------------------------------------------------------------------------------------------
def terrain_params(d):
    p = _ffi.TerrainParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def host_terrain(d, m, origin, params, lo, hi):
    sl = region_slices(origin, lo, hi)
    d[sl], m[sl], n = T.eval_box(terrain_params(params), lo, hi, d[sl], m[sl])
    return n


def host_columns(d, m, origin, lo, hi, axis, flags):
    top, material, info = COL.column_field_host(d, m, origin, lo, hi, axis, flags)
    if axis == 1 and not flags:
        return top, material, info, *COL.scatter_host(top, material, info, *VL.SCATTER)
    return top, material, info


def host_quads(d, m, origin, lo, hi, ignore):
    records = M.extract_quads_host(d, m, origin, lo, hi, ignore)
    return records, M.extract_quads_host.totals[1]


HOST_READ = {
    "distance": lambda d, m, origin, lo, hi, radius, flags: D.distance_field_host(d, origin, lo, hi, radius, flags),
    "flood": lambda d, m, origin, lo, hi, seeds, K, flags, material: F.flood_field_host(d, m, origin, lo, hi, seeds, K, flags, material),
    "columns": host_columns,
    "lod": lambda d, m, origin, lo, hi, levels, flags: L.reduce_host(d, m, origin, lo, hi, levels, flags),
    "bricks": lambda d, m, origin, lo, hi, flags: B.encode_host(d, m, origin, lo, hi, flags),
    "quads": host_quads,
    "components": lambda d, m, origin, lo, hi: K.label_components_host(d, origin, lo, hi),
    "sweep": lambda d, m, origin, table, direction, max_distance, flags: [
        tuple(int(SW.sweep_voxels_host(d, origin, VL.MODELS[name][0], ST.placement(*place), direction, max_distance, flags)[k]) for k in ("n_overlap", "travel", "blocked"))
        for name, place in table],
    "capture": lambda d, m, origin, lo, hi: ST.capture_voxels_host(d, m, origin, lo, hi),
}


def host_write(family, d, m, origin, snaps, args):
    """The host build of one writer on (d, m), in place where it writes in place.  Returns (result, d, m, origin), or None when the family
    has no host build (upload, set_voxels, brush, voxelize and the two CUTs are the model's own or a device entry's)."""
    if family == "terrain":
        return host_terrain(d, m, origin, **args), d, m, origin
    if family == "stamp_models":
        n = sum(ST.stamp_voxels_host(d, m, origin, *VL.MODELS[name], ST.placement(*place), args["mode"], args["value"]) for name, place in args["table"])
        return n, d, m, origin
    if family == "stamp_affine":
        n = sum(A.stamp_affine_host(d, m, origin, *VL.MODELS[name], VL.affine_record(forward), args["lo"], args["hi"], args["mode"], args["value"])
                for name, forward in args["table"])
        return n, d, m, origin
    if family == "apply_shapes":
        return SH.apply_host(d, m, origin, SHR.record(args["shapes"])), d, m, origin
    if family == "restore":
        stream = snaps["bricks"]["want"] if args.get("stream") is None else args["stream"]
        B.decode_host(d, m, origin, *stream, args["dst"], B.KEEP_OTHERS if args["keep_others"] else 0)
        return None, d, m, origin
    if family == "edit_by_distance":
        return D.distance_edit_host(d, m, origin, *snaps["distance"]["want"], args["op"], args["d2"], args["density"], args["material"]), d, m, origin
    if family == "edit_by_flood":
        return F.flood_edit_host(d, m, origin, *snaps["flood"]["want"], args["op"], args["d"], args["density"], args["material"]), d, m, origin
    if family == "scroll":
        d, m, info = S.scroll_voxels_host(d, m, origin, args["delta"])
        new = tuple(o + s for o, s in zip(origin, args["delta"]))
        counts = []
        if args["terrain"] is not None:
            counts = [host_terrain(d, m, new, args["terrain"], lo, hi) for lo, hi in S.boxes(info, "exposed")]
        return (info, counts), d, m, new
    if family == "scatter":
        return COL.scatter_host(*snaps["columns"]["want"][:3], *VL.SCATTER), d, m, origin
    return None


@LIVES
def test_the_host_builds_live_the_same_lives(index):
    driven = set()
    snaps_before = {}
    for i, step, before, life, want in VL.replay(VL.schedule(index)):
        tag = VL.label(index, i, step)
        d, m, origin = before[0].copy(), before[1].copy(), before[2]
        if step["kind"] == "reader":
            got = HOST_READ[step["family"]](d, m, origin, **step["args"])
            assert VL.norm(got) == VL.norm(want), f"{tag}: the host build and the reference differ"
            driven.add(step["family"])
        elif step["kind"] in ("writer", "deferred"):
            out = host_write(step["family"], d, m, origin, snaps_before, step["args"])
            if out is not None:
                got, d, m, origin = out
                assert VL.norm(got) == VL.norm(want), f"{tag}: counts or info differ, host {got}, reference {want}"
                assert origin == life.origin and d.tobytes() == life.d.tobytes() and m.tobytes() == life.m.tobytes(), f"{tag}: the arrays differ"
                driven.add(step["family"])
            elif step["family"] == "capture_cut":
                assert VL.norm(ST.capture_voxels_host(d, m, origin, **step["args"])) == VL.norm(want), tag
        snaps_before = dict(life.snaps)                            # (a scroll drops what it cuts: the next consumer finds what the model holds)
    assert driven >= set(VL.READERS) | {"terrain", "stamp_models", "stamp_affine", "apply_shapes", "restore", "edit_by_distance", "edit_by_flood", "scroll"}
