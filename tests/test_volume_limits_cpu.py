"""CPU: the volume operations' host builds (include/blok_world.h through blok_amd/*.py) against their numpy references on the cases of
tests/limit_cases.py — the feature tests' scenes in boxes that touch the ends of the int16 lattice, and boxes of 16384 cells on one axis —
byte for byte, and, from the references alone, what makes each of those cases hard, so that none turns easy unnoticed.  The closed forms
of the long boxes are pinned here to the iterative references at limit_cases.LENGTH_PINNED cells.  tests/test_volume_limits_gpu.py runs
the same cases on the device.

The host builds take any int32 placement: that a placement one voxel beyond the lattice is refused is the device entry's rule
(blok_hip_check_instances) and asserted on the GPU; here the reference states that the placement does leave the lattice by one voxel."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import bricks as B
from blok_amd import components as CO
from blok_amd import distance as D
from blok_amd import mesh as M
from blok_amd import stamp as ST
from blok_amd import sweep as SW
from blok_amd import terrain as T
from tests import bricks_reference as BR
from tests import components_reference as CR
from tests import distance_reference as DR
from tests import limit_cases as LC
from tests import oracle_ffi as O
from tests import quads_reference as QR
from tests import stamp_reference as SR
from tests import sweep_reference as SWR
from tests import terrain_reference as TR
from tests import voxelize_reference as VR
from tests.conftest import records_equal
from tests.harness_ffi import HostKernel
from tests.terrain_cases import prior
from tests.test_volume_rebuild_gpu import FH, FW, Pair, boundary_sequence, oracle_frames
from tests.test_voxelize_cpu import shim, shim_voxelize      # noqa: F401  (module fixture)
from tests.volume_tree_reference import box_levels, reference_tree

LIMIT = pytest.mark.parametrize("which", LC.LIMITS)
LONG = pytest.mark.parametrize("box", LC.LONG_BOXES, ids=LC.LONG_IDS)
LO, HI = LC.LATTICE_LO, LC.LATTICE_HI


def bits_equal(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def on_all_six_faces(density):
    return all(LC.faces_filled(density))


# ---- the tables themselves ------------------------------------------------------------------------------------------------------------------
def test_the_boxes_touch_the_lattice_and_the_long_ones_have_seven_levels():
    for shape in (LC.SHAPE, LC.DISTANCE_SHAPE, LC.REBUILD_SHAPE):
        low, high, mixed = (LC.limit_origin(w, shape) for w in LC.LIMITS)
        assert low == (LO, LO, LO) and LC.box_hi(high, shape) == (HI, HI, HI)
        assert mixed[0] == LO and mixed[1] + shape[1] == HI and mixed[2] % 4 != 0
    assert [b.axis for b in LC.LONG_BOXES] == [0, 1, 2]
    for b in LC.LONG_BOXES:
        assert b.length == 16384 and box_levels(b.shape) == 7
    x, y, z = LC.LONG_BOXES
    assert (x.origin[0], x.hi[0]) == (16384, HI) and (y.origin[1], y.hi[1]) == (LO, -16384) and z.origin[2] < 0 < z.hi[2]


# ---- rebuild and edits: the boundary sequence, its frames through the tree-walk kernel body ---------------------------------------------------
def final_state(which):
    p = Pair(None, LC.limit_origin(which, LC.REBUILD_SHAPE), LC.REBUILD_SHAPE)
    boundary_sequence(p)
    p.name_every_filled_voxel()
    return p.model


FLOORS = LC.FRAME_FLOORS                                    # derived there from the counts this test prints


@pytest.mark.parametrize("which", ["LOW", "HIGH"])
def test_kernel_body_frames_of_the_final_states_equal_the_oracle(which):
    model = final_state(which)
    assert on_all_six_faces(model.density)
    z, y, x = np.nonzero(model.filled)
    lo = np.array([x.min(), y.min(), z.min()]) + model.origin
    hi = np.array([x.max(), y.max(), z.max()]) + model.origin
    assert (which == "LOW" and (lo == LO).all()) or (which == "HIGH" and (hi == HI - 1).all())
    ow = O.OracleWorld(128, 1.0)
    ow.set_voxels(np.stack([x, y, z], 1) + np.asarray(model.origin), model.ids[z, y, x])
    ow.rebuild()
    hk = HostKernel(*ow.pack())
    for k, (cam, ref, hits) in enumerate(oracle_frames(model)):
        print(f"{which} camera {k}: oracle hits {hits}, misses {FW * FH - hits}")
        assert hits >= FLOORS[which][k][0] and FW * FH - hits >= FLOORS[which][k][1], (which, k, hits)
        same = records_equal(hk.trace_primary(cam, FW, FH), ref)
        assert same.all(), (which, k, f"{int((~same).sum())} of {len(ref)} records differ, the first at pixel {int(np.flatnonzero(~same)[0])}")


@LONG
def test_long_sparse_fill_is_sparse_and_reaches_both_ends(box):
    d, m = LC.sparse_fill(box)
    f = d > 0
    assert d.shape == box.shape[::-1] and 0.009 < f.mean() < 0.012 and np.isnan(d).any() and (m > 0).all()
    col = np.nonzero(f.any(axis=tuple(k for k in range(3) if k != 2 - box.axis)))[0]
    assert col[0] == 0 and col[-1] == box.length - 1 and len(col) > box.length // 2 and int(np.diff(col).max()) < 16      # filled cells all along the long axis
    nodes, mats = reference_tree(f, m, 7)
    assert len(mats) == int(f.sum()) and len(nodes) > box.length // 4                   # thousands of bricks in a row
    ends = LC.end_voxels(box)
    assert (ends.min(axis=0) == box.origin).all() and (ends.max(axis=0) + 1 == box.hi).all()


# ---- sweep ---------------------------------------------------------------------------------------------------------------------------------
def host_sweep(d, origin, xyz, case):
    _, _, place, direction, max_distance, flags = case[:6]
    r = SW.sweep_voxels_host(d, origin, xyz, ST.placement(*place), direction, max_distance, flags)
    return (int(r["n_overlap"]), int(r["travel"]), int(r["blocked"]))


@LIMIT
def test_sweep_limit_cases_equal_the_reference(which):
    origin = LC.limit_origin(which, LC.SHAPE)
    models = SWR.models()
    lows, highs = [], []
    for scene, d in SWR.scenes().items():
        want = SWR.expected(scene, origin)
        cases = SWR.cases(origin)[scene]
        assert len(cases) == len(SWR.cases()[scene])
        for case, w in zip(cases, want):
            assert host_sweep(d, origin, models[case[1]], case) == w, (scene, case[0])
            lo, hi = LC.world_box(models[case[1]], case[2])
            assert all(LO <= c for c in lo) and all(c <= HI for c in hi), (scene, case[0])
            lows.append(lo); highs.append(hi)
    assert on_all_six_faces(SWR.scenes()["prior"]) and on_all_six_faces(SWR.scenes()["thinned"])
    lows, highs = np.array(lows), np.array(highs)
    for a in range(3):                                          # placements flush against every end of the lattice that the box touches
        assert (lows[:, a] == LO).any() == (origin[a] == LO) and (highs[:, a] == HI).any() == (origin[a] + LC.SHAPE[a] == HI)
    results = [w for scene in SWR.scenes() for w in SWR.expected(scene, origin)]
    assert len(set(results)) >= 100                             # and the cases still tell many answers apart


@LONG
def test_sweep_long_cases_equal_the_reference_and_the_closed_form(box):
    d = LC.sweep_fill(box)
    models = SWR.models()
    cases = LC.sweep_cases(box)
    for case in cases:
        want = case[6]
        assert SWR.sweep(d, box.origin, models[case[1]], case[2], case[3], case[4], case[5]) == want, case[0]
        assert host_sweep(d, box.origin, models[case[1]], case) == want, case[0]
    for direction in (2 * box.axis, 2 * box.axis + 1):          # along both signs of the long axis
        mine = [c for c in cases if c[3] == direction]
        assert any(c[6][1] >= 16000 and c[6][2] == 1 and c[5] == 0 for c in mine)
        assert any(c[4] == LC.FAR and c[6] == (0, LC.FAR, 0) for c in mine)
        assert any(c[5] == SWR.BOX_IS_SOLID and c[6][2] == 1 and c[6][1] == box.length - 6 for c in mine)


# ---- components ----------------------------------------------------------------------------------------------------------------------------
@LIMIT
def test_components_limit_cases_equal_the_reference(which):
    origin = LC.limit_origin(which, LC.SHAPE)
    hi = LC.box_hi(origin, LC.SHAPE)
    for name, (d, m, rlo, rhi) in CR.cases(origin).items():
        labels, records = CR.expected(name, origin)
        got_labels, got_records = CO.label_components_host(d, origin, rlo, rhi)
        assert got_labels.tobytes() == labels.tobytes() and got_records.tobytes() == records.tobytes(), name
        assert CR.cases()[name][0] is d                           # the arrays of the box at ORIGIN
    d = CR.cases(origin)["whole box"][0]
    _, records = CR.expected("whole box", origin)
    assert on_all_six_faces(d)
    for a in range(3):
        assert int(records["lo"][:, a].min()) == origin[a] and int(records["hi"][:, a].max()) == hi[a]
    assert int(np.bitwise_or.reduce(records["touches"])) == 0b111111
    # the components that capture-component and CUT take on the GPU: one of several voxels on every face that is an end of the lattice
    ends = LC.components_at_lattice_ends(records, origin, LC.SHAPE)
    assert [f for f, _ in ends] == {"LOW": [1, 3, 5], "HIGH": [0, 2, 4], "MIXED": [1, 2]}[which]
    for face, rec in ends:
        a = face // 2
        assert int(rec["n_voxels"]) > 1 and (int(rec["hi"][a]) == HI if face % 2 == 0 else int(rec["lo"][a]) == LO)


@LONG
def test_components_long_bars_equal_the_closed_form(box):
    d, m = LC.components_fill(box)
    labels, records = LC.components_expected(box)
    got_labels, got_records = CO.label_components_host(d, box.origin)
    assert got_labels.tobytes() == labels.tobytes() and got_records.tobytes() == records.tobytes()
    # the closed form against the iterative reference where that is fast
    short = box.shortened()
    want = CR.label(LC.components_fill(short)[0], short.origin)
    closed = LC.components_expected(short)
    assert closed[0].tobytes() == want[0].tobytes() and closed[1].tobytes() == want[1].tobytes() and len(want[1]) >= 8
    # what makes it hard
    n, a = box.length, box.axis
    whole = records[records["label"] == box.index(0, *LC.BAR_AT)][0]
    assert int(whole["n_voxels"]) == n and int(whole["lo"][a]) == box.origin[a] and int(whole["hi"][a]) == box.hi[a]
    assert int(whole["touches"]) == (1 << (2 * a)) | (1 << (2 * a + 1))      # both end faces and no other
    gaps = sorted({g % n for g in LC.GAPS})
    pieces = 1 + sum(1 for g0, g1 in zip(gaps, gaps[1:]) if g1 > g0 + 1) + 1      # before the first gap, between gaps that are not neighbours, after the last
    assert len(records) == 1 + pieces == 10
    assert {g % 4 for g in gaps} >= {0, 3} and {g % 64 for g in gaps} >= {0, 63}   # cells either side of brick and 64-cell boundaries
    broken = records[records["label"] != whole["label"]]
    assert int(broken["n_voxels"].sum()) == n - len(gaps) and int(broken["n_voxels"].max()) > 8000      # one piece crosses thousands of bricks


# ---- bricks --------------------------------------------------------------------------------------------------------------------------------
@LIMIT
def test_bricks_limit_scene_equals_the_reference(which):
    origin = LC.limit_origin(which, LC.SHAPE)
    d, m = BR.scene(origin)
    assert on_all_six_faces(d)
    if which != "LOW":
        assert not bits_equal(d, BR.scene(LC.limit_origin("LOW", LC.SHAPE))[0])      # the terrain is one of the world coordinate
    for flags in (0, BR.FILLED_ONLY):
        for lo, hi in BR.scene_regions(origin) + BR.scene_aligned(origin)[1:]:
            want = BR.encode(d, m, origin, lo, hi, flags)
            assert BR.same_stream(B.encode_host(d, m, origin, lo, hi, flags), want), (lo, hi, flags)
            assert len(want[1]) > 0
    # a stream taken at one end of the box decoded at the other
    lo, hi = BR.scene_regions(origin)[1]
    s = BR.encode(d, m, origin, lo, hi, 0)
    dst = tuple(origin[a] + LC.SHAPE[a] - (hi[a] - lo[a]) for a in range(3))
    want = BR.decode(d, m, origin, s, dst)
    got_d, got_m = np.array(d), np.array(m)
    B.decode_host(got_d, got_m, origin, *s, dst_lo=dst)
    assert bits_equal(got_d, want[0]) and got_m.tobytes() == want[1].tobytes()


@LONG
def test_bricks_long_row_equals_the_reference(box):
    d, m = LC.bricks_fill(box)
    regions = LC.bricks_regions(box)
    assert regions[1][0][box.axis] == box.origin[box.axis] + 1
    for flags in (0, BR.FILLED_ONLY):
        for lo, hi in regions:
            want = BR.encode(d, m, box.origin, lo, hi, flags)
            assert BR.same_stream(B.encode_host(d, m, box.origin, lo, hi, flags), want), (lo, hi, flags)
            nb = [(int(e) + 3) // 4 for e in want[0]["ext"][0]]
            b = want[1]["brick"].astype(np.int64)
            across = b // nb[0] if box.axis == 0 else (b % nb[0] + nb[0] * (b // (nb[0] * nb[1])) if box.axis == 1 else b % (nb[0] * nb[1]))
            assert np.bincount(across).max() >= 4096 and len(want[2]) > 0 and len(want[3]) > 0      # one brick row holds that many records
            assert set(np.unique(want[1]["kind"]).tolist()) >= {0, 3}
    s = BR.encode(d, m, box.origin, *regions[2], 0)
    want = BR.decode(np.zeros_like(d), np.zeros_like(m), box.origin, s, regions[1][0], 0)
    got_d, got_m = np.zeros_like(d), np.zeros_like(m)
    B.decode_host(got_d, got_m, box.origin, *s, dst_lo=regions[1][0])
    assert bits_equal(got_d, want[0]) and got_m.tobytes() == want[1].tobytes()


# ---- distance ------------------------------------------------------------------------------------------------------------------------------
@LIMIT
def test_distance_limit_scene_equals_the_reference(which):
    origin = LC.limit_origin(which, LC.DISTANCE_SHAPE)
    d, m = LC.distance_scene()
    assert on_all_six_faces(d) and not on_all_six_faces(DR.scene()[0])
    cases = DR.scene_cases(origin)
    assert len(cases) == len(DR.scene_cases())
    for lo, hi, radius, flags in cases:
        want = DR.field(d, origin, lo, hi, radius, flags)
        got = D.distance_field_host(d, origin, lo, hi, radius, flags)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (lo, hi, radius, flags)
    # the edits, whole box: the host's equal the model's
    for op, flags, d2 in ((DR.GROW, 0, 9), (DR.SHRINK, DR.TO_EMPTY, 4), (DR.HOLLOW, DR.TO_EMPTY, 2)):
        field = DR.field(d, origin, None, None, 3, flags)
        a, b = (d.copy(), m.copy()), (d.copy(), m.copy())
        n = DR.edit(*a, *field, op, d2, 0.75, 6, origin=origin)
        assert D.distance_edit_host(*b, origin, *field, op, d2, 0.75, 6) == n > 0
        assert bits_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


@LONG
def test_distance_long_fields_equal_the_closed_form(box):
    sources = LC.distance_sources(box)
    d, m = DR.volume_with(box.shape, sources)
    want = DR.from_sources(box.shape, sources, 255)
    got, info = D.distance_field_host(d, box.origin, None, None, 255, 0)
    assert got.tobytes() == want.tobytes() and info.tobytes() == DR.make_info(box.origin, (0, 0, 0), box.shape, 255, 0, want).tobytes()
    assert (want == 65025).any() and (want == DR.FAR).any() and int((want == 0).sum()) == len(sources)
    along = sorted(s[box.axis] for s in sources)
    assert along[0] == 0 and along[-1] == box.length - 1 and box.length // 2 in along and 64 in np.diff(along)
    # the closed form against the separable model where that is fast, and a region that starts off the brick grid
    short = box.shortened()
    src = LC.distance_sources(short)
    ds, _ = DR.volume_with(short.shape, src)
    assert DR.from_sources(short.shape, src, 12).tobytes() == DR.field(ds, short.origin, None, None, 12, 0)[0].tobytes()
    assert DR.field(ds, short.origin, None, None, 12, 0, pad=0)[0].tobytes() == DR.field(ds, short.origin, None, None, 12, 0)[0].tobytes()
    lone = [short.cell(20, 1, 2)]                                 # a lone source: cells at exactly R and beyond it along the axis, up to R = 255
    for sources_pinned in (src, lone):
        dp, _ = DR.volume_with(short.shape, sources_pinned)
        for radius in (255, 64, 3):                               # the radii of the long cases, up to the cap: without the padding the model is fast
            capped = DR.field(dp, short.origin, None, None, radius, 0, pad=0)
            assert DR.from_sources(short.shape, sources_pinned, radius).tobytes() == capped[0].tobytes()
            assert D.distance_field_host(dp, short.origin, None, None, radius, 0)[0].tobytes() == capped[0].tobytes()
            if sources_pinned is lone:
                assert (capped[0] == radius * radius).any() and (capped[0] == DR.FAR).any()
    lo, hi = LC.bricks_regions(box)[2]
    l = tuple(lo[a] - box.origin[a] for a in range(3))
    cut = np.ascontiguousarray(want[l[2]:hi[2] - box.origin[2], l[1]:hi[1] - box.origin[1], l[0]:hi[0] - box.origin[0]])
    got, info = D.distance_field_host(d, box.origin, lo, hi, 255, 0)
    assert got.tobytes() == cut.tobytes() and info.tobytes() == DR.make_info(box.origin, l, cut.shape[::-1], 255, 0, cut).tobytes()


@LONG
def test_distance_long_rod_to_empty_and_its_edits_equal_the_reference(box):
    d, m = LC.rod_fill(box)
    for flags in (DR.TO_EMPTY, DR.TO_EMPTY | DR.BOX_IS_SOLID):
        want = DR.field(d, box.origin, None, None, 2, flags)
        got = D.distance_field_host(d, box.origin, None, None, 2, flags)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    field = DR.field(d, box.origin, None, None, 2, DR.TO_EMPTY)
    assert int(field[0].max()) == 4 and (field[0] == 1).sum() > 8 * (box.length - 16)      # the rod has an inside, two cells from empty space
    for op, d2 in ((DR.SHRINK, 1), (DR.HOLLOW, 1)):
        a, b = (d.copy(), m.copy()), (d.copy(), m.copy())
        n = DR.edit(*a, *field, op, d2, origin=box.origin)
        assert D.distance_edit_host(*b, box.origin, *field, op, d2) == n >= box.length - 16
        assert bits_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


# ---- quads ---------------------------------------------------------------------------------------------------------------------------------
def quads_prior():
    d0, m0 = prior(LC.SHAPE[::-1])
    d0[::3, ::2, ::5] = -0.5
    d0[1::7, ::3, ::2] = np.nan
    return d0, m0


def same_quads(a, b):
    return np.ascontiguousarray(a, dtype=QR.DTYPE).tobytes() == np.ascontiguousarray(b, dtype=QR.DTYPE).tobytes()


@LIMIT
def test_quads_limit_scene_equals_the_reference(which):
    origin = LC.limit_origin(which, LC.SHAPE)
    d, m = quads_prior()
    assert on_all_six_faces(d)
    regions = BR.scene_regions(origin)                            # the ragged regions of tests/test_quads_gpu.py
    for (lo, hi), ignore in ((regions[0], False), (regions[1], True), (regions[3], False), (regions[4], True)):
        want, n_faces = QR.extract(d, m, origin, lo, hi, ignore)
        got = M.extract_quads_host(d, m, origin, lo, hi, ignore)
        assert same_quads(got, want) and M.extract_quads_host.totals == (len(want), n_faces), (lo, hi, ignore)
        if lo is None:
            hi_box = LC.box_hi(origin, LC.SHAPE)
            for a in range(3):                                    # quads on both outer faces of the box: world int32 coordinates at the lattice's ends
                on_axis = want[np.isin(want["face"], (2 * a, 2 * a + 1))]
                assert int(on_axis["lo"][:, a].min()) == origin[a] and int(on_axis["lo"][:, a].max()) == hi_box[a]


@LONG
def test_quads_long_slab_and_seams_equal_the_reference(box):
    n, a = box.length, box.axis
    d, m = LC.quads_fill(box, "slab")
    want, n_faces = QR.extract(d, m, box.origin)
    assert same_quads(M.extract_quads_host(d, m, box.origin), want) and M.extract_quads_host.totals == (6, n_faces)
    assert sorted(max(int(q["du"]), int(q["dv"])) for q in want)[2:] == [n] * 4 and n_faces == 2 * n * box.nu + 2 * n + 2 * box.nu
    d, m = LC.quads_fill(box, "seams")
    want, n_faces = QR.extract(d, m, box.origin)
    assert same_quads(M.extract_quads_host(d, m, box.origin), want)
    runs = LC.seam_runs(box)
    assert {r[0] for r in runs} >= {63, 64, 65, n - 64, n - 1} and {r[1] for r in runs} >= {62, 63, 64, n - 2, n - 1}
    u, v = QR.PLANE_AXES[box.u_axis]                              # a side face of the row: the runs are its quads
    side = want[want["face"] == 2 * box.u_axis]
    length = side["du"] if u == a else side["dv"]
    first = side["lo"][:, a] - box.origin[a]
    assert sorted(zip(first.tolist(), (first + length - 1).tolist(), side["material"].tolist())) == sorted(runs)


# ---- terrain -------------------------------------------------------------------------------------------------------------------------------
def terrain_pinned(p, kw, lo, hi, before=(None, None)):
    """The host evaluation of the region equals the numpy reference's; returns the reference's arrays."""
    got_d, got_m, n = T.eval_box(p, lo, hi, *before)
    ref_d, ref_m = TR.eval_box(kw, lo, hi, *before)
    assert bits_equal(got_d, ref_d) and got_m.tobytes() == ref_m.tobytes() and n > 0
    return ref_d, ref_m


@LIMIT
def test_terrain_limit_boxes_equal_the_reference(which):
    """Every parameter set and region that tests/test_volume_limits_gpu.py runs in the limit boxes."""
    origin = LC.limit_origin(which, LC.SHAPE)
    hi = LC.box_hi(origin, LC.SHAPE)
    d0, m0 = prior(LC.SHAPE[::-1])
    lo_r, hi_r = BR.scene_regions(origin)[1]
    sl = tuple(slice(lo_r[a] - origin[a], hi_r[a] - origin[a]) for a in (2, 1, 0))
    whole = {}
    for tag, p, kw in LC.limit_terrain_cases(origin):
        assert kw["cave_octaves"] > 0
        whole[tag], _ = terrain_pinned(p, kw, origin, hi, (d0, m0) if kw["flags"] & 4 else (None, None))
        terrain_pinned(p, kw, lo_r, hi_r, (d0[sl], m0[sl]))      # the ragged region, over prior content
    # what makes them hard, from the reference's arrays: the solid terrains stand on five faces, the tall one is cut off by the sixth (it
    # writes voxels at y = 32767 in HIGH and MIXED); a shell is open at the top
    assert on_all_six_faces(whole["tall"]) and LC.faces_filled(whole["flags 0"]) == [True, True, False, True, True, True]
    assert all(LC.faces_filled(whole["flags 3"])[k] for k in (0, 1, 3, 4, 5)) and 0.05 < (whole["flags 3"] > 0).mean() < 0.5
    other = LC.limit_origin("HIGH" if which != "HIGH" else "LOW", LC.SHAPE)
    _, p2, kw2 = LC.limit_terrain_cases(other)[1]
    assert not bits_equal(TR.eval_box(kw2, other, LC.box_hi(other, LC.SHAPE))[0], whole["flags 3"])      # a function of the world coordinate, not of the box


@LONG
def test_terrain_long_boxes_equal_the_reference(box):
    """Every parameter set and region that tests/test_volume_limits_gpu.py runs in the long boxes."""
    d0, m0 = LC.sparse_fill(box)
    for flags in LC.LONG_TERRAIN_FLAGS:
        p, kw = LC.long_terrain_params(box, flags)
        ref_d, _ = terrain_pinned(p, kw, box.origin, box.hi, (d0, m0) if flags & 4 else (None, None))
        filled = ref_d > 0
        assert 0.02 < filled.mean() < 0.9 and filled[0].any() and filled[-1].any() and filled[:, :, 0].any() and filled[:, :, -1].any()
    lo, hi = LC.bricks_regions(box)[2]                            # off the brick grid on the long axis, with the last parameter set, over content
    sl = tuple(slice(lo[a] - box.origin[a], hi[a] - box.origin[a]) for a in (2, 1, 0))
    terrain_pinned(p, kw, lo, hi, (np.ascontiguousarray(d0[sl]), np.ascontiguousarray(m0[sl])))


# ---- voxelize ------------------------------------------------------------------------------------------------------------------------------
@LIMIT
def test_voxelize_limit_mesh_equals_the_reference(shim, which):
    origin = LC.limit_origin(which, LC.SHAPE)
    (pos, tri), lo_m, hi_m = LC.limit_mesh(which)
    planes = set(pos.reshape(-1).tolist())
    assert (float(LO) in planes) == (which != "HIGH") and (float(HI) in planes) == (which != "LOW")
    for solid in (False, True):
        rc, d, m, n = shim_voxelize(shim, pos, tri, origin, LC.SHAPE, material=3, density=1.5, solid=solid)
        filled, ids = VR.voxelize(pos, tri, origin, LC.SHAPE, material=3, solid=solid)
        assert rc == 0 and np.array_equal(d > 0, filled) and np.array_equal(m, ids) and n == int(filled.sum()) > 2000
        assert sum(LC.faces_filled(d)) >= 3
        d0, m0 = stamp_prior()                                    # over prior content, as the GPU test runs it
        rc, d, m, n = shim_voxelize(shim, pos, tri, origin, LC.SHAPE, material=3, density=1.5, solid=solid, dens=d0, ids=m0)
        want_d, want_m = LC.voxelized_over(d0, m0, filled, ids, 1.5)
        assert rc == 0 and bits_equal(d, want_d) and np.array_equal(m, want_m) and n == int(filled.sum())


@LONG
def test_voxelize_long_prism_equals_the_closed_form(shim, box):
    pos, tri, _ = LC.prism(box)
    q = VR.snap(pos)[tri.astype(np.int64)]
    span = (q.max(axis=1) // 256 - q.min(axis=1) // 256 + 1).max()
    assert LC.SEGMENT <= span <= 2048 and len(tri) == 8 * 9 + 4      # nine segments, each triangle within the 2048-voxel limit
    for solid in (False, True):
        want = LC.prism_expected(box, solid)
        rc, d, m, n = shim_voxelize(shim, pos, tri, box.origin, box.shape, material=3, density=1.5, solid=solid)
        assert rc == 0 and n == int(want.sum())
        assert np.array_equal(d, np.where(want, np.float32(1.5), np.float32(0))) and np.array_equal(m, np.where(want, 3, 0))
        short = box.shortened()
        ps, ts, _ = LC.prism(short)
        filled, ids = VR.voxelize(ps, ts, short.origin, short.shape, material=3, solid=solid)
        assert np.array_equal(filled, LC.prism_expected(short, solid)) and np.array_equal(ids, np.where(filled, 3, 0))
    assert int(LC.prism_expected(box, True).sum()) > int(LC.prism_expected(box, False).sum()) > 16000
    d0, m0 = LC.sparse_fill(box)                                  # solid, over content, as the GPU test runs it
    want = LC.prism_expected(box, True)
    rc, d, m, n = shim_voxelize(shim, pos, tri, box.origin, box.shape, material=3, density=1.5, solid=True, dens=d0, ids=m0)
    want_d, want_m = LC.voxelized_over(d0, m0, want, np.where(want, 3, 0), 1.5)
    assert rc == 0 and bits_equal(d, want_d) and np.array_equal(m, want_m) and n == int(want.sum())


# ---- stamp and capture -----------------------------------------------------------------------------------------------------------------------
def stamp_prior():
    d0, m0 = prior(LC.SHAPE[::-1])
    d0[::3, ::2, ::5] = -0.5
    d0[1::7, ::3, ::2] = np.nan
    return np.ascontiguousarray(d0), np.ascontiguousarray(m0)


def stamped_both_ways(d0, m0, origin, xyz, mm, place, mode, value=1.5):
    a, b = (d0.copy(), m0.copy()), (d0.copy(), m0.copy())
    want = SR.stamp(*a, origin, xyz, mm, place, mode, value)
    got = ST.stamp_voxels_host(*b, origin, xyz, mm, ST.placement(*place), mode, value)
    assert got == want and bits_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), (place, mode)
    return want


@LIMIT
def test_stamp_limit_placements_equal_the_reference(which):
    origin = LC.limit_origin(which, LC.SHAPE)
    hi = LC.box_hi(origin, LC.SHAPE)
    d0, m0 = stamp_prior()
    xyz, mm = SR.small_model()
    n = len(np.unique(xyz, axis=0))
    assert on_all_six_faces(d0)
    for end in (1, -1):
        flush, beyond = LC.stamp_flush(xyz, end), LC.stamp_beyond(xyz, end)
        assert len({(p[1], p[2]) for p in flush}) == 48
        for k, place in enumerate(flush):
            lo_w, hi_w = LC.world_box(xyz, place)
            assert hi_w == (HI, HI, HI) if end > 0 else lo_w == (LO, LO, LO)
            inside = all(origin[a] <= lo_w[a] and hi_w[a] <= hi[a] for a in range(3))
            assert inside == (which == ("HIGH" if end > 0 else "LOW"))
            written = stamped_both_ways(d0, m0, origin, xyz, mm, place, (SR.SET, SR.KEEP, SR.ERASE)[k % 3])
            assert (written == n or k % 3 == 1) if inside else written < n
            lo_b, hi_b = LC.world_box(xyz, beyond[k])             # one voxel further: it leaves the lattice by exactly one voxel on one axis
            assert sorted(max(h - HI, 0) + max(LO - l, 0) for l, h in zip(lo_b, hi_b)) == [0, 0, 1]
    for k, place in enumerate(LC.stamp_clipped(origin, LC.SHAPE)):
        assert 0 < SR.clipped(xyz, origin, LC.SHAPE[::-1], place) < n
        assert stamped_both_ways(d0, m0, origin, xyz, mm, place, (SR.SET, SR.KEEP, SR.ERASE)[k % 3]) > 0
    for k, place in enumerate(LC.stamp_flush_in(xyz, origin, LC.SHAPE)):
        lo_w, hi_w = LC.world_box(xyz, place)
        assert all(origin[a] <= lo_w[a] and hi_w[a] <= hi[a] and (lo_w[a] == LO) == (origin[a] == LO) and (hi_w[a] == HI) == (hi[a] == HI) for a in range(3))
        assert SR.clipped(xyz, origin, LC.SHAPE[::-1], place) == 0
        stamped_both_ways(d0, m0, origin, xyz, mm, place, (SR.SET, SR.KEEP, SR.ERASE)[k % 3])
    # capture: the whole box, and a region in the corner at the lattice's end
    for lo, hi_r in ((None, None), (tuple(h - 21 for h in hi), hi), (origin, tuple(o + 19 for o in origin))):
        want = SR.capture(d0, m0, origin, lo, hi_r)
        got = ST.capture_voxels_host(d0, m0, origin, lo, hi_r)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and len(want[1]) > 100


@LONG
def test_stamp_and_capture_long_boxes_equal_the_reference(box):
    d0, m0 = LC.sparse_fill(box)
    xyz, mm = LC.rod_model()
    places = LC.long_stamp_places(box)
    boxes = [LC.world_box(xyz, p) for p in places]
    a = box.axis
    assert any(lo[a] == box.origin[a] for lo, _ in boxes) and any(hi[a] == box.hi[a] for _, hi in boxes)                  # flush against both ends
    assert any(lo[a] < box.origin[a] or hi[a] > box.hi[a] for lo, hi in boxes) and all(LO <= lo[a] and hi[a] <= HI for lo, hi in boxes)
    for k, place in enumerate(places):
        assert stamped_both_ways(d0, m0, box.origin, xyz, mm, place, (SR.SET, SR.KEEP, SR.ERASE)[k % 3]) > 0
    want = SR.capture(d0, m0, box.origin)
    got = ST.capture_voxels_host(d0, m0, box.origin)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert int(want[0][:, a].min()) == 0 and int(want[0][:, a].max()) == box.length - 1 and SWR.model_levels(want[0]) == 7
