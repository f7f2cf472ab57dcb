"""GPU: the shadow rays' last-occluder map behind every kind of volume edit, as NUMBERS.  The map is an upper bound per texel that is kept
across rebuilds and raised only where an edit says it may have filled something (api.hip: update_sun_map), so it stays valid only while
every writer tells gpu_volume_commit a box that covers what it wrote and Edit::MayFill whenever an empty cell may have become filled.  A
writer that under-reports either keeps every array, tree and first hit right: only the map shows it.

Per case of tests/sun_map_cases.py (tests/test_sun_map_writers_cpu.py proves that each can fail) and brick layout: the base content is
uploaded and rebuilt, its map is tight; the edit is applied, what the entry returns and the whole download equal the family's numpy
reference; one rebuild; then, by the case's class,
    fills            the map is valid (Verdict.assert_valid: bounds_reference.sun_delta, 8 ulp of the largest plane value, nothing wider),
                     no tightening is owed, one loose edit was counted, the texels out of the box's reach hold the bits they held; where
                     the committed box is the whole volume or the lattice moved, the map was searched anew and is tight;
    clears           the map is valid and every texel holds the bits it held; one loose edit was counted;
    writes_nothing   the texels and the info record hold the bits they held (a brush that changes nothing still commits its box: one
                     loose edit, as test_the_tightening_cycle of tests/test_sun_map_gpu.py counts its empty brushes).
"Out of the box's reach" is taken for the box the case declares, as it stands: gpu_volume_commit notes the box each writer hands it, and
every writer hands over what it may have written.  Only apply_shapes commits more (shapes_kernels.hip aligns each shape's box outwards to
the 4-cell bricks before it joins them): for that family alone the declared box is aligned the same way.  Once per family, path-traced planes with the map on and off are bit-identical and the
colour differs from the one before the edit.  And one tightening cycle behind 32 rebuilds of mixed writers.

Measured on an MI355X over all cases and both layouts (every test prints its own through Verdict.report): no texel stood more than
2.5e-5 voxel (0.10 delta) below its lower bound; the tight maps — fresh, searched anew, drained — deviate by at most 3.8e-5 voxel (0.16
delta, the 256-cube of the cycle; 6.4e-6 = 0.10 delta in the 64-cube); loose texels behind one filling edit stand up to 85 voxels above
hi, behind the cycle's 32nd rebuild up to 180, as the raise intends."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import world as W
from tests import bounds_reference as B
from tests import sun_map_cases as SC
from tests.conftest import SEED
from tests.test_sun_map_gpu import BAND_TEXELS, BIG, CUBE, LAYOUTS, LOOSE_EDITS, ORIGIN, TOP, Verdict, sparse_content, tracer, unchanged_outside

pytestmark = pytest.mark.gpu

COMMITS_WITHOUT_WRITING = ("brush",)      # families whose entry commits its box whatever it changed


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def voxels_of(w):
    return B.voxels_of(w.filled(), w.origin)


def brick_box(box, origin, shape):
    """The box aligned outwards to the 4-cell bricks of the volume at `origin`, cut with it."""
    lo = tuple(origin[a] + (box[0][a] - origin[a]) // 4 * 4 for a in range(3))
    hi = tuple(min(origin[a] + -(-(box[1][a] - origin[a]) // 4) * 4, origin[a] + shape[a]) for a in range(3))
    return lo, hi


def apply(case, t, ids, w, download=True):
    """The case on the model `w` and on the device: the entries return what the references return, the arrays are the model's."""
    want = case.on_model(w)
    got = case.on_device(t, ids, want)
    assert SC.norm(got) == SC.norm(want), f"{case}: the entry returned {got}, the reference {want}"
    if download:
        gd, gm = t.volume_download()
        assert gd.tobytes() == w.d.tobytes() and gm.tobytes() == w.m.tobytes(), (case, "the arrays differ from the reference's")
        assert tuple(t.volume_scroll((0, 0, 0))["origin"][0].tolist()) == w.origin, case


def start(case, keyed, mats):
    """A tracer with the case's base content installed, its models, the model's world and the verdict on the fresh map."""
    t = tracer(keyed)
    t.volume_create(ORIGIN, CUBE, 128, 1.0)
    w = case.world()
    t.volume_upload(w.d, w.m)
    ids = SC.create_models(t)
    st = t.volume_rebuild(mats)
    assert int(st.levels) == 3 and tuple(int(c) for c in st.origin) == ORIGIN
    before = Verdict(t, voxels_of(w))
    before.assert_tight(f"{case.name}: base")
    assert int(before.info["loose_edits"]) == 0 and int(before.info["tighten_pending"]) == 0
    return t, ids, w, before


def same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


@LAYOUTS
@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_the_map_behind_a_writer(case, keyed, mats):
    t, ids, w, before = start(case, keyed, mats)
    try:
        info_before = t.sun_map(want_map=False)[0].copy()
        apply(case, t, ids, w)
        t.volume_rebuild(mats)
        after = Verdict(t, voxels_of(w))
        after.report(f"{case.name}, {'keyed' if keyed else 'general'}")
        loose = int(after.info["loose_edits"])
        if case.cls == SC.FILLS:
            after.assert_valid(case.name)
            assert int(after.info["tighten_pending"]) == 0
            if case.box is None:                                      # the whole volume, or another lattice: a new world to the map
                assert loose == 0
                after.assert_tight(f"{case.name}: searched anew")
                if not case.lattice_moves:
                    assert (after.lo > before.lo + 1.0).any()
            else:
                assert loose == 1
                box = brick_box(case.box, ORIGIN, CUBE) if case.family == "apply_shapes" else case.box
                unchanged_outside(before, after, box, case.name)
                assert (after.lo > before.lo + 1.0).any(), "the edit must add something taller than what stood there"
                assert (after.texels != before.texels).any()
        elif case.cls == SC.CLEARS:
            after.assert_valid(case.name)
            assert same_bits(after.texels, before.texels), (case, "a clearing edit changed the map")
            assert loose == 1 and int(after.info["tighten_pending"]) == 0
        else:
            assert same_bits(after.texels, before.texels), (case, "an edit that wrote nothing changed the map")
            info_before["loose_edits"] += 1 if case.family in COMMITS_WITHOUT_WRITING else 0
            assert t.sun_map(want_map=False)[0].tobytes() == info_before.tobytes(), (case, "the info record changed")
    finally:
        t.shutdown()


# ---- path-traced planes, once per family ---------------------------------------------------------------------------------------------------
def cameras():
    c = [ORIGIN[a] + CUBE[a] / 2 for a in range(3)]
    return [W.camera_look_at((c[0] + 70.0, c[1] + 60.0, c[2] + 80.0), tuple(c), 60.0, 64, 64),
            W.camera_look_at((c[0] - 75.0, c[1] + 50.0, c[2] - 70.0), tuple(c), 60.0, 64, 64)]


def same_planes(t, tag):
    """test_edit_commit_gpu.Scene.same at 64 x 64: every plane bit-identical with the map off and on; returns the colour planes."""
    planes = []
    for cam in cameras():
        t.set_sun_map(False)
        plain = t.trace_paths(cam, spp=2, max_bounces=2, frame_index=4)
        t.set_sun_map(True)
        got = t.trace_paths(cam, spp=2, max_bounces=2, frame_index=4)
        for k in plain:
            assert got[k].tobytes() == plain[k].tobytes(), (tag, k)
        planes.append(plain["color"].tobytes())
    return planes


def first_of(family):
    own = [c for c in SC.CASES if c.family == family]
    return next((c for c in own if c.cls == SC.FILLS), own[0])


@LAYOUTS
@pytest.mark.parametrize("family", SC.FAMILIES)
def test_path_traced_planes_do_not_see_the_map(family, keyed, mats):
    case = first_of(family)
    t, ids, w, _ = start(case, keyed, mats)
    try:
        first = same_planes(t, f"{case.name}: base")
        apply(case, t, ids, w)
        t.volume_rebuild(mats)
        assert same_planes(t, case.name) != first, (case, "the edit is not seen")
    finally:
        t.shutdown()


# ---- the tightening cycle behind mixed writers -----------------------------------------------------------------------------------------------
FAR_SHIFT = (184, 84, 184)                # the same cases at the far end of the BIG box: the union of the edits' boxes spans the map
CYCLE_FILLS = ("shapes SET column", "affine SET lattice rotation", "stamp KEEP", "terrain ADD", "voxelize a prism against two faces",
               "flood FILL_UNREACHED a sealed shaft", "brush ADD 1", "shapes ADD capsule")
CYCLE_CLEARS = ("shapes that cannot fill", "affine ERASE", "stamp ERASE", "flood PAINT and CLEAR", "distance SHRINK", "brush SUBTRACT 0", "distance HOLLOW")


def cycle_schedule():
    """32 cases, a filling and a clearing one in turn, each family's turn at either end of the box; the 32nd clears, so that no raise
    follows the first band."""
    near, far = {c.name: c for c in SC.table()}, {c.name: c for c in SC.table(FAR_SHIFT)}
    out = []
    for k in range(1, LOOSE_EDITS + 1):
        pair = (k - 1) // 2
        name = CYCLE_FILLS[pair % len(CYCLE_FILLS)] if k % 2 else CYCLE_CLEARS[pair % len(CYCLE_CLEARS)]
        out.append((far if (pair + pair // 8) % 2 else near)[name])
    assert len({c.family for c in out}) >= 8 and out[-1].cls == SC.CLEARS
    return out


@LAYOUTS
def test_the_tightening_cycle_behind_mixed_writers(keyed, mats):
    d, m = sparse_content(BIG, 30, fill=0.0002, top=TOP)
    w = SC.World(d, m, ORIGIN)
    schedule = cycle_schedule()
    for case in schedule:                                                 # what the clearing cases clear, at either end
        for lo, hi in case.base:
            w.d[w.slices(lo, hi)], w.m[w.slices(lo, hi)] = 1.0, 3
    t = tracer(keyed)
    try:
        t.volume_create(ORIGIN, BIG, 128, 1.0)
        t.volume_upload(w.d, w.m)
        ids = SC.create_models(t)
        assert int(t.volume_rebuild(mats).levels) == 4
        fresh = Verdict(t, voxels_of(w))
        fresh.assert_tight("fresh 256-cube map")
        nv, nu = fresh.map.shape
        boxes = []
        for k, case in enumerate(schedule, start=1):
            apply(case, t, ids, w, download=False)
            boxes.append(case.box)
            t.volume_rebuild(mats)
            v = Verdict(t, voxels_of(w))
            v.assert_valid(f"rebuild {k} behind {case.name}")
            assert int(v.info["loose_edits"]) == k % LOOSE_EDITS, (k, case)
            assert int(v.info["tighten_pending"]) == (1 if k == LOOSE_EDITS else 0), (k, case)
        v.report("after the 32nd rebuild")
        gd, gm = t.volume_download()
        assert gd.tobytes() == w.d.tobytes() and gm.tobytes() == w.m.tobytes(), "the arrays differ from the reference's"
        # the rectangle, less the first band (searched by the 32nd call itself), contains the texels of every edit's box
        u0, u1, v0, v1 = (int(v.info[key]) for key in ("pending_u0", "pending_u1", "pending_v0", "pending_v1"))
        rows = max(1, BAND_TEXELS // (u1 - u0 + 1))
        for box in boxes:
            iv, iu = np.nonzero(v.reached(*box))
            assert u0 <= iu.min() and iu.max() <= u1 and v0 - rows <= iv.min() and iv.max() <= v1, (box, (u0, u1, v0, v1))
        rect = np.zeros((nv, nu), bool)
        rect[v0 - rows:v1 + 1, u0:u1 + 1] = True
        assert (u1 - u0 + 1) * (v1 - v0 + 1) > 2 * BAND_TEXELS, "the rectangle must need several bands"
        # clearing brushes at an empty place: a band of rows per rebuild
        empty_at = (ORIGIN[0] + 100.5, ORIGIN[1] + 140.5, ORIGIN[2] + 90.5)
        n_bands = 1
        while int(v.info["tighten_pending"]):
            assert n_bands < 40
            t.volume_apply_brush(empty_at, 1.2, 0.0, 1)
            t.volume_rebuild(mats)
            band = Verdict(t, voxels_of(w))
            band.assert_valid(f"band {n_bands}")
            if v1 - v0 + 1 <= rows:
                assert int(band.info["tighten_pending"]) == 0
            else:
                v0 += rows
                assert int(band.info["tighten_pending"]) == 1
                assert tuple(int(band.info[key]) for key in ("pending_u0", "pending_u1", "pending_v0", "pending_v1")) == (u0, u1, v0, v1)
            assert int(band.info["loose_edits"]) == n_bands
            n_bands += 1
            v = band
        assert n_bands >= 3
        v.assert_tight("drained behind mixed writers")
        assert (v.texels[~rect].view(np.uint32) == fresh.texels[~rect].view(np.uint32)).all(), "texels outside the rectangle were never touched"
        gd, gm = t.volume_download()
        assert gd.tobytes() == w.d.tobytes() and gm.tobytes() == w.m.tobytes()
    finally:
        t.shutdown()
