"""GPU: blok_hip_volume_stamp_models and blok_hip_volume_capture_model against the numpy model of their contract
(tests/stamp_reference.py): the volume's arrays byte for byte after every call, the rebuilt tree against volume_tree_reference, a baked
instance against the traced one, captured models against blok_hip_model_create's byte for byte.  Both brick layouts unless said.

Not covered: BLOK_ERR_UNSUPPORTED for a volume above 2^32 cells (its two arrays alone are 32 GiB).
Boxes at the ends of the int16 lattice and boxes of 16384 cells on one axis are covered in tests/test_volume_limits_gpu.py."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import stamp as ST
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import stamp_reference as R
from tests.conftest import SEED, records_equal
from tests.terrain_cases import prior
from tests.volume_tree_reference import DenseModel, box_levels, reference_tree

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
MODES = (R.SET, R.KEEP, R.ERASE)
ORIGIN, SHAPE = (-40, -44, -24), (96, 80, 64)


def _tracer(w=64, h=64):
    from blok_amd.tracer import HipTracer
    return HipTracer(w, h).init()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def prior_with_empties(shape_xyz=SHAPE):
    """terrain_cases.prior plus negative and NaN densities, as test_quads_gpu.py builds it."""
    d0, m0 = prior(tuple(shape_xyz)[::-1])
    d0[::3, ::2, ::5] = -0.5
    d0[1::7, ::3, ::2] = np.nan
    return np.ascontiguousarray(d0), np.ascontiguousarray(m0)


def places(table, model_ids):
    """INSTANCE records of [(model index, (offset, axis, flip))]."""
    return np.concatenate([ST.placement(p[0], p[1], p[2], model_ids[i]) for i, p in table])


def arrays_equal(t, d, m, tag):
    gd, gm = t.volume_download()
    assert gd.tobytes() == d.tobytes(), (tag, "density", int((gd.view(np.uint32) != d.view(np.uint32)).sum()))
    assert gm.tobytes() == m.tobytes(), (tag, "ids", int((gm != m).sum()))


def tree_equal(t, d, m, origin, mats, tag):
    """After a rebuild the tree is reference_tree of the reference arrays, byte for byte."""
    st = t.volume_rebuild(mats)
    levels = box_levels(d.shape[::-1])
    ref_nodes, ref_mats = reference_tree(d > 0, m, levels)
    assert (st.n_voxels, st.n_tree_nodes, st.levels, tuple(st.origin)) == (len(ref_mats), len(ref_nodes), levels, tuple(origin)), tag
    nodes, ids = t.download_tree()
    assert nodes.tobytes() == ref_nodes.tobytes(), (tag, "nodes")
    assert ids.tobytes() == ref_mats.tobytes(), (tag, "materials")


class Both:
    """The same stamps to the volume and to the reference arrays."""

    def __init__(self, t, keyed, origin, shape, d0, m0, models):
        self.t, self.origin, self.models = t, origin, models
        t.set_volume_layout(keyed)
        t.volume_create(origin, shape)
        t.volume_upload(d0, m0)
        self.d, self.m = d0.copy(), m0.copy()
        self.ids = [t.model_create(xyz, mm) for xyz, mm in models]

    def stamp(self, table, mode, value=1.5, tag=None):
        """table: [(model index, (offset, axis, flip))], one call."""
        want = 0
        for i, place in table:
            want += R.stamp(self.d, self.m, self.origin, *self.models[i], place, mode, value)
        got = self.t.volume_stamp_models(places(table, self.ids), mode, value)
        assert got == want, (tag, got, want)
        arrays_equal(self.t, self.d, self.m, tag)
        return want


# ---- arrays -------------------------------------------------------------------------------------------------------------------------

@LAYOUTS
def test_every_orientation_and_mode_gives_the_reference_arrays(keyed):
    t = _tracer()
    b = Both(t, keyed, ORIGIN, SHAPE, *prior_with_empties(), [R.small_model(), R.large_model()])
    rng = np.random.default_rng(17)
    written = {mode: 0 for mode in MODES}
    for mode in MODES:
        for axis, flip in R.ORIENTATIONS:
            offset = tuple(int(v) for v in rng.integers((-34, -38, -18), (50, 30, 34)))      # always inside: the model reaches 4 from its offset
            written[mode] += b.stamp([(0, (offset, axis, flip))], mode, 0.5 + flip, ("small", mode, axis, flip))
    for mode in MODES:
        for axis, flip in R.LARGE_ORIENTATIONS:                # 70 voxels long: clipped whenever its long axis runs along z (64)
            offset = tuple(int(v) for v in rng.integers((0, -10, 0), (16, 6, 16)))
            written[mode] += b.stamp([(1, (offset, axis, flip))], mode, 2.0, ("large", mode, axis, flip))
    assert all(n > 1000 for n in written.values()), written
    t.shutdown()


# ---- clipping and order -------------------------------------------------------------------------------------------------------------

CLIP_ORIGIN, CLIP_SHAPE = (-9, -7, -5), (24, 20, 16)
# an offset ON a face of the box: the small model has voxels on both sides of zero along every local axis, so some of it lands on either side
CLIP_OFFSETS = {"-x": (-9, 3, 1), "+x": (15, 3, 1), "-y": (2, -7, 1), "+y": (2, 13, 1), "-z": (2, 3, -5), "+z": (2, 3, 11)}


@LAYOUTS
def test_clipping_at_each_face_wholly_outside_and_tables_in_order(keyed):
    t = _tracer()
    xyz, mm = R.small_model()
    twin = (xyz.copy(), mm + np.uint32(5000))
    d0, m0 = prior_with_empties(CLIP_SHAPE)
    b = Both(t, keyed, CLIP_ORIGIN, CLIP_SHAPE, d0, m0, [(xyz, mm), twin, R.large_model()])
    def fresh():                                               # every case starts from the prior content, as on the CPU
        t.volume_upload(d0, m0)
        b.d, b.m = d0.copy(), m0.copy()

    for mode in MODES:
        for face, offset in CLIP_OFFSETS.items():
            for axis, flip in (((0, 1, 2), 0), ((1, 2, 0), 5), ((2, 1, 0), 2)):
                place = (offset, axis, flip)
                assert 0 < R.clipped(xyz, CLIP_ORIGIN, CLIP_SHAPE[::-1], place) < len(xyz)
                fresh()
                assert b.stamp([(0, place)], mode, 1.5, (mode, face, axis, flip)) > 0      # (the count is the reference's: the case clips and writes)
        for offset in ((60, 3, 1), (2, -40, 1), (2, 3, 30000), (-30000, 3, 1)):      # wholly outside: nothing written, not an error
            assert b.stamp([(0, (offset, (0, 1, 2), 3))], mode, 1.5, (mode, offset)) == 0
    # the large model hangs out of this small box on every side
    for mode in MODES:
        fresh()
        assert b.stamp([(2, ((3, 2, 1), (1, 2, 0), 3))], mode, 0.75, ("large", mode)) > 0
    # two overlapping placements in one call: the later one wins where both write
    place_a, place_b = ((2, 3, 1), (0, 1, 2), 0), ((4, 2, 2), (1, 0, 2), 2)
    wa = {tuple(w): int(v) for w, v in zip(R.world_voxels(xyz, *place_a), mm)}
    wb = {tuple(w): int(v) for w, v in zip(R.world_voxels(xyz, *place_b), twin[1])}
    overlap = set(wa) & set(wb)
    assert overlap and any(wa[w] != wb[w] for w in overlap)
    for mode in (R.ERASE, R.KEEP, R.SET):
        b.stamp([(0, place_a), (1, place_b)], mode, 1.25, ("pair", mode))
    assert all(int(b.m[w[2] - CLIP_ORIGIN[2], w[1] - CLIP_ORIGIN[1], w[0] - CLIP_ORIGIN[0]]) == wb[w] for w in overlap)
    # five placements with chained overlaps, models alternating, in one call
    chain = [(k % 2, ((-4 + 3 * k, -2 + 2 * k, -2 + k), axis, flip))
             for k, (axis, flip) in enumerate((((0, 1, 2), 0), ((1, 0, 2), 1), ((2, 1, 0), 6), ((0, 2, 1), 3), ((1, 2, 0), 4)))]
    for (_, pa), (_, pb) in zip(chain, chain[1:]):
        assert {tuple(w) for w in R.world_voxels(xyz, *pa)} & {tuple(w) for w in R.world_voxels(xyz, *pb)}, "the chain is broken"
    for mode in (R.ERASE, R.KEEP, R.SET, R.ERASE):
        b.stamp(chain, mode, 3.0, ("chain", mode))
    assert t.volume_stamp_models(np.zeros(0, dtype=_ffi.INSTANCE)) == 0          # an empty table is fine
    arrays_equal(t, b.d, b.m, "empty table")
    t.shutdown()


# ---- masks and tree -----------------------------------------------------------------------------------------------------------------

def _bricks(d, m):
    """(mask per brick, ids per brick) of box-local 4^3 bricks of [z][y][x] arrays whose extents are multiples of 4."""
    nz, ny, nx = d.shape
    f = (d > 0).reshape(nz // 4, 4, ny // 4, 4, nx // 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(nz // 4, ny // 4, nx // 4, 64)
    i = np.where(d > 0, m, 0).reshape(nz // 4, 4, ny // 4, 4, nx // 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(nz // 4, ny // 4, nx // 4, 64)
    return f, i


@LAYOUTS
def test_masks_and_tree_follow_mixed_edits(keyed, mats):
    origin, shape = (-40, -44, -24), (136, 72, 64)              # content only in x < 64: the 64-cells beyond start empty
    d0, m0 = prior_with_empties(shape)
    d0[:, :, 64:] = 0.0
    m0[:, :, 64:] = 0
    xyz, mm = R.small_model()
    big = R.large_model()
    # a solid 12^3 block and its twin with other materials (the same voxels: a SET of the twin changes ids under unchanged masks)
    g = np.arange(12)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    block_m = (np.arange(len(block)) % 200 + 1).astype(np.uint32)
    t = _tracer()
    b = Both(t, keyed, origin, shape, d0, m0, [(xyz, mm % 250), big, (block, block_m), (block, block_m + np.uint32(7))])
    model = DenseModel(origin, shape)                           # for the brush and set_voxels, on the same arrays
    seen = {"emptied bricks": 0, "bricks in an empty 64-cell": 0, "ids under an unchanged mask": 0}

    def step(tag, fn):
        before = _bricks(b.d, b.m)
        empty_cells = [not (b.d[:, :, x0:x0 + 64] > 0).any() for x0 in (0, 64)]      # the slab x0 .. x0 + 64 of the box: all its 64-cells
        fn()
        after = _bricks(b.d, b.m)
        was, now = before[0].any(axis=-1), after[0].any(axis=-1)
        seen["emptied bricks"] += int((was & ~now).sum()) if tag.startswith("erase") else 0
        for k, x0 in enumerate((0, 64)):
            if empty_cells[k] and tag.startswith(("set", "keep")):
                seen["bricks in an empty 64-cell"] += int(now[:, :, x0 // 4:(x0 + 64) // 4].sum())
        if tag.startswith("set") and (before[0] == after[0]).all():
            seen["ids under an unchanged mask"] += int(((before[1] != after[1]).any(axis=-1)).sum())
        arrays_equal(t, b.d, b.m, tag)
        tree_equal(t, b.d, b.m, origin, mats, tag)

    def edit(fn_model, fn_device):
        model.density, model.ids = b.d, b.m
        fn_model(model)
        b.d, b.m = model.density, model.ids
        fn_device()

    step("upload", lambda: None)
    step("set block", lambda: b.stamp([(2, ((-20, -30, -10), (0, 1, 2), 0))], R.SET, 1.0))
    step("set twin: ids only", lambda: b.stamp([(3, ((-20, -30, -10), (0, 1, 2), 0))], R.SET, 1.0))
    step("set large into the empty cell", lambda: b.stamp([(1, ((62, -10, 8), (0, 1, 2), 0))], R.SET, 2.0))
    step("brush add", lambda: edit(lambda mdl: mdl.brush((10.5, -8.5, 4.5), 6.0, 1.0, 0), lambda: t.volume_apply_brush((10.5, -8.5, 4.5), 6.0, 1.0, 0)))
    step("keep small over the ball", lambda: b.stamp([(0, ((10, -8, 4), (2, 0, 1), 5)), (0, ((14, -9, 6), (1, 0, 2), 2))], R.KEEP, 0.5))
    step("erase block: whole bricks", lambda: b.stamp([(2, ((-20, -30, -10), (0, 1, 2), 0))], R.ERASE))
    pts = np.array([(-19, -29, -9), (-18, -29, -9), (70, 0, 0), (70, 0, 1)], dtype=np.int32)
    step("set_voxels", lambda: edit(lambda mdl: mdl.set_voxels(pts, [3, 4, 5, 6], [1.0, 0.0, 2.0, -1.0]), lambda: t.volume_set_voxels(pts, [3, 4, 5, 6], [1.0, 0.0, 2.0, -1.0])))
    step("erase large rotated", lambda: b.stamp([(1, ((60, -8, 6), (0, 2, 1), 2))], R.ERASE))
    step("brush dig", lambda: edit(lambda mdl: mdl.brush((60.5, -8.5, 8.5), 5.0, 0.0, 1), lambda: t.volume_apply_brush((60.5, -8.5, 8.5), 5.0, 0.0, 1)))
    step("keep large flipped", lambda: b.stamp([(1, ((20, 0, 10), (1, 0, 2), 7))], R.KEEP, 0.25))
    step("set table", lambda: b.stamp([(0, ((80, 10, 20), (0, 1, 2), 0)), (2, ((76, 6, 16), (2, 1, 0), 1)), (3, ((30, -40, -20), (0, 1, 2), 4))], R.SET, 1.0))
    step("erase table", lambda: b.stamp([(3, ((76, 6, 16), (2, 1, 0), 1)), (0, ((80, 10, 20), (0, 1, 2), 0))], R.ERASE))
    assert all(n > 0 for n in seen.values()), seen
    t.shutdown()


# ---- the refresh switch -------------------------------------------------------------------------------------------------------------

def test_a_large_stamp_takes_the_upload_path_of_a_keyed_volume(mats):
    """keyed_refresh switches at 65 536 bricks in an edit's range (blok_hip_debug.h: blok_hip_volume_refresh_counts)."""
    origin, shape = (-80, -84, -88), (168, 168, 168)
    rng = np.random.default_rng(23)
    sparse = np.unique(np.concatenate([rng.integers(0, 166, size=(20000, 3)), [[0, 0, 0], [165, 165, 165]]]).astype(np.int32), axis=0)
    sparse_m = rng.integers(1, 250, size=len(sparse)).astype(np.uint32)
    d0, m0 = prior((168, 168, 168), seed=9)
    t = _tracer()
    xyz, mm = R.small_model()
    b = Both(t, True, origin, shape, d0, m0, [(sparse, sparse_m), (xyz, mm % 250)])
    counts = t.volume_refresh_counts()
    big = ((-79, -83, -87), (0, 1, 2), 0)                       # box-local [1, 167) on every axis: bricks 0 .. 41, 42^3 = 74 088 > 65 536
    assert ((167 - 1) // 4 - 1 // 4 + 1) ** 3 > 65536
    b.stamp([(0, big)], R.SET, 1.0, "large")
    after_big = t.volume_refresh_counts()
    assert tuple(x - y for x, y in zip(after_big, counts)) == (0, 1, 0)
    tree_equal(t, b.d, b.m, origin, mats, "large")
    b.stamp([(1, ((5, 6, 7), (2, 0, 1), 3))], R.SET, 1.0, "small")
    assert tuple(x - y for x, y in zip(t.volume_refresh_counts(), after_big)) == (1, 0, 0)
    tree_equal(t, b.d, b.m, origin, mats, "small")
    t.shutdown()


# ---- the sun map --------------------------------------------------------------------------------------------------------------------

def test_sun_map_stays_valid_across_stamps(mats):
    """The scene of test_brush.py::test_sun_map_stays_valid_across_volume_edits.  A SET or KEEP stamp may fill voxels, which the shadow
    rays' last-occluder map has to be told (gpu_build.h: Edit::MayFill): every path-traced plane stays bit-identical with the map on and off.
    The tower stands on open ground in front of the first camera, so its shadow falls on visible terrain."""
    w, h = 160, 120
    t = _tracer(w, h)
    t.volume_create((0, 0, 0), (64, 96, 64), 128, 1.0)
    ids = W.scene_dense(64, SEED)
    z, y, x = np.nonzero(ids)
    t.volume_set_voxels(np.stack([x, y, z], 1).astype(np.int32), ids[z, y, x], np.ones(len(x), dtype=np.float32))
    t.volume_rebuild(mats)
    cams = [W.scene_camera(64, 0, w, h, SEED), W.camera_look_at((5.0, 30.0, 5.0), (40.0, 12.0, 40.0), 70.0, w, h)]
    g = np.stack(np.meshgrid(np.arange(5), np.arange(44), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    tower = t.model_create(g, np.full(len(g), 7, dtype=np.uint32))

    def same(tag):
        for cam in cams:
            t.set_sun_map(False)
            plain = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            t.set_sun_map(True)
            got = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            for k in plain:
                assert got[k].tobytes() == plain[k].tobytes(), (tag, k)

    same("scene")
    assert t.volume_stamp_models(ST.placement((30, 40, 30), model=tower), R.SET, 1.0) == len(g)      # above the terrain: a new shadow
    t.volume_rebuild(mats)
    same("set")
    assert t.volume_stamp_models(ST.placement((14, 84, 40), (1, 0, 2), 1, model=tower), R.KEEP, 1.0) > 0      # lying on its side, elsewhere
    t.volume_rebuild(mats)
    same("keep")
    assert t.volume_stamp_models(ST.placement((30, 40, 30), model=tower), R.ERASE) == len(g)
    t.volume_rebuild(mats)
    same("erase")
    t.shutdown()


# ---- a baked instance lies where the traced one was seen ----------------------------------------------------------------------------

BAKE_ORIENTATIONS = [((0, 1, 2), 0), ((0, 2, 1), 1), ((1, 0, 2), 2), ((1, 2, 0), 4), ((2, 0, 1), 7), ((2, 1, 0), 3), ((1, 2, 0), 5), ((0, 1, 2), 6)]
assert {a for a, _ in BAKE_ORIENTATIONS} == set(itertools.permutations((0, 1, 2)))
assert all(any((f >> k) & 1 for _, f in BAKE_ORIENTATIONS) for k in range(3))
NORMALS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.int64)      # blok_hit::face 0..5


def face_rays(d, origin):
    """For each filled voxel, each face whose three outward neighbour cells are empty (cells outside the box are): a ray from the face
    centre plus 3 along the normal, pointing back.  Every coordinate is a multiple of one half, so no ray grazes an edge.
    Returns (rays, voxel (n, 3) world, face (n,))."""
    f = np.pad(d > 0, 3)
    z, y, x = np.nonzero(d > 0)
    rays, voxels, faces = [], [], []
    for face, n in enumerate(NORMALS):
        free = np.ones(len(x), dtype=bool)
        for s in (1, 2, 3):
            free &= ~f[z + 3 + s * n[2], y + 3 + s * n[1], x + 3 + s * n[0]]
        v = np.stack([x[free], y[free], z[free]], axis=1).astype(np.int64) + np.asarray(origin, dtype=np.int64)
        r = np.zeros(len(v), dtype=_ffi.RAY)
        r["org"] = (v + 0.5 + 3.5 * n).astype(np.float32)
        r["dir"] = (-n).astype(np.float32)
        r["tmin"], r["tmax"] = 0.001, 10000.0
        rays.append(r); voxels.append(v); faces.append(np.full(len(v), face, dtype=np.uint8))
    return np.concatenate(rays), np.concatenate(voxels), np.concatenate(faces)


@LAYOUTS
def test_a_baked_instance_is_hit_where_the_traced_one_was(keyed, mats):
    origin, shape = (-20, -18, -14), (48, 40, 32)
    d0, m0 = prior(shape[::-1], seed=4)
    d0[d0 > 0] = 1.0
    xyz, mm = R.small_model()
    lx, lm = R.large_model()
    keep = (lx[:, 0] >= -12) & (lx[:, 0] < 10)                  # 22 x 9 x 21 of the large model: fits the box in every orientation
    model = (np.concatenate([lx[keep], xyz + np.int32([0, 8, 0])]), np.concatenate([lm[keep] % 150 + 100, mm % 150 + 100]).astype(np.uint32))
    t = _tracer()
    for axis, flip in BAKE_ORIENTATIONS:
        place = ((3, 2, 1), axis, flip)
        assert R.clipped(model[0], origin, shape[::-1], place) == 0
        b = Both(t, keyed, origin, shape, d0, m0, [model])
        inst = places([(0, place)], b.ids)
        # the final arrays, from the reference alone: KEEP is the composition's own tie rule, "a tie goes to the world"
        fd, fm = d0.copy(), m0.copy()
        written = R.stamp(fd, fm, origin, *model, place, R.KEEP, 1.0)
        assert written < len(model[1]), "the model overlaps none of the world's voxels"
        rays, voxels, faces = face_rays(fd, origin)
        local = voxels - np.asarray(origin)
        on_model = ~(d0[local[:, 2], local[:, 1], local[:, 0]] > 0)            # filled now, empty before: a model voxel
        assert len(rays) >= 500 and int(on_model.sum()) >= 50, (axis, flip, len(rays), int(on_model.sum()))
        # side B: the world unstamped, the model as an instance
        t.volume_rebuild(mats)
        hits_b, _ = t.trace_rays_instanced(rays, inst)
        # side A: baked
        assert t.volume_stamp_models(inst, R.KEEP, 1.0) == written
        arrays_equal(t, fd, fm, (axis, flip))
        t.volume_rebuild(mats)
        hits_a = t.trace_rays(rays)
        for hits in (hits_a, hits_b):
            assert (hits["hit"] == 1).all()
            assert (hits["voxel"].astype(np.int64) == voxels).all()
            assert (hits["face"] == faces).all()
            assert (hits["material_id"] == fm[local[:, 2], local[:, 1], local[:, 0]]).all()
        t.model_destroy(b.ids[0])
    t.shutdown()


# ---- capture ------------------------------------------------------------------------------------------------------------------------

def captured_equals_created(t, d, m, origin, lo, hi, tag, cut=False):
    """The captured model is the model model_create builds from the reference's list: both arrays and the info block."""
    xyz, mm = R.capture(d, m, origin, lo, hi)
    assert len(mm) > 0, tag
    got = t.volume_capture_model(lo, hi, cut=cut)
    assert t.last_capture_voxels == len(mm), tag
    want = t.model_create(xyz, mm)
    assert want == got + 1, tag
    gn, gm, gi = t.model_download(got)
    wn, wm, wi = t.model_download(want)
    assert gi == wi, (tag, gi, wi)
    assert gn.tobytes() == wn.tobytes(), (tag, "nodes", gn.shape, wn.shape)
    assert gm.tobytes() == wm.tobytes(), (tag, "materials")
    return got, gi


@LAYOUTS
def test_captured_models_equal_created_ones(keyed, mats):
    d0, m0 = prior_with_empties()
    m0[(d0 > 0.9) & (d0 < 1.4)] = 0                             # filled voxels with material id 0 are filled voxels
    # a region whose filled voxels start off the 16-grid: the first 21 / 18 / 35 layers of the region (-30, -40, -20) .. (50, 30, 38) are emptied
    d0[4:39, 4:74, 10:90] = 0.0
    d0[4:62, 4:74, 10:31] = 0.0
    d0[4:62, 4:22, 10:90] = 0.0
    t = _tracer()
    t.set_volume_layout(keyed)
    t.volume_create(ORIGIN, SHAPE)
    t.volume_upload(d0, m0)
    d, m = d0.copy(), m0.copy()
    regions = {"whole box": (None, None), "ragged": ((-31, -39, -13), (38, 21, 30)), "one thick in z": ((-8, -20, 20), (24, 4, 21)),
               "one thick in y": ((-40, 3, -24), (56, 4, 40)), "one thick in x": ((17, -44, -20), (18, 36, 33)),
               "off the 16-grid": ((-30, -40, -20), (50, 30, 38)), "one voxel": None}
    z, y, x = (int(v[0]) for v in np.nonzero((d > 0) & (m == 0)))
    regions["one voxel"] = ((x + ORIGIN[0], y + ORIGIN[1], z + ORIGIN[2]), (x + ORIGIN[0] + 1, y + ORIGIN[1] + 1, z + ORIGIN[2] + 1))
    for tag, (lo, hi) in regions.items():
        _, info = captured_equals_created(t, d, m, ORIGIN, lo, hi, tag)
        if tag == "off the 16-grid":
            assert all(c % 16 != 0 and c > 16 for c in info["lo"]) and any(o != 0 for o in info["origin"]), info
        if tag == "ragged":
            assert (R.capture(d, m, ORIGIN, lo, hi)[1] == 0).any()
    arrays_equal(t, d, m, "capture reads only")
    # an empty region: refused, no id consumed
    d[24:33, 44:53, 40:49] = 0.0
    m[24:33, 44:53, 40:49] = 0
    t.volume_set_voxels(np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32),
                        np.zeros(729, dtype=np.uint32), np.zeros(729, dtype=np.float32))
    arrays_equal(t, d, m, "emptied")
    with pytest.raises(BlokError) as e:
        t.volume_capture_model((0, 0, 0), (9, 9, 9))
    assert e.value.status == BLOK_ERR_UNSUPPORTED
    next_id = t.model_create(np.zeros((1, 3), dtype=np.int32), np.ones(1, dtype=np.uint32))
    # CUT: the model as before, the region's filled voxels cleared, the tree after a rebuild
    lo, hi = (-31, -39, -13), (38, 21, 30)
    got, _ = captured_equals_created(t, d, m, ORIGIN, lo, hi, "cut", cut=True)
    assert got == next_id + 1
    R.cut(d, m, ORIGIN, lo, hi)
    arrays_equal(t, d, m, "cut")
    tree_equal(t, d, m, ORIGIN, mats, "cut")
    t.shutdown()


def test_a_deep_captured_model_gets_its_stack(mats):
    """With only one-level models in the store, a captured model of four levels must refresh the descriptors and the stack depth the
    instance kernels size their LDS by: the frame with it equals the frame with its model_create twin."""
    w, h = 96, 64
    t = _tracer(w, h)
    origin, shape = (-8, -8, -8), (112, 48, 48)
    t.volume_create(origin, shape)
    d0, m0 = prior(shape[::-1], seed=6)
    m0 = np.ascontiguousarray(np.where(d0 > 0, m0 * 11 % 250, 0), dtype=np.uint32)
    t.volume_upload(d0, m0)
    small = t.model_create(np.array([(0, 0, 0), (3, 3, 3)], dtype=np.int32), np.array([1, 2], dtype=np.uint32))
    assert t.model_download(small)[2]["levels"] == 1
    lo, hi = (-6, -5, -4), (94, 30, 33)                         # 100 voxels along x: above 64, four levels
    deep = t.volume_capture_model(lo, hi)
    assert t.model_download(deep)[2]["levels"] == 4
    t.volume_upload(None, None)
    t.volume_set_voxels(np.array([(0, 0, 0)], dtype=np.int32), [5], [1.0])
    t.volume_rebuild(mats)                                      # a world of one voxel; the model hangs in front of the camera
    cam = W.camera_look_at((50.0, 60.0, -90.0), (50.0, 15.0, 15.0), 60.0, w, h)
    inst = ST.placement((0, 0, 0), (0, 1, 2), 0, deep)
    hits, ids, _ = t.trace_primary_instanced(cam, inst)
    assert (ids == 0).sum() > 500
    twin = t.model_create(*R.capture(d0, m0, origin, lo, hi))
    hits2, ids2, _ = t.trace_primary_instanced(cam, ST.placement((0, 0, 0), (0, 1, 2), 0, twin))
    assert records_equal(hits, hits2).all() and (ids == ids2).all()
    t.shutdown()


@LAYOUTS
def test_cut_and_carry(keyed, mats):
    d0, m0 = prior_with_empties()
    t = _tracer()
    t.set_volume_layout(keyed)
    t.volume_create(ORIGIN, SHAPE)
    t.volume_upload(d0, m0)
    d, m = d0.copy(), m0.copy()
    lo, hi = (-31, -39, -13), (-3, -10, 12)
    xyz, mm = R.capture(d, m, ORIGIN, lo, hi)
    rock = t.volume_capture_model(lo, hi, cut=True)
    R.cut(d, m, ORIGIN, lo, hi)
    place = ((20, 10, 5), (2, 0, 1), 5)
    want = R.stamp(d, m, ORIGIN, xyz, mm, place, R.SET, 0.75)
    assert t.volume_stamp_models(ST.placement(*place, model=rock), R.SET, 0.75) == want == len(mm)
    arrays_equal(t, d, m, "carried")
    tree_equal(t, d, m, ORIGIN, mats, "carried")
    t.shutdown()


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_change_nothing():
    t = _tracer()
    xyz, mm = R.small_model()
    with pytest.raises(BlokError) as e:                         # no volume
        t.volume_stamp_models(ST.placement((0, 0, 0)), R.SET, 1.0)
    assert e.value.status == BLOK_ERR_NO_WORLD
    with pytest.raises(BlokError) as e:
        t.volume_capture_model()
    assert e.value.status == BLOK_ERR_NO_WORLD
    d0, m0 = prior_with_empties(CLIP_SHAPE)
    t.volume_create(CLIP_ORIGIN, CLIP_SHAPE)
    t.volume_upload(d0, m0)
    model = t.model_create(xyz, mm)
    gone = t.model_create(xyz, mm)
    t.model_destroy(gone)
    good = ST.placement((2, 3, 1), model=model)

    def unchanged(tag):
        """The volume downloads as it was, and the store still holds gone + 1 models: the next id is unknown to it."""
        arrays_equal(t, d0, m0, tag)
        with pytest.raises(BlokError) as e:
            t.check_instances(ST.placement((0, 0, 0), model=gone + 1))
        assert f"unknown model {gone + 1}" in str(e.value), (tag, str(e.value))

    def refused(status, text, place=good, mode=R.SET, value=1.0):
        with pytest.raises(BlokError) as e:
            t.volume_stamp_models(place, mode, value)
        assert e.value.status == status and text in str(e.value), str(e.value)
        unchanged(text)

    refused(BLOK_ERR_INVALID_ARG, "unknown mode", mode=3)
    refused(BLOK_ERR_INVALID_ARG, "unknown mode", mode=-1)
    for value in (0.0, -1.0, float("nan"), float("inf")):
        refused(BLOK_ERR_INVALID_ARG, "density", value=value)
        refused(BLOK_ERR_INVALID_ARG, "density", mode=R.KEEP, value=value)
    # what blok_hip_check_instances checks, with its messages, naming the instance: the second record of the table is the bad one
    for field, bad, text in (("axis", (0, 0, 2), "instance 1: axis is not a permutation"), ("flip", 8, "instance 1: flip has bits"),
                             ("reserved", (0, 1, 0), "instance 1: reserved field"), ("model", 99, "instance 1: unknown model 99"),
                             ("model", gone, f"instance 1: unknown model {gone}"), ("offset", (40000, 0, 0), "instance 1: world box outside")):
        table = np.concatenate([good, good])
        table[field][1] = bad
        refused(BLOK_ERR_INVALID_ARG, text, place=table)
        with pytest.raises(BlokError) as e:
            t.check_instances(table)
        assert text in str(e.value)
    rc = _ffi.hip_lib().blok_hip_volume_stamp_models(t._ctx, None, 2, 0, 1.0, None)
    assert rc == BLOK_ERR_INVALID_ARG
    unchanged("null table")
    assert t.volume_stamp_models(good, R.ERASE, float("nan")) > 0          # ERASE ignores the density argument
    t.volume_upload(d0, m0)
    # capture
    import ctypes as C
    lib, out, n = _ffi.hip_lib(), C.c_uint32(77), C.c_uint64(5)
    lo3, hi3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4)
    for tag, status, args in (("lo alone", BLOK_ERR_INVALID_ARG, (lo3, None, 0, C.byref(out))), ("hi alone", BLOK_ERR_INVALID_ARG, (None, hi3, 0, C.byref(out))),
                              ("lo above hi", BLOK_ERR_INVALID_ARG, (hi3, lo3, 0, C.byref(out))), ("unknown flag", BLOK_ERR_INVALID_ARG, (lo3, hi3, 2, C.byref(out))),
                              ("null output", BLOK_ERR_INVALID_ARG, (lo3, hi3, 0, None)),
                              ("leaves the box below", BLOK_ERR_UNSUPPORTED, ((C.c_int32 * 3)(-10, 0, 0), hi3, 1, C.byref(out))),
                              ("leaves the box above", BLOK_ERR_UNSUPPORTED, (lo3, (C.c_int32 * 3)(4, 4, 12), 1, C.byref(out))),
                              ("an empty region holds nothing", BLOK_ERR_UNSUPPORTED, (lo3, lo3, 1, C.byref(out)))):
        n.value = 5
        assert lib.blok_hip_volume_capture_model(t._ctx, *args, C.byref(n)) == status, tag
        assert (out.value, n.value) == (77, 0), tag
        unchanged(tag)
    assert t.model_create(xyz, mm) == gone + 1                  # no refused call took a model id
    with pytest.raises(BlokError) as e:
        t.model_download(gone)
    assert e.value.status == BLOK_ERR_INVALID_ARG
    t.shutdown()
