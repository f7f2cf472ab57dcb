"""GPU: blok_hip_volume_stamp_affine against the numpy model of its contract (tests/affine_reference.py): the volume's arrays byte for byte
and the count after every call, the rebuilt tree against volume_tree_reference, blok_hip_volume_stamp_models at exponent 0, a baked scaled
instance against the traced one.  Both brick layouts.

The ways a wave of the kernel (blok_amd/csrc/hip/affine_kernels.hip) can go, and the case of affine_reference.CASES that takes each — PATHS
below, checked against the rule itself by affine_reference.tile_classes:
    a tile wholly outside the model's interval        "yaw 30" (the corners of the box the turned model does not reach)
    the uniform descent leaving at an empty child     "scale 16, sparse" (a tile is one brick of the model, and most of its bricks are empty)
    a tile cut by the model's box                     "yaw 30"
    a whole wave inside one model voxel               "scale 8, a region 8 cells wide"
    lanes in far-apart bricks                         "scale 1/64, sparse"
    a row step skipped                                "compound rotation, scale 1.5"
    a region of one cell                              "one cell"
    a region ending at x = 63, 64 and 65 cells        "x ends at 63", "x ends at 64", "x ends at 65"

Not covered: BLOK_ERR_UNSUPPORTED for a volume above 2^32 cells (its two arrays alone are 32 GiB)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import affine as AF
from blok_amd import stamp as ST
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import affine_reference as R
from tests import stamp_reference as SR
from tests.conftest import SEED
from tests.test_affine_cpu import clip_region, prior_with_empties, to_affine
from tests.volume_tree_reference import box_levels, reference_tree

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
BOXES = pytest.mark.parametrize("origin,shape", [(R.ORIGIN, R.SHAPE), (R.ODD_ORIGIN, R.ODD_SHAPE)], ids=["box", "odd box"])
MODES = (R.SET, R.KEEP, R.ERASE)

PATHS = {"outside": "yaw 30", "empty cell": "scale 16, sparse", "cut": "yaw 30", "one voxel": "scale 8, a region 8 cells wide", "far apart": "scale 1/64, sparse",
         "row skipped": "compound rotation, scale 1.5"}


def _tracer(w=64, h=64):
    from blok_amd.tracer import HipTracer
    return HipTracer(w, h).init()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def arrays_equal(t, d, m, tag):
    gd, gm = t.volume_download()
    assert gd.tobytes() == d.tobytes(), (tag, "density", int((gd.view(np.uint32) != d.view(np.uint32)).sum()))
    assert gm.tobytes() == m.tobytes(), (tag, "ids", int((gm != m).sum()))


def tree_equal(t, d, m, origin, mats, tag):
    st = t.volume_rebuild(mats)
    levels = box_levels(d.shape[::-1])
    ref_nodes, ref_mats = reference_tree(d > 0, m, levels)
    assert (st.n_voxels, st.n_tree_nodes, st.levels, tuple(st.origin)) == (len(ref_mats), len(ref_nodes), levels, tuple(origin)), tag
    nodes, ids = t.download_tree()
    assert nodes.tobytes() == ref_nodes.tobytes(), (tag, "nodes")
    assert ids.tobytes() == ref_mats.tobytes(), (tag, "materials")


class Both:
    """The same calls to the volume and to the reference arrays."""

    def __init__(self, t, keyed, origin, shape, d0, m0):
        self.t, self.origin, self.shape = t, origin, shape
        t.set_volume_layout(keyed)
        t.volume_create(origin, shape)
        t.volume_upload(d0, m0)
        self.d, self.m = d0.copy(), m0.copy()
        self.ids = {name: t.model_create(*model) for name, model in R.MODELS.items()}

    def stamp(self, table, mode, value=1.5, tag=None):
        """table: [(model name, AFFINE record, region or None)] with one region for all, one call."""
        region = table[0][2]
        lo, hi = clip_region(region, self.origin, self.shape)
        want = 0
        recs = []
        for name, rec, _ in table:
            want += R.stamp(self.d, self.m, self.origin, *R.MODELS[name], rec, lo, hi, mode, value)
            rec = rec.copy()
            rec["model"] = self.ids[name]
            recs.append(rec)
        got = self.t.volume_stamp_affine(np.concatenate(recs), lo, hi, mode, value)
        assert got == want, (tag, got, want)
        arrays_equal(self.t, self.d, self.m, tag)
        return want


def test_the_named_cases_take_the_named_paths():
    for path, name in PATHS.items():
        model, spec, region = R.CASES[name]
        lo, hi = clip_region(region, R.ORIGIN, R.SHAPE)
        classes = R.tile_classes(to_affine(spec), R.ORIGIN, R.SHAPE, lo, hi, *R.MODELS[model])
        assert classes[path] > 0 and classes["tiles"] > classes[path], (path, name, classes)
    assert _ffi.hip_lib().blok_hip_abi_version() >= (1 << 16) | 18


@LAYOUTS
@BOXES
def test_the_matrix_table_gives_the_reference_arrays_and_tree(keyed, origin, shape, mats):
    t = _tracer()
    b = Both(t, keyed, origin, shape, *prior_with_empties(shape))
    written = {mode: 0 for mode in MODES}
    for k, (name, (model, spec, region)) in enumerate(R.CASES.items()):
        rec = to_affine(spec)
        for mode in MODES:
            if mode != R.SET:                                   # KEEP and ERASE meet the prior content, not the SET just made
                b.t.volume_upload(*prior_with_empties(shape))
                b.d, b.m = prior_with_empties(shape)
            written[mode] += b.stamp([(model, rec, region)], mode, 0.5 + k, (name, mode))
    assert all(n > 10000 for n in written.values()), written
    tree_equal(t, b.d, b.m, origin, mats, "after the table")
    # a plain set_voxels and a rebuild afterwards: the dirty flags the stamps left were right
    pts = np.array([origin, (origin[0] + 5, origin[1] + 6, origin[2] + 7), (origin[0] + shape[0] - 1, origin[1] + shape[1] - 1, origin[2] + shape[2] - 1)], dtype=np.int32)
    t.volume_set_voxels(pts, [3, 4, 5], [1.0, 0.0, 2.0])
    for p, mm, dd in zip(pts, (3, 4, 5), (1.0, 0.0, 2.0)):
        c = tuple(int(v) for v in (p - np.asarray(origin))[::-1])
        b.d[c], b.m[c] = dd, mm
    b.stamp([("block", to_affine(R.CASES["shear"][1]), None)], R.ERASE, 1.0, "erase after set_voxels")
    tree_equal(t, b.d, b.m, origin, mats, "after set_voxels")
    t.shutdown()


@LAYOUTS
def test_exponent_zero_equals_stamp_models(keyed):
    t = _tracer()
    d0, m0 = prior_with_empties(R.SHAPE)
    b = Both(t, keyed, R.ORIGIN, R.SHAPE, d0, m0)
    rng = np.random.default_rng(17)
    table = []
    for k, (axis, flip) in enumerate(SR.ORIENTATIONS):
        name = "small" if k % 3 else "large"
        table.append(ST.placement(tuple(int(v) for v in rng.integers((-34, -38, -18), (50, 30, 34))), axis, flip, b.ids[name]))
    table = np.concatenate(table)
    records = np.concatenate([AF.from_instance(p) for p in table])
    for mode in MODES:
        t.volume_upload(d0, m0)
        n_models = t.volume_stamp_models(table, mode, 1.25)
        want = t.volume_download()
        t.volume_upload(d0, m0)
        assert t.volume_stamp_affine(records, None, None, mode, 1.25) == n_models > 0
        arrays_equal(t, *want, ("48 orientations", mode))
    t.shutdown()


@LAYOUTS
def test_a_baked_scaled_instance_is_seen_where_the_traced_one_was(keyed, mats):
    """set_scale 1, 2, 3: the baked volume traced as the world against the world plus the traced scaled instance: hit, material and face
    per pixel.  (t and the voxel are not compared: the two walks use different cell sizes.)"""
    w, h = 96, 64
    t = _tracer(w, h)
    t.set_volume_layout(keyed)
    models = {name: (R.MODELS[name][0], (R.MODELS[name][1] % 150 + 100).astype(np.uint32)) for name in ("small", "block")}
    cases = [(1, "block", ((4, -6, 10), (0, 1, 2), 0)), (2, "block", ((10, -4, 6), (2, 0, 1), 3)), (3, "small", ((0, -10, 2), (1, 2, 0), 5)),
             (3, "small", ((0, -10, 0), (0, 1, 2), 0))]
    far = np.array([(R.ORIGIN[0], R.ORIGIN[1], R.ORIGIN[2])], dtype=np.int32)      # the world's one own voxel, in a corner no model reaches
    for e, name, (offset, axis, flip) in cases:
        t.volume_create(R.ORIGIN, R.SHAPE)
        t.volume_set_voxels(far, [7], [1.0])
        t.volume_rebuild(mats)
        model = t.model_create(*models[name])
        t.model_set_scale(model, e)
        place = ST.placement(offset, axis, flip, model)
        t.check_instances(place)
        rec = AF.from_instance(place, e)
        d = np.zeros(tuple(R.SHAPE)[::-1], dtype=np.float32)
        m = np.zeros(tuple(R.SHAPE)[::-1], dtype=np.uint32)
        d[0, 0, 0], m[0, 0, 0] = 1.0, 7
        want = R.stamp(d, m, R.ORIGIN, *models[name], rec, None, None, R.SET, 1.0)
        assert want == len(models[name][1]) * 8 ** e, "the scaled model is clipped by the box"
        for cam in (W.camera_look_at((70.0, 60.0, 90.0), (8.0, -4.0, 8.0), 60.0, w, h), W.camera_look_at((-60.0, 10.0, -70.0), (8.0, -4.0, 8.0), 55.0, w, h)):
            hits_b, ids_b, _ = t.trace_primary_instanced(cam, place)
            assert (ids_b == 0).sum() > 100, (e, name)
            assert t.volume_stamp_affine(rec, None, None, R.SET, 1.0) == want      # the entry takes the scaled model; its exponent is not looked at
            arrays_equal(t, d, m, (e, name))
            t.volume_rebuild(mats)
            hits_a, _, _ = t.trace_primary_instanced(cam, np.zeros(0, dtype=_ffi.INSTANCE))
            for field in ("hit", "material_id", "face"):
                assert (hits_a[field] == hits_b[field]).all(), (e, name, field, int((hits_a[field] != hits_b[field]).sum()))
            t.volume_upload(None, None)                         # back to the world's one voxel for the next camera
            t.volume_set_voxels(far, [7], [1.0])
            t.volume_rebuild(mats)
        with pytest.raises(BlokError) as err:                   # the other volume entries still refuse the scaled model
            t.volume_stamp_models(place, R.SET, 1.0)
        assert err.value.status == BLOK_ERR_UNSUPPORTED
        t.model_destroy(model)
    t.shutdown()


@LAYOUTS
def test_tables_apply_in_order_and_keep_counts_what_it_filled(keyed):
    t = _tracer()
    d0, m0 = prior_with_empties(R.SHAPE)
    b = Both(t, keyed, R.ORIGIN, R.SHAPE, d0, m0)
    a = to_affine(R.CASES["yaw 30"][1])
    c = to_affine(R.CASES["mirror"][1])
    s = to_affine(R.CASES["scale 12, every side"][1])
    # the two placements of the large model overlap, and disagree where they do
    da, ma, db, mb = (np.zeros_like(x) for x in (d0, m0, d0, m0))
    R.stamp(da, ma, R.ORIGIN, *R.MODELS["large"], a, None, None, R.SET, 1.0)
    R.stamp(db, mb, R.ORIGIN, *R.MODELS["large"], c, None, None, R.SET, 1.0)
    overlap = (da > 0) & (db > 0)
    assert overlap.sum() > 100 and (ma[overlap] != mb[overlap]).any()
    b.stamp([("large", a, None), ("large", c, None)], R.SET, 1.25, "pair")
    assert (b.m[overlap] == mb[overlap]).all()                  # the later one wins
    b.stamp([("large", c, None), ("large", a, None)], R.SET, 1.25, "pair reversed")
    assert (b.m[overlap] == ma[overlap]).all()
    # KEEP counts the cells that were empty and got filled: the second record finds the first one's cells taken
    t.volume_upload(d0, m0)
    b.d, b.m = d0.copy(), m0.copy()
    empty_before = int((~(d0 > 0)).sum())
    n = b.stamp([("large", a, None), ("block", s, None), ("large", c, None)], R.KEEP, 0.75, "keep")
    assert n == empty_before - int((~(b.d > 0)).sum()) > 0
    assert b.stamp([("large", a, None), ("block", s, None), ("large", c, None)], R.KEEP, 0.75, "keep again") == 0
    b.stamp([("block", s, None), ("large", a, None)], R.ERASE, 1.0, "erase")
    assert t.volume_stamp_affine(np.zeros(0, dtype=_ffi.AFFINE)) == 0      # an empty table is fine
    arrays_equal(t, b.d, b.m, "empty table")
    t.shutdown()


def test_refused_calls_change_nothing():
    t = _tracer()
    good = AF.from_instance(ST.placement((2, 3, 1)))
    with pytest.raises(BlokError) as e:                         # no volume
        t.volume_stamp_affine(good)
    assert e.value.status == BLOK_ERR_NO_WORLD
    origin, shape = (-9, -7, -5), (24, 20, 16)
    d0, m0 = prior_with_empties(shape)
    t.volume_create(origin, shape)
    t.volume_upload(d0, m0)
    model = t.model_create(*R.MODELS["small"])
    gone = t.model_create(*R.MODELS["small"])
    t.model_destroy(gone)
    good["model"] = model

    def refused(status, text, rec=good, lo=None, hi=None, mode=R.SET, value=1.0):
        with pytest.raises(BlokError) as e:
            t.volume_stamp_affine(rec, lo, hi, mode, value)
        assert e.value.status == status and text in str(e.value), str(e.value)
        arrays_equal(t, d0, m0, text)

    def second(field, value):
        """A table of two records, the second one changed."""
        table = np.concatenate([good, good])
        table[field][1] = value
        return table

    refused(BLOK_ERR_INVALID_ARG, "unknown mode", mode=3)
    refused(BLOK_ERR_INVALID_ARG, "unknown mode", mode=-1)
    for value in (0.0, -1.0, float("nan"), float("inf")):
        refused(BLOK_ERR_INVALID_ARG, "density", value=value)
        refused(BLOK_ERR_INVALID_ARG, "density", mode=R.KEEP, value=value)
    refused(BLOK_ERR_INVALID_ARG, "record 1: unknown model 99", rec=second("model", 99))
    refused(BLOK_ERR_INVALID_ARG, f"record 1: unknown model {gone}", rec=second("model", gone))
    refused(BLOK_ERR_INVALID_ARG, "record 1: reserved", rec=second("reserved", (0, 0, 0, 0, 2)))
    m = good["m"][0].copy()
    m[2, 0] = -(1 << 22) - 1
    refused(BLOK_ERR_INVALID_ARG, "record 1: |m|", rec=second("m", m))
    refused(BLOK_ERR_INVALID_ARG, "record 1: |t|", rec=second("t", (0, 0, (1 << 40) + 1)))
    refused(BLOK_ERR_INVALID_ARG, "record 1: a cell of the box", rec=second("anchor", (14 - (1 << 20), 0, 0)))
    refused(BLOK_ERR_INVALID_ARG, "record 1: a cell of the box", rec=second("anchor", (0, -7 + (1 << 20), 0)))
    refused(BLOK_ERR_INVALID_ARG, "one region pointer", lo=(0, 0, 0))
    refused(BLOK_ERR_INVALID_ARG, "one region pointer", hi=(1, 1, 1))
    refused(BLOK_ERR_INVALID_ARG, "region_lo above", lo=(2, 2, 2), hi=(3, 1, 3))
    refused(BLOK_ERR_UNSUPPORTED, "leaves", lo=(-10, 0, 0), hi=(3, 3, 3))
    refused(BLOK_ERR_UNSUPPORTED, "leaves", lo=(0, 0, 0), hi=(3, 3, 12))
    n = C.c_uint64(5)
    assert _ffi.hip_lib().blok_hip_volume_stamp_affine(t._ctx, None, 2, None, None, 0, 1.0, C.byref(n)) == BLOK_ERR_INVALID_ARG
    assert n.value == 0
    arrays_equal(t, d0, m0, "null table")
    # legal: the limits met exactly, an empty region, ERASE with any density
    edge = good.copy()
    edge["anchor"] = (14 - (1 << 20) + 1, 0, -5 + (1 << 20) - 1)
    edge["m"][0, 0, 0], edge["t"][0, 1] = 1 << 22, -(1 << 40)
    d, mm = d0.copy(), m0.copy()
    want = R.stamp(d, mm, origin, *R.MODELS["small"], edge, None, None, R.SET, 1.0)
    assert t.volume_stamp_affine(edge) == want
    arrays_equal(t, d, mm, "at the limits")
    t.volume_upload(d0, m0)
    assert t.volume_stamp_affine(good, (1, 1, 1), (1, 5, 5)) == 0
    arrays_equal(t, d0, m0, "empty region")
    assert t.volume_stamp_affine(good, None, None, R.ERASE, float("nan")) == len(R.MODELS["small"][1])
    t.shutdown()
