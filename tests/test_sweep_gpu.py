"""GPU: blok_hip_volume_sweep_models against the numpy model of its contract (tests/sweep_reference.py): every result record for record,
and the volume byte for byte afterwards (a sweep reads only).  Both brick layouts unless said.  The shapes, scenes and cases are the
shared ones of sweep_reference.py, on which tests/test_sweep_cpu.py pins the host build and asserts what makes each of them hard.

Not covered: BLOK_ERR_UNSUPPORTED for a volume above 2^32 cells (its two arrays alone are 32 GiB).
Boxes at the ends of the int16 lattice and boxes of 16384 cells on one axis are covered in tests/test_volume_limits_gpu.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import stamp as ST
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import components_reference as CR
from tests import stamp_reference as SR
from tests import sweep_reference as R
from tests.conftest import SEED
from tests.volume_tree_reference import DenseModel, box_levels, reference_tree

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD = -1, -4
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
ORIGIN, SHAPE = R.ORIGIN, R.SHAPE


def _tracer(w=64, h=64):
    from blok_amd.tracer import HipTracer
    return HipTracer(w, h).init()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def prior_with_empties(shape_xyz=SHAPE):
    """terrain_cases.prior plus negative and NaN densities, as test_stamp_gpu.py builds it (the shared scenes start from it)."""
    return R.prior_with_empties(shape_xyz)


def ids_of(d):
    return np.ascontiguousarray(np.where(R.filled_cells(d), 5, 0).astype(np.uint32))


def arrays_equal(t, d, m, tag):
    gd, gm = t.volume_download()
    assert gd.tobytes() == d.tobytes(), (tag, "density", int((gd.view(np.uint32) != d.view(np.uint32)).sum()))
    assert gm.tobytes() == m.tobytes(), (tag, "ids", int((gm != m).sum()))


def as_tuples(records):
    return [(int(r["n_overlap"]), int(r["travel"]), int(r["blocked"])) for r in records]


def volume(t, keyed, d, m, origin=ORIGIN, shape=SHAPE):
    t.set_volume_layout(keyed)
    t.volume_create(origin, shape)
    t.volume_upload(d, m)


def create_models(t):
    return {name: t.model_create(xyz, np.arange(1, len(xyz) + 1, dtype=np.uint32)) for name, xyz in R.models().items()}


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------

@LAYOUTS
def test_every_shared_case_gives_the_reference_record(keyed):
    """One call per case, then the same cases as one table per (direction, max_distance, flags): both equal the reference."""
    t = _tracer()
    ids = None
    for scene, d in R.scenes().items():
        m = ids_of(d)
        volume(t, keyed, d, m)
        ids = ids or create_models(t)
        assert t.model_download(ids["bar"])[2]["levels"] >= 3
        cases, want = R.cases()[scene], R.expected(scene)
        groups = {}
        for i, (tag, name, place, direction, max_distance, flags) in enumerate(cases):
            got = as_tuples(t.volume_sweep_models(ST.placement(*place, model=ids[name]), direction, max_distance, flags))
            assert got == [want[i]], (scene, tag, got, want[i])
            groups.setdefault((direction, max_distance, flags), []).append(i)
        for (direction, max_distance, flags), members in groups.items():
            table = np.concatenate([ST.placement(*cases[i][2], model=ids[cases[i][1]]) for i in members])
            got = as_tuples(t.volume_sweep_models(table, direction, max_distance, flags))
            assert got == [want[i] for i in members], (scene, direction, max_distance, flags)
        arrays_equal(t, d, m, scene)
    t.shutdown()


# ---- one table, many placements -----------------------------------------------------------------------------------------------------

@LAYOUTS
def test_a_table_of_300_placements_equals_the_reference_and_the_single_calls(keyed):
    d = R.scenes()["thinned"]
    m = ids_of(d)
    t = _tracer()
    volume(t, keyed, d, m)
    ids = create_models(t)
    models = R.models()
    names = ("small", "cube", "ell", "comb", "bar")
    rng = np.random.default_rng(41)
    table = []
    for k in range(300):
        if k % 10 == 9:
            table.append(table[int(rng.integers(0, k))])       # a duplicate of an earlier placement
            continue
        name = names[int(rng.integers(0, len(names)))]
        axis, flip = SR.ORIENTATIONS[int(rng.integers(0, 48))]
        local = tuple(int(c) for c in rng.integers((-6, -6, -6), (SHAPE[0] + 6, SHAPE[1] + 6, SHAPE[2] + 6)))
        table.append((name, R.at(local, (axis, flip))))
    records = np.concatenate([ST.placement(*place, model=ids[name]) for name, place in table])
    for direction, max_distance, flags in ((3, 60, 0), (0, R.FAR, R.BOX_IS_SOLID), (5, 9, 0)):
        want = [R.sweep(d, ORIGIN, models[name], place, direction, max_distance, flags) for name, place in table]
        got = as_tuples(t.volume_sweep_models(records, direction, max_distance, flags))
        assert got == want, (direction, [i for i in range(300) if got[i] != want[i]][:5])
        singles = [as_tuples(t.volume_sweep_models(records[i:i + 1], direction, max_distance, flags))[0] for i in range(300)]
        assert singles == want
        assert len(set(want)) >= 20, len(set(want))
    arrays_equal(t, d, m, "table")
    assert len(t.volume_sweep_models(np.zeros(0, dtype=_ffi.INSTANCE), 3, 10)) == 0      # an empty table is fine
    t.shutdown()


@LAYOUTS
def test_several_teeth_with_the_same_minimum(keyed):
    """Three teeth of the comb, each in a brick column of its own, stop at the same distance: their waves race for the placement's
    result word and may give up on each other's value.  Sixty-four copies in one table, every answer the reference's."""
    d = R.scenes()["plate"]
    m = ids_of(d)
    t = _tracer()
    volume(t, keyed, d, m)
    comb = t.model_create(R.comb_model(), np.ones(len(R.comb_model()), dtype=np.uint32))
    place = R.at(R.COMB_TIE_AT)
    table = np.concatenate([ST.placement(*place, model=comb)] * 64)
    for max_distance in (100, 3, 4, R.FAR):
        want = R.sweep(d, ORIGIN, R.comb_model(), place, 3, max_distance)
        assert want[1] == 3
        assert as_tuples(t.volume_sweep_models(table, 3, max_distance)) == [want] * 64
    arrays_equal(t, d, m, "combs")
    t.shutdown()


# ---- cut and drop -------------------------------------------------------------------------------------------------------------------

@LAYOUTS
def test_cut_and_drop(keyed, mats):
    """A pillar on a ground plate, severed by a SUBTRACT brush: the floating top is found by its label, lifted out with CUT, swept down
    and stamped where it comes to rest, on the stub."""
    origin, shape = (-20, -18, -14), (48, 40, 32)
    model = DenseModel(origin, shape)
    model.density[:, 0:2, :] = 1.0
    model.density[14:18, 2:36, 22:26] = 1.5                     # 4 x 4 across, box-local y 2 .. 35
    model.ids[model.density > 0] = 3
    model.ids[14:18, 2:36, 22:26] += np.arange(34, dtype=np.uint32)[None, :, None]
    t = _tracer()
    volume(t, keyed, model.density.copy(), model.ids.copy(), origin, shape)
    centre = (origin[0] + 24.0, origin[1] + 20.0, origin[2] + 16.0)
    model.brush(centre, 5.0, 0.0, 1)
    t.volume_apply_brush(centre, 5.0, 0.0, 1)
    d, m = model.density, model.ids
    arrays_equal(t, d, m, "severed")
    filled_before = int((d > 0).sum())
    n_components, _ = t.volume_label_components()
    labels, records = CR.label(d, origin)
    assert n_components == len(records) == 2
    floating = records[records["touches"] & 8 == 0]
    assert len(floating) == 1
    rec = floating[0]
    column = d[15, :, 23] > 0                                   # one column of the pillar, box-local y
    top_lo = int(rec["lo"][1]) - origin[1]
    gap = top_lo - 1 - int(np.nonzero(column[:top_lo])[0].max())
    assert gap >= 8 and all((d[z, :, x] > 0).tolist() == column.tolist() for z in range(14, 18) for x in range(22, 26)), "the cut is flat"
    xyz, mm, _ = CR.members(d, m, origin, (labels, None, None), rec)
    piece, at = t.volume_capture_component(int(rec["label"]), cut=True)
    assert at == tuple(int(c) for c in rec["lo"]) and t.last_capture_voxels == len(mm)
    CR.clear_members(d, m, origin, (labels, None, None), rec)
    arrays_equal(t, d, m, "cut")
    got = as_tuples(t.volume_sweep_models(ST.placement(at, model=piece), 3, shape[1], R.BOX_IS_SOLID))[0]
    assert got == R.sweep(d, origin, xyz, (at, (0, 1, 2), 0), 3, shape[1], R.BOX_IS_SOLID) == (0, gap, 1)
    rest = (at[0], at[1] - got[1], at[2])
    want = SR.stamp(d, m, origin, xyz, mm, (rest, (0, 1, 2), 0), SR.SET, 1.5)
    assert t.volume_stamp_models(ST.placement(rest, model=piece), SR.SET, 1.5) == want == len(mm)
    arrays_equal(t, d, m, "dropped")
    assert int((d > 0).sum()) == filled_before
    assert as_tuples(t.volume_sweep_models(ST.placement(rest, model=piece), 3, 5))[0] == (len(mm), 0, 1)      # it lies there now
    st = t.volume_rebuild(mats)
    levels = box_levels(shape)
    ref_nodes, ref_mats = reference_tree(d > 0, m, levels)
    assert (st.n_voxels, st.n_tree_nodes, st.levels, tuple(st.origin)) == (len(ref_mats), len(ref_nodes), levels, tuple(origin))
    nodes, ids = t.download_tree()
    assert nodes.tobytes() == ref_nodes.tobytes() and ids.tobytes() == ref_mats.tobytes()
    assert t.volume_label_components()[0] == 1
    t.shutdown()


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_change_nothing():
    t = _tracer()
    lib = _ffi.hip_lib()
    xyz, mm = SR.small_model()
    with pytest.raises(BlokError) as e:                         # no volume
        t.volume_sweep_models(ST.placement((0, 0, 0)), 3, 10)
    assert e.value.status == BLOK_ERR_NO_WORLD
    d0, m0 = prior_with_empties((24, 20, 16))
    t.volume_create((-9, -7, -5), (24, 20, 16))
    t.volume_upload(d0, m0)
    model = t.model_create(xyz, mm)
    gone = t.model_create(xyz, mm)
    t.model_destroy(gone)
    good = ST.placement((2, 3, 1), model=model)
    n_components, _ = t.volume_label_components()
    snapshot = t.volume_components_download(0, n_components).tobytes()

    def refused(text, table=good, direction=3, flags=0, null_results=False):
        inst = np.ascontiguousarray(table, dtype=_ffi.INSTANCE).reshape(-1)
        out = np.full(max(len(inst), 1), 77, dtype=_ffi.SWEEP_RESULT)
        rc = lib.blok_hip_volume_sweep_models(t._ctx, _ffi.ptr(inst), len(inst), direction, 10, flags, None if null_results else _ffi.ptr(out))
        assert rc == BLOK_ERR_INVALID_ARG, text
        assert text in lib.blok_hip_last_error(t._ctx).decode(), (text, lib.blok_hip_last_error(t._ctx))
        assert (out["travel"] == 77).all() and (out["n_overlap"] == 77).all() and (out["blocked"] == 77).all(), text
        arrays_equal(t, d0, m0, text)

    refused("direction", direction=6)
    refused("direction", direction=0xFFFFFFFF)
    refused("unknown flag bits", flags=2)
    refused("unknown flag bits", flags=0x80000001)
    refused("null result array", null_results=True)
    for field, bad, text in (("axis", (0, 0, 2), "instance 1: axis is not a permutation"), ("flip", 8, "instance 1: flip has bits"),
                             ("reserved", (0, 1, 0), "instance 1: reserved field"), ("model", 99, "instance 1: unknown model 99"),
                             ("model", gone, f"instance 1: unknown model {gone}"), ("offset", (40000, 0, 0), "instance 1: world box outside")):
        table = np.concatenate([good, good])
        table[field][1] = bad
        refused(text, table=table)
        with pytest.raises(BlokError) as e:
            t.check_instances(table)
        assert text in str(e.value)
    out = np.full(2, 77, dtype=_ffi.SWEEP_RESULT)
    assert lib.blok_hip_volume_sweep_models(t._ctx, None, 2, 3, 10, 0, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG
    assert (out["travel"] == 77).all()
    assert lib.blok_hip_volume_sweep_models(t._ctx, None, 0, 3, 10, 0, None) == 0
    # a good call still answers, and neither it nor the refusals disturbed the snapshot
    want = R.sweep(d0, (-9, -7, -5), xyz, ((2, 3, 1), (0, 1, 2), 0), 3, 10)
    assert as_tuples(t.volume_sweep_models(good, 3, 10)) == [want]
    assert t.volume_components_download(0, n_components).tobytes() == snapshot
    arrays_equal(t, d0, m0, "after all")
    t.shutdown()
