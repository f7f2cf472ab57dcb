"""GPU: emissive models as lights (include/blok_hip.h, "emissive models as lights"): the device's model tables against the
host build, byte for byte, with their errors and their life; the prefix kernel of an instance table against the numpy rule of
tests/model_lights_reference.py, exactly, with the overflow pair — through blok_hip_instance_lights_info, with no frame."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, BlokError
from tests import instance_oracle as IO
from tests import model_lights_cases as MC
from tests import model_lights_reference as MR

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG = -1
CASES = MC.table()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def tracer(mats=None, a_world_plate=False):
    """A tracer over a small resident volume (a floor; with a_world_plate a glowing 2 x 2 plate and the world's light table of it)."""
    from blok_amd.tracer import HipTracer
    t = HipTracer(64, 48).init()
    d = np.zeros((16, 16, 16), dtype=np.float32)
    m = np.zeros((16, 16, 16), dtype=np.uint32)
    d[:, 0, :], m[:, 0, :] = 1.0, MC.GREY
    if a_world_plate:
        d[4:6, 8, 4:6], m[4:6, 8, 4:6] = 1.0, MC.GLOW
    t.volume_create((0, 0, 0), (16, 16, 16))
    t.volume_upload(d, m)
    t.volume_rebuild(MC.materials() if mats is None else mats)
    if a_world_plate:
        t.volume_extract_quads()
        assert int(LT.from_quads(t)["n_faces"][0]) == 2 * 4 + 4 * 2
    return t


def same_table(t, model, want):
    info = LT.model_lights_info(t, model)
    assert (int(info["n"][0]), int(info["n_faces"][0]), int(info["bytes"][0])) == (len(want), len(want), 32 * len(want))
    assert LT.model_lights_download(t, model).tobytes() == want.tobytes()


def test_device_table_equals_the_host_build_over_the_case_table(torch_cuda):
    t = tracer()
    installed = None
    for case in CASES:
        if installed is None or installed.tobytes() != case.materials.tobytes():
            t.volume_rebuild(case.materials)
            installed = case.materials
        model = t.model_create(case.xyz, case.ids)
        want = LT.host_model_lights(case.xyz, case.ids, case.materials)
        info = LT.model_lights(t, model)
        print(f"{case.name}: {len(want)} faces")
        assert int(info["n"][0]) == len(want) and (case.n_faces is None or len(want) == case.n_faces)
        same_table(t, model, want)
        if len(want) > 7:                                # in pieces, and ranges at and past the end
            pieces = LT.model_lights_download(t, model, page=5)
            assert pieces.tobytes() == want.tobytes()
            assert LT.model_lights_download(t, model, 3, 4).tobytes() == want[3:7].tobytes()
            assert len(LT.model_lights_download(t, model, len(want), 0)) == 0
            with pytest.raises(BlokError) as e:
                LT.model_lights_download(t, model, len(want) - 1, 2)
            assert e.value.status == BLOK_ERR_INVALID_ARG
    t.shutdown()


def test_a_captured_model_gets_the_table_of_its_voxels(torch_cuda):
    """A tree the device built (a region of the volume captured as a model) is walked like one the host built."""
    t = tracer(a_world_plate=True)
    model = t.volume_capture_model((3, 7, 3), (8, 10, 8))
    assert t.last_capture_voxels == 4
    info = LT.model_lights(t, model)
    assert int(info["n"][0]) == 2 * 4 + 4 * 2
    got = LT.model_lights_download(t, model)
    _, mats, minfo = t.model_download(model)
    assert (got["material"] == MC.GLOW).all() and len(mats) == 4 and got["cum"].tolist() == list(range(16))
    lo = np.array(minfo["lo"])
    plus = np.stack([got["face"] == 0, got["face"] == 2, got["face"] == 4], axis=1)
    voxels = {tuple(v) for v in (got["lo"] - plus - lo).tolist()}
    assert voxels == {(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)}
    t.shutdown()


def test_every_error_leaves_the_old_table_and_the_life_of_a_table(torch_cuda):
    t = tracer()
    lantern = MC.cube(3)
    ids = np.full(len(lantern), MC.GLOW, dtype=np.uint32)
    want = LT.host_model_lights(lantern, ids, MC.materials())
    a, b = t.model_create(lantern, ids), t.model_create(lantern[:1], ids[:1])
    LT.model_lights(t, a)
    LT.model_lights(t, b)
    for call in (lambda: t._check(t._lib.blok_hip_model_lights(t._ctx, a, 1, None)), lambda: LT.model_lights(t, 99),
                 lambda: LT.model_lights_info(t, 99), lambda: LT.model_lights_download(t, 99), lambda: LT.model_lights_clear(t, 99)):
        with pytest.raises(BlokError) as e:
            call()
        assert e.value.status == BLOK_ERR_INVALID_ARG
        same_table(t, a, want)
    # a change of scale keeps the table: the records are in model cells
    t.model_set_scale(a, 3)
    same_table(t, a, want)
    header, icum = LT.instance_lights_info(t, np.array([IO.instance(a, (40, 40, 40)), IO.instance(b, (0, 20, 0))], dtype=INSTANCE))
    assert icum.tolist() == [0, 54 * 64, 54 * 64 + 6] and int(header["n_lit"][0]) == 2
    # clear drops one; a rebuilt table of no faces drops too
    LT.model_lights_clear(t, b)
    assert int(LT.model_lights_info(t, b)["n"][0]) == 0
    same_table(t, a, want)
    grey = t.model_create(lantern, np.full(len(lantern), MC.GREY, dtype=np.uint32))
    assert int(LT.model_lights(t, grey)["n"][0]) == 0 and len(LT.model_lights_download(t, grey)) == 0
    # destroy frees it (the id is unknown from then on) and leaves the others
    c = t.model_create(lantern, ids)
    LT.model_lights(t, c)
    t.model_destroy(c)
    with pytest.raises(BlokError):
        LT.model_lights_info(t, c)
    same_table(t, a, want)
    # every call that installs another material table drops them all: a rebuild of the volume ...
    t.volume_rebuild(MC.materials())
    assert int(LT.model_lights_info(t, a)["n"][0]) == 0
    header, icum = LT.instance_lights_info(t, np.array([IO.instance(a, (40, 40, 40))], dtype=INSTANCE))
    assert icum.tolist() == [0, 0] and int(header["a_total"][0]) == 0
    LT.model_lights(t, a)                                # (built again under the new table)
    same_table(t, a, want)
    # ... and an uploaded world
    from tests import oracle_ffi as O
    ow = O.OracleWorld(128, 1.0)
    ow.set_voxels(np.array([(0, 0, 0), (1, 0, 0)], dtype=np.int32), np.array([1, 1], dtype=np.uint32))
    ow.rebuild()
    nodes, subs = ow.pack()
    t.add_world(W.PackedWorld(nodes, subs, MC.materials()))
    assert int(LT.model_lights_info(t, a)["n"][0]) == 0
    LT.model_lights(t, a)
    same_table(t, a, want)
    t.shutdown()


def test_no_material_table_is_an_error(torch_cuda):
    from blok_amd.tracer import HipTracer
    t = HipTracer(64, 48).init()
    model = t.model_create(MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32))
    with pytest.raises(BlokError) as e:
        LT.model_lights(t, model)
    assert e.value.status == BLOK_ERR_INVALID_ARG
    t.shutdown()


# ---- the prefix ------------------------------------------------------------------------------------------------------------------------------
def _store(t):
    """Models of exponents 0, 1 and 3 with tables, one without, one destroyed; and their description for the numpy rule."""
    lantern = MC.cube(3)
    glow = np.full(27, MC.GLOW, dtype=np.uint32)
    bar = np.array([(x, 0, 0) for x in range(-2, 5)], dtype=np.int32)
    ids, models = [], {}
    for n, (xyz, mat, e, lit) in enumerate(((lantern, glow, 0, True), (bar, np.full(7, MC.GLOW2, dtype=np.uint32), 1, True), (lantern, glow, 3, True),
                                            (lantern, glow, 0, False), (lantern, glow, 0, True))):
        m = t.model_create(xyz, mat)
        assert m == n
        if e:
            t.model_set_scale(m, e)
        n_faces = int(LT.model_lights(t, m)["n"][0]) if lit else 0
        models[m] = dict(lo=xyz.min(axis=0), hi=xyz.max(axis=0) + 1, e=e, live=True, n_faces=n_faces)
        ids.append(m)
    t.model_destroy(4)
    models[4]["live"] = False
    assert [models[m]["n_faces"] for m in range(4)] == [54, 7 * 4 + 2, 54, 0]
    return models


def _table(n, rng):
    """n records over the store's models, with unusable ones in between: a model id out of range, the destroyed model, flip 8, a box that
    leaves the lattice, the model without a table."""
    t = np.zeros(n, dtype=INSTANCE)
    for i in range(n):
        axis, flip = IO.SIGNED_PERMUTATIONS[int(rng.integers(48))]
        t[i] = IO.instance(int(rng.integers(0, 4)), rng.integers(-2000, 2000, 3), axis, flip)
        kind = i % 7
        if kind == 2:
            t["model"][i] = 5 + int(rng.integers(0, 3)) * 1000
        elif kind == 3:
            t["model"][i] = 4
        elif kind == 4:
            t["flip"][i] = 8
        elif kind == 5:
            t["offset"][i] = (40000, 0, 0)
    return t


@pytest.mark.parametrize("a_world", [False, True], ids=["no world table", "a world table"])
def test_instance_lights_info_equals_the_numpy_rule(torch_cuda, a_world):
    t = tracer(a_world_plate=a_world)
    world_faces = 16 if a_world else 0
    models = _store(t)
    rng = np.random.default_rng(5)
    for n in (0, 1, 63, 64, 65, 300):
        table = _table(n, rng)
        want_icum, want = MR.prefix(table, models, a_world=world_faces)
        header, icum = LT.instance_lights_info(t, table)
        print(f"{n} instances: A_inst {want['a_inst']}, {want['n_lit']} lit")
        assert icum.tobytes() == want_icum.tobytes()
        assert {k: header[k][0].item() for k in ("a_inst", "a_total", "n_lit", "disabled")} == {k: want[k] for k in ("a_inst", "a_total", "n_lit", "disabled")}
        assert header["area_world"][0] == want["area_world"] and int(header["reserved"][0]) == 0
        assert n < 63 or 0 < want["n_lit"] < n
    with pytest.raises(BlokError) as e:
        t._check(t._lib.blok_hip_instance_lights_info(t._ctx, None, 3, None, None))
    assert e.value.status == BLOK_ERR_INVALID_ARG
    t.shutdown()


def test_the_overflow_pair_disables_instance_lights_and_nothing_fails(torch_cuda):
    t = tracer()
    lantern = t.model_create(MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32))
    t.model_set_scale(lantern, 8)
    assert int(LT.model_lights(t, lantern)["n"][0]) == 54
    models = {lantern: dict(lo=(0, 0, 0), hi=(3, 3, 3), e=8, live=True, n_faces=54)}
    for n, disabled in ((1213, 0), (1214, 1)):
        table = np.zeros(n, dtype=INSTANCE)
        table["model"], table["axis"] = lantern, (0, 1, 2)
        want_icum, want = MR.prefix(table, models)
        assert want["disabled"] == disabled
        header, icum = LT.instance_lights_info(t, table)
        assert icum.tobytes() == want_icum.tobytes()
        assert (int(header["disabled"][0]), int(header["a_inst"][0]), int(header["a_total"][0]), int(header["n_lit"][0])) == \
               (disabled, want["a_inst"], want["a_total"], want["n_lit"])
        assert header["area_world"][0] == want["area_world"]
    t.shutdown()
