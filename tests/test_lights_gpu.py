"""GPU: the light table on the device (include/blok_hip.h, "emissive voxels as lights": blok_hip_lights_from_quads, blok_hip_set_lights,
blok_hip_lights_info, blok_hip_lights_download) against the host build (blok_lights_from_quads) over tests/lights_cases.py, byte for byte
and in both brick layouts; the table's life and the errors, each of which leaves the installed table in place."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import world as W
from blok_amd._ffi import LIGHT, BlokError
from tests import lights_cases as LC

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
CASES = LC.table()


def _tracer():
    from blok_amd.tracer import HipTracer
    return HipTracer(32, 32).init()


def _install(t, case):
    t.volume_create(case.origin, case.shape)
    t.volume_upload(case.density, case.ids)
    t.volume_rebuild(case.materials)


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
def test_from_quads_equals_the_host_build_over_the_case_table(keyed):
    t = _tracer()
    t.set_volume_layout(keyed)
    for case in CASES:
        _install(t, case)
        assert int(LT.info(t)["n"][0]) == 0, "a rebuild clears the table"
        quads = t.volume_extract_quads()
        assert quads.tobytes() == LC.quads_of(case).tobytes()
        want, want_info = LT.host_from_quads(quads, case.materials, 1.0)
        info = LT.from_quads(t)
        got = LT.download(t)
        print(f"{case.name}: {len(quads)} quads -> device {int(info['n'][0])} lights / {int(info['n_faces'][0])} faces, host {len(want)} / {int(want_info['n_faces'][0])}")
        assert got.tobytes() == want.tobytes()
        for k in ("n", "n_faces", "n_owned", "area_world"):
            assert info[k][0] == want_info[k][0], k
        assert int(info["bytes"][0]) == (32 * len(want) + 8192 if len(want) else 0)
        assert LT.info(t).tobytes() == info.tobytes()
        # in pieces
        n = len(want)
        if n > 2:
            cut = n // 3
            parts = [LT.download(t, 0, cut), LT.download(t, cut, 1), LT.download(t, cut + 1, n - cut - 1, page=5), LT.download(t, n, 0)]
            assert np.concatenate(parts).tobytes() == want.tobytes()
        with pytest.raises(BlokError) as e:
            LT.download(t, n, 1)
        assert e.value.status == BLOK_ERR_INVALID_ARG
    t.shutdown()


def test_errors_leave_the_installed_table_and_a_new_world_clears_it():
    t = _tracer()
    with pytest.raises(BlokError) as e:
        LT.from_quads(t)
    assert e.value.status == BLOK_ERR_NO_WORLD
    plate = CASES[4]
    _install(t, plate)
    with pytest.raises(BlokError) as e:                     # a world, but no quads snapshot yet
        LT.from_quads(t)
    assert e.value.status == BLOK_ERR_INVALID_ARG and "snapshot" in str(e.value)
    t.volume_extract_quads()
    first = LT.from_quads(t)
    table = LT.download(t)
    assert int(first["n"][0]) == plate.n_lights and int(first["n_faces"][0]) == plate.n_faces and int(first["n_owned"][0]) == 2

    def unchanged():
        assert LT.info(t).tobytes() == first.tobytes() and LT.download(t).tobytes() == table.tobytes()

    with pytest.raises(BlokError) as e:                     # unknown flag bits
        t._check(t._lib.blok_hip_lights_from_quads(t._ctx, 1, None))
    assert e.value.status == BLOK_ERR_INVALID_ARG
    unchanged()
    t.volume_extract_quads(ignore_material=True)            # the keys of this snapshot are no material ids
    with pytest.raises(BlokError) as e:
        LT.from_quads(t)
    assert e.value.status == BLOK_ERR_INVALID_ARG and "IGNORE_MATERIAL" in str(e.value)
    unchanged()
    t.volume_extract_quads(count_only=True)                  # keeps nothing: the ignoring snapshot is still the context's
    with pytest.raises(BlokError):
        LT.from_quads(t)
    unchanged()
    # set_lights: each rule refuses and leaves the table
    for field, value, status in (("face", 6, BLOK_ERR_INVALID_ARG), ("du", 0, BLOK_ERR_INVALID_ARG), ("cum", 3, BLOK_ERR_INVALID_ARG)):
        bad = table.copy()
        bad[field][1] = value
        with pytest.raises(BlokError) as e:
            LT.set(t, bad)
        assert e.value.status == status and "light 1" in str(e.value)
        unchanged()
    bad = table[:1].copy()
    bad["lo"][0] = (0, 40000, 0)
    with pytest.raises(BlokError) as e:
        LT.set(t, bad)
    assert e.value.status == BLOK_ERR_INVALID_ARG
    forged = np.zeros(1, dtype=LIGHT)
    forged["lo"], forged["du"], forged["dv"], forged["face"] = (-32768, -32768, -32768), 65536, 65536, 4
    with pytest.raises(BlokError) as e:
        LT.set(t, forged)
    assert e.value.status == BLOK_ERR_UNSUPPORTED
    unchanged()
    # edits, a new extraction and a scroll leave it alone
    t.volume_set_voxels(np.array([[0, 5, 0]], dtype=np.int32), np.array([LC.GLOW_B], dtype=np.uint32), np.array([1.0], dtype=np.float32))
    t.volume_extract_quads()
    unchanged()
    # a host table installed, read back, cleared
    half = table[:7].copy()
    info = LT.set(t, half)
    assert int(info["n"][0]) == 7 and int(info["n_faces"][0]) == int((half["du"].astype(np.int64) * half["dv"]).sum())
    assert info["area_world"][0] == np.float32(int(info["n_faces"][0]))
    assert LT.download(t).tobytes() == half.tobytes()
    LT.clear(t)
    assert int(LT.info(t)["n"][0]) == 0 and int(LT.info(t)["bytes"][0]) == 0 and len(LT.download(t)) == 0
    # from_quads that keeps nothing installs the empty table
    LT.set(t, half)
    t.volume_rebuild(LC.materials()[:3])                     # no emissive material left; the rebuild has cleared the table already
    assert int(LT.info(t)["n"][0]) == 0
    LT.set(t, half)
    t.volume_extract_quads()
    assert int(LT.from_quads(t)["n"][0]) == 0 and int(LT.info(t)["n"][0]) == 0
    # no material table
    t.volume_rebuild(None)
    with pytest.raises(BlokError) as e:
        LT.from_quads(t)
    assert e.value.status == BLOK_ERR_INVALID_ARG and "material" in str(e.value)
    # another world through upload_world clears as well
    t.volume_rebuild(plate.materials)
    t.volume_extract_quads()
    assert int(LT.from_quads(t)["n"][0]) > 0
    cm = W.ChunkManager(128, 1.0)
    cm.set_voxels(np.array([[1, 1, 1], [2, 1, 1]], dtype=np.int32), np.array([1, 3], dtype=np.uint32))
    cm.rebuild_dirty_chunks()
    t.add_world(cm.pack_chunks_to_gpu_svo(plate.materials))
    assert int(LT.info(t)["n"][0]) == 0
    # a world that is not a volume: host quads, host build, set_lights
    lights = np.zeros(1, dtype=LIGHT)
    lights["lo"], lights["du"], lights["dv"], lights["material"], lights["face"] = (2, 2, 1), 1, 1, 3, 2
    assert int(LT.set(t, lights)["n_owned"][0]) == 1
    t.shutdown()
