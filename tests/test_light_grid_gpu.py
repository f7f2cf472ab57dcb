"""GPU: the light grid on the device (include/blok_hip.h, "the light grid": blok_hip_build_light_grid, blok_hip_light_grid_info,
blok_hip_light_grid_download, blok_hip_light_grid_clear) against the host build (blok_light_grid_build) byte for byte in all three
arrays, over tests/light_grid_cases.py through set_lights and over a table from lights_from_quads; the piecewise downloads; the errors,
each of which leaves the installed grid; what drops the grid and what keeps it."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import lights as LT
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import light_grid_cases as GC
from tests import lights_cases as LC

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
CASES = GC.table()
START, FACES, ITEMS = _ffi.LIGHT_GRID_START, _ffi.LIGHT_GRID_FACES, _ffi.LIGHT_GRID_ITEMS


def _tracer(case=None):
    """A tracer with a small volume as its world (set_lights wants one)."""
    from blok_amd.tracer import HipTracer
    t = HipTracer(32, 32).init()
    case = case or LC.table()[1]
    t.volume_create(case.origin, case.shape)
    t.volume_upload(case.density, case.ids)
    t.volume_rebuild(case.materials)
    return t


def _grid(t):
    return LT.grid_download(t, START), LT.grid_download(t, FACES), LT.grid_download(t, ITEMS)


def _same(t, lights, c, reach, share, info):
    start, faces, items, want = LT.host_build_grid(lights, c, reach, share)
    got = _grid(t)
    assert got[0].tobytes() == start.tobytes(), "start"
    assert got[1].tobytes() == faces.tobytes(), "faces"
    assert got[2].tobytes() == items.tobytes(), "items"
    assert info.tobytes() == want.tobytes() and LT.grid_info(t).tobytes() == want.tobytes()
    return want


def test_device_grid_equals_the_host_build_over_the_case_table():
    t = _tracer()
    for case in CASES:
        LT.set(t, case.lights)
        assert int(LT.grid_info(t)["n_cells"][0]) == 0, "set_lights drops the grid"
        for n, (c, reach) in enumerate(case.params):
            share = (1, 192, 255)[n % 3]
            info = LT.build_grid(t, c, reach, share)
            want = _same(t, case.lights, c, reach, share, info)
            print(f"{case.name}: c {c} R {reach}: {int(want['n_cells'][0])} cells, {int(want['n_items'][0])} items, longest {int(want['max_items'][0])}")
    t.shutdown()


@pytest.mark.parametrize("which", [4, 8], ids=["plate", "above 4096 lights"])
def test_grid_over_a_table_from_quads_and_the_piecewise_downloads(which):
    """The second volume gives more than 4096 lights and more than 10^5 items: many workgroups in every pass, and the sort's path for
    large inputs."""
    case = LC.table()[which]
    t = _tracer(case)
    t.volume_extract_quads()
    n_lights = int(LT.from_quads(t)["n"][0])
    assert n_lights == case.n_lights if case.n_lights is not None else n_lights > 4096
    table = LT.download(t)
    info = LT.build_grid(t, 2, 1, 128)
    want = _same(t, table, 2, 1, 128, info)
    n_cells, n_items = int(want["n_cells"][0]), int(want["n_items"][0])
    print(f"{case.name}: {n_lights} lights -> {n_cells} cells, {n_items} items, longest {int(want['max_items'][0])}")
    assert n_cells > 256 and n_items > n_cells and (which != 4 or int(want["n_nonempty"][0]) < n_cells) and (which != 8 or n_items > 100000)
    whole = _grid(t)
    for what, n in ((START, n_cells + 1), (FACES, n_cells), (ITEMS, n_items)):
        cut = n // 3
        parts = [LT.grid_download(t, what, 0, cut), LT.grid_download(t, what, cut, 1), LT.grid_download(t, what, cut + 1, n - cut - 1, page=7), LT.grid_download(t, what, n, 0)]
        assert np.concatenate(parts).tobytes() == whole[what].tobytes()
        with pytest.raises(BlokError) as e:
            LT.grid_download(t, what, n, 1)
        assert e.value.status == BLOK_ERR_INVALID_ARG
    with pytest.raises(BlokError) as e:
        LT.grid_download(t, 3, 0, 0)
    assert e.value.status == BLOK_ERR_INVALID_ARG
    t.shutdown()


def test_a_grid_of_exactly_2_to_the_24_cells_is_built():
    """The cap itself passes (one layer of cells more is refused: below): two lights in opposite corners of 256^3 cells."""
    name, lights, c, reach, passes = GC.limit_cases()[0]
    assert passes
    t = _tracer()
    LT.set(t, lights)
    info = LT.build_grid(t, c, reach, 128)
    assert int(info["n_cells"][0]) == 2 ** 24 and int(info["n_items"][0]) == 2 and int(info["n_nonempty"][0]) == 2 and int(info["max_items"][0]) == 1
    _same(t, lights, c, reach, 128, info)
    t.shutdown()


def test_every_error_leaves_the_installed_grid():
    t = _tracer()
    with pytest.raises(BlokError) as e:                     # no light table
        LT.build_grid(t, 4, 1, 128)
    assert e.value.status == BLOK_ERR_INVALID_ARG and "light table" in str(e.value)
    with pytest.raises(BlokError):                          # ... and no grid to download
        LT.grid_download(t, START, 0, 0)
    # tables that fit at c = 6 and cross a limit at c = 2
    for name, lights, c, reach, passes in GC.limit_cases()[1::2]:
        LT.set(t, lights)
        first = LT.build_grid(t, 6, 0, 200)
        kept = _grid(t)

        def unchanged():
            assert LT.grid_info(t).tobytes() == first.tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(_grid(t), kept))

        with pytest.raises(BlokError) as e:
            LT.build_grid(t, c, reach, 128)
        assert e.value.status == BLOK_ERR_UNSUPPORTED, name
        unchanged()
        for args in ((1, 0, 128), (13, 0, 128), (4, 4, 128), (4, 1, 0), (4, 1, 256)):
            with pytest.raises(BlokError) as e:
                LT.build_grid(t, *args)
            assert e.value.status == BLOK_ERR_INVALID_ARG
        with pytest.raises(BlokError) as e:                 # unknown flag bits
            t._check(t._lib.blok_hip_build_light_grid(t._ctx, 4, 1, 128, 1, None))
        assert e.value.status == BLOK_ERR_INVALID_ARG
        unchanged()
    t.shutdown()


def test_what_drops_the_grid_and_what_keeps_it():
    plate = LC.table()[4]
    t = _tracer(plate)
    t.volume_extract_quads()
    LT.from_quads(t)
    table = LT.download(t)

    def build():
        assert int(LT.build_grid(t, 3, 1, 192)["n_cells"][0]) > 0
        return LT.grid_info(t), _grid(t)

    def gone():
        assert LT.grid_info(t).tobytes() == np.zeros(1, dtype=_ffi.LIGHT_GRID_INFO).tobytes()
        with pytest.raises(BlokError):
            LT.grid_download(t, FACES, 0, 0)

    # kept: an edit, a new extraction, a scroll
    info, kept = build()
    t.volume_set_voxels(np.array([[0, 5, 0]], dtype=np.int32), np.array([LC.GLOW_B], dtype=np.uint32), np.array([1.0], dtype=np.float32))
    t.volume_extract_quads()
    t.volume_scroll((4, 0, 0))
    assert LT.grid_info(t).tobytes() == info.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(_grid(t), kept))
    assert LT.download(t).tobytes() == table.tobytes()
    # dropped: its own clear, set_lights, lights_from_quads, clearing the table, a new world
    LT.clear_grid(t)
    gone()
    assert LT.download(t).tobytes() == table.tobytes(), "clearing the grid leaves the table"
    build()
    LT.set(t, table[:5])
    gone()
    build()
    LT.from_quads(t)
    gone()
    build()
    LT.clear(t)
    gone()
    LT.set(t, table)
    build()
    t.volume_rebuild(plate.materials)
    gone()
    # ... and a world that is not the volume, through upload_world
    t.volume_extract_quads()
    LT.from_quads(t)
    build()
    cm = W.ChunkManager(128, 1.0)
    cm.set_voxels(np.array([[1, 1, 1], [2, 1, 1]], dtype=np.int32), np.array([1, 3], dtype=np.uint32))
    cm.rebuild_dirty_chunks()
    t.add_world(cm.pack_chunks_to_gpu_svo(plate.materials))
    gone()
    assert int(LT.info(t)["n"][0]) == 0
    t.shutdown()
