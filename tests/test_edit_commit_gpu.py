"""GPU: the filling edits whose way to the shadow rays' last-occluder map had no test — a whole-box upload over an installed world, an
upload of zeros, edit_by_distance that grows, edit_by_flood that fills — and a clearing edit behind a filling one that changed nothing.
Each edit is recorded by gpu_volume_commit (gpu_build.h) and reaches the map through blok_hip_volume_rebuild; the check is the one of
tests/test_bricks_gpu.py::test_restore_that_adds_tall_geometry_keeps_the_sun_map_valid: every path-traced plane is bit-identical with the
map on and off, and where the edit adds tall geometry the image changes (the tower casts a shadow both cameras see).  Both layouts."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import world as W
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
W_PX, H_PX = 160, 120
SHAPE = (64, 96, 64)
_world = {}


def world():
    """The scene in the box's arrays ([z][y][x]), the same with a 6 x 5 tower above its highest voxel, and that voxel's height: computed
    once, never changed."""
    if not _world:
        ids = W.scene_dense(64, SEED)
        m = np.zeros((SHAPE[2], SHAPE[1], SHAPE[0]), np.uint32)
        m[:, :64, :] = ids
        d = (m > 0).astype(np.float32)
        top = int(np.nonzero(ids)[1].max())
        dt, mt = d.copy(), m.copy()
        dt[30:35, top + 1:min(top + 30, 95), 28:34] = 1.0
        mt[30:35, top + 1:min(top + 30, 95), 28:34] = 7
        assert int((dt > d).sum()) > 100
        for a in (d, m, dt, mt):
            a.setflags(write=False)
        _world.update(plain=(d, m), tower=(dt, mt), top=top)
    return _world


class Scene:
    """One context with the 64 x 96 x 64 volume at the origin in the given layout, and the check of every plane under two cameras."""

    def __init__(self, keyed):
        from blok_amd.tracer import HipTracer
        self.mats = W.scene_materials(SEED)
        self.t = HipTracer(W_PX, H_PX).init()
        self.t.set_volume_layout(keyed)
        self.t.volume_create((0, 0, 0), SHAPE, 128, 1.0)
        self.cams = [W.scene_camera(64, 0, W_PX, H_PX, SEED), W.camera_look_at((5.0, 30.0, 5.0), (40.0, 12.0, 40.0), 70.0, W_PX, H_PX)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.t.shutdown()

    def rebuild(self):
        return self.t.volume_rebuild(self.mats)

    def same(self, tag):
        """Every returned plane is bit-identical with the shadow rays' map off and on; returns the colour planes."""
        planes = []
        for cam in self.cams:
            self.t.set_sun_map(False)
            plain = self.t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            self.t.set_sun_map(True)
            got = self.t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            for k in plain:
                assert got[k].tobytes() == plain[k].tobytes(), (tag, k)
            planes.append(plain["color"].tobytes())
        return planes


@LAYOUTS
def test_upload_of_taller_geometry_over_an_uploaded_world(keyed):
    """upload(A), rebuild, upload(B) with a tower, rebuild: the lattice stays, so the map is kept — and has to learn of the tower."""
    w = world()
    with Scene(keyed) as s:
        s.t.volume_upload(*w["plain"])
        s.rebuild()
        first = s.same("scene")
        s.t.volume_upload(*w["tower"])
        s.rebuild()
        assert s.same("scene with tower") != first


@LAYOUTS
def test_upload_of_zeros_over_a_world_and_the_world_again(keyed):
    w = world()
    with Scene(keyed) as s:
        s.t.volume_upload(*w["tower"])
        s.rebuild()
        first = s.same("scene with tower")
        s.t.volume_upload(None, None)
        assert s.rebuild().n_voxels == 0
        assert s.same("sky") != first                                # (nothing left to hit)
        s.t.volume_upload(*w["tower"])
        assert s.rebuild().n_voxels == int((w["tower"][0] > 0).sum())
        assert s.same("scene with tower again") == first


@LAYOUTS
def test_edit_by_distance_that_grows_the_tower(keyed):
    w = world()
    top = w["top"]
    with Scene(keyed) as s:
        s.t.volume_upload(*w["tower"])
        s.rebuild()
        thin = s.same("scene with tower")
        s.t.volume_distance_field((22, top - 4, 24), (40, 96, 41), max_radius=4)
        assert s.t.volume_edit_by_distance(_ffi.DISTANCE_GROW, 9, 1.0, 7) > 1000      # three voxels on every side of the tower
        s.rebuild()
        assert s.same("tower grown") != thin


@LAYOUTS
def test_edit_by_flood_that_fills_the_tower(keyed):
    w = world()
    top = w["top"]
    lo, hi = (28, top + 1, 30), (34, min(top + 30, 95), 35)          # the tower's site: empty in the plain scene
    with Scene(keyed) as s:
        s.t.volume_upload(*w["plain"])
        s.rebuild()
        first = s.same("scene")
        s.t.volume_flood_field(lo, hi, seeds=[lo], max_steps=64)
        assert s.t.volume_edit_by_flood(_ffi.FLOOD_FILL, 64, 1.0, 7) == 6 * 5 * (hi[1] - lo[1])
        s.rebuild()
        assert s.same("site filled") != first
        d, m = s.t.volume_download()
        assert d.tobytes() == w["tower"][0].tobytes() and m.tobytes() == w["tower"][1].tobytes()


# What blok_hip_volume_refresh_counts advances by over the two brushes below (keyed edit path, keyed upload path, general layout): read
# once from a library built of the commit before gpu_volume_commit existed, running this test: (1, 0, 0) -> (3, 0, 0) keyed and
# (0, 0, 1) -> (0, 0, 3) general — one refresh per brush, on the edit's path of its layout.
BRUSH_PAIR_REFRESHES = {True: (2, 0, 0), False: (0, 0, 2)}


@LAYOUTS
def test_a_dig_behind_an_add_brush_that_changed_nothing(keyed):
    """An ADD brush of radius 0 on a filled voxel fills nothing; the SUBTRACT brush behind it digs the tower away.  The pair is recorded
    as one box that may have been filled: valid, and no more refreshes than before."""
    w = world()
    top = w["top"]
    z, y, x = (int(v) for v in np.argwhere(w["plain"][0] > 0)[0])           # a filled voxel
    with Scene(keyed) as s:
        s.t.volume_upload(*w["tower"])
        s.rebuild()
        first = s.same("scene with tower")
        before = s.t.volume_refresh_counts()
        s.t.volume_apply_brush((x + 0.5, y + 0.5, z + 0.5), 0.0, 1.0, 0)
        s.t.volume_apply_brush((31.0, top + 14.0, 32.5), 16.0, 0.0, 1)
        after = s.t.volume_refresh_counts()
        print(f"refresh counts {before} -> {after}")
        assert tuple(a - b for a, b in zip(after, before)) == BRUSH_PAIR_REFRESHES[keyed]
        s.rebuild()
        assert s.same("dug") != first
