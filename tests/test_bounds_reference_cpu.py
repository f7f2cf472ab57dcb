"""CPU: tests/bounds_reference.py — what the GPU modules hold the beam pre-pass and the shadow rays' map against — pinned to something
independent: the oracle's tracer (no shadow ray's any-hit answer changes under the reference's lower map, no primary hit lies before the
reference's lower start parameter) and brute force over every voxel, texel, tile and corner."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import world as W
from tests import bounds_reference as B
from tests import oracle_ffi as O
from tests.conftest import SEED


def packed(xyz, mats):
    cm = W.ChunkManager(128, 1.0)
    cm.set_voxels(np.asarray(xyz, dtype=np.int32), np.asarray(mats, dtype=np.uint32))
    cm.rebuild_dirty_chunks()
    return cm.pack_chunks_to_gpu_svo(W.scene_materials(SEED))


def random_volume(n=24, seed=5, fill=0.08, origin=(-7, 3, -20)):
    rng = np.random.default_rng(seed)
    return B.voxels_of(rng.random((n, n, n)) < fill, origin)


def shadow_rays(voxels, info, count, seed):
    """Origins just off filled faces — a hair along the face normal, as the shader starts its shadow rays, on either side of the face, as
    float32 hit points land — and in free space, along s.  (Only an origin inside a voxel can be cut short by a map that is less than
    0.3 too low: a ray that enters a voxel from outside does so at least min(s) = 0.3 before the voxel's farthest corner.)"""
    rng = np.random.default_rng(seed)
    v = voxels[rng.integers(0, len(voxels), size=count // 2)].astype(np.float64)
    face = rng.integers(0, 6, size=len(v))
    on = v + 1.0 - rng.random((len(v), 3)) ** 3                          # anywhere on the face, more of them towards the voxel's farthest corner
    axis, high = face // 2, face % 2
    on[np.arange(len(v)), axis] = v[np.arange(len(v)), axis] + high + np.where(rng.random(len(v)) < 0.5, 1.0e-3, -1.0e-3)
    lo, hi = voxels.min(axis=0) - 6.0, voxels.max(axis=0) + 7.0
    free = rng.uniform(lo, hi, size=(count - len(v), 3))
    rays = np.zeros(count, dtype=O.RAY)
    rays["org"] = np.concatenate([on, free]).astype(np.float32)
    rays["dir"] = np.asarray(info["s"], dtype=np.float32)
    rays["tmin"], rays["tmax"] = 0.001, 1000.0
    return rays


@pytest.mark.parametrize("scene", ["random 24", "scene 64"])
def test_sun_reference_caps_no_shadow_ray_wrongly(scene):
    """A shadow ray's any-hit answer is the same with tmax capped at the reference's LOWER map exactly as path_core.h caps it; with that
    map lowered by 0.2 in every texel at least one answer changes (the check bites)."""
    if scene == "random 24":
        voxels = random_volume()
    else:
        voxels = B.voxels_of(W.scene_dense(64, SEED) != 0, (0, 0, 0))
    pw = packed(voxels, np.ones(len(voxels), np.uint32))
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    origin, edge = B.cube_of(voxels)
    info = B.sun_frame(origin, edge)
    lo, hi = B.sun_map_bounds(voxels, info, B.sun_delta(info, origin, edge))
    assert (lo <= hi).all() and (lo > -B.K_BEAM_NONE).sum() > len(voxels) ** (2.0 / 3.0)
    rays = shadow_rays(voxels, info, 8000, 17)
    plain, ctr = lat.trace(rays, threads=8)
    assert 500 < ctr["hits"] < len(rays) - 500

    def capped(texels):
        tmax, empty = B.sun_capped_tmax(info, texels, rays["org"], 0.001, 1000.0)
        r = rays.copy()
        r["tmax"] = tmax
        got, _ = lat.trace(r, threads=8)
        return np.where(empty, 0, got["hit"])
    assert (capped(lo.astype(np.float32)) == plain["hit"]).all()
    lowered = np.where(lo > -B.K_BEAM_NONE, lo - 0.2, lo).astype(np.float32)
    changed = int((capped(lowered) != plain["hit"]).sum())
    print(f"{scene}: {int(ctr['hits'])} of {len(rays)} shadow rays hit; {changed} answers change under the map lowered by 0.2")
    assert changed >= 1


def corner_rays(cam, w, h, rects, like):
    """Rays through the four corners, the four edge midpoints and the centre of every tile's pixel rectangle (continuous pixel
    coordinates), nine per tile."""
    pts = np.array([(x, y) for px, py, px_end, py_end in rects for x in (px, 0.5 * (px + px_end), px_end) for y in (py, 0.5 * (py + py_end), py_end)], dtype=np.float64)
    _, fwd, right, up, t, a = B.camera_vectors(cam)
    u = (2.0 * pts[:, 0] / w - 1.0) * t * a
    v = (1.0 - 2.0 * pts[:, 1] / h) * t
    d = fwd + right * u[:, None] + up * v[:, None]
    rays = np.zeros(len(pts), dtype=O.RAY)
    rays["dir"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["org"], rays["tmin"], rays["tmax"] = like["org"], like["tmin"], like["tmax"]
    return rays


def test_beam_reference_lies_below_every_primary_hit():
    """40 random cameras over the odd world, frame 161 x 93, tiles of 8 and 32: every oracle primary hit's t in a tile is >= the tile's
    t0_lo, through the pixel centres and through the corners and edges of the tile's pixel rectangle; a tile whose t0_lo says "none" has
    no hit."""
    xyz, mats = B.odd_world_voxels()
    voxels = np.unique(xyz.astype(np.int64), axis=0)
    pw = packed(xyz, mats)
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    w, h = 161, 93
    origin, edge = B.cube_of(voxels)
    n_hits = n_none = 0
    least = np.inf
    for k, (eye, target, fov) in enumerate(B.random_cameras(40, w, h, 99)):
        cam = W.camera_look_at(eye, target, fov, w, h)
        rays = O.primary_rays(cam, w, h)
        hits, _ = lat.trace(rays, threads=8)
        t = np.where(hits["hit"] == 1, hits["t"].astype(np.float64), np.inf).reshape(h, w)
        for tile in (8, 32):
            lo, hi, eps = B.beam_tile_bounds(voxels, cam, w, h, (0, 0, w, h), tile, 1.0, B.beam_delta(cam, 1.0, origin, edge))
            assert (lo <= hi).all()
            rects = B.tile_rects((0, 0, w, h), tile)
            extra = corner_rays(cam, w, h, rects, rays[0])
            ehits, _ = lat.trace(extra, threads=8)
            et = np.where(ehits["hit"] == 1, ehits["t"].astype(np.float64), np.inf).reshape(len(rects), -1)
            for i, (px, py, px_end, py_end) in enumerate(rects):
                first = min(t[py:py_end, px:px_end].min(), et[i].min())
                if lo[i] >= B.K_BEAM_NONE:
                    n_none += 1
                    assert first == np.inf, (k, tile, i)
                elif first < np.inf:
                    n_hits += 1
                    least = min(least, first - lo[i])
                    assert first >= lo[i], (k, tile, i, first, lo[i])
    print(f"{n_hits} tiles with hits, {n_none} tiles without a voxel; least t - t0_lo = {least:.4f}")
    assert n_hits > 2000 and n_none > 2000


def test_vectorised_references_equal_brute_force():
    """8^3 volume: inner / outer of the sun map against a loop over every voxel, texel and corner; the same for the beam's tiles."""
    voxels = random_volume(8, 3, 0.15, (-3, 2, -5))
    assert len(voxels) > 40
    origin, edge = B.cube_of(voxels)
    info = B.sun_frame(origin, edge)
    for delta in (B.sun_delta(info, origin, edge), 0.01):
        lo, hi = B.sun_map_bounds(voxels, info, delta)
        blo, bhi = B.sun_map_bounds_brute(voxels, info, delta)
        assert np.array_equal(lo, blo) and np.array_equal(hi, bhi)
    assert (lo != hi).any()                                           # (at delta 0.01 the two sets differ somewhere)
    w, h = 45, 27
    for eye, target, fov in (((30.0, 20.0, -30.0), (0.0, 6.0, -1.0), 50.0), ((1.3, 6.2, -1.1), (9.0, 7.0, 5.0), 120.0), ((0.0, 40.0, 0.0), (0.5, 0.0, -1.5), 8.0)):
        cam = W.camera_look_at(eye, target, fov, w, h)
        for tile, rect in ((8, (0, 0, w, h)), (16, (5, 3, 33, 20))):
            for delta0 in (B.beam_delta(cam, 1.0, origin, edge), 0.01):
                lo, hi, _ = B.beam_tile_bounds(voxels, cam, w, h, rect, tile, 1.0, delta0)
                blo, bhi = B.beam_tile_bounds_brute(voxels, cam, w, h, rect, tile, 1.0, delta0)
                assert np.allclose(lo, blo, rtol=0, atol=1e-9) and np.allclose(hi, bhi, rtol=0, atol=1e-9)
