"""A plain model of stamping a placed model into a voxel volume and of capturing a region as a voxel list — TESTS ONLY, numpy alone,
written from the contract in include/blok_hip.h (blok_hip_volume_stamp_models, blok_hip_volume_capture_model), not from the product's
shared header.

Placement (axis, flip, offset): a filled model voxel v' lands on the world voxel w with, for each local axis k,
    w[axis[k]] = offset[axis[k]] + v'[k]          if flip bit k is clear,
    w[axis[k]] = offset[axis[k]] - 1 - v'[k]      if it is set.
Arrays are [z][y][x] over a box whose voxel (0, 0, 0) sits at world `origin`; a voxel is filled iff density > 0."""
from __future__ import annotations

import itertools

import numpy as np

SET, KEEP, ERASE = 0, 1, 2

# the 48 orientations: every permutation of the axes with every combination of flips
ORIENTATIONS = [(axis, flip) for axis in itertools.permutations((0, 1, 2)) for flip in range(8)]
assert len(ORIENTATIONS) == 48


def world_voxels(model_xyz, offset, axis, flip) -> np.ndarray:
    """(n, 3) int64 world voxels of the (n, 3) local voxels."""
    v = np.asarray(model_xyz, dtype=np.int64).reshape(-1, 3)
    w = np.zeros_like(v)
    for k in range(3):
        a = int(axis[k])
        w[:, a] = (int(offset[a]) - 1 - v[:, k]) if (int(flip) >> k) & 1 else (int(offset[a]) + v[:, k])
    return w


def last_wins(model_xyz, model_mats):
    """The voxel list with duplicates removed, keeping the last entry of every voxel (model_create's rule)."""
    v = np.asarray(model_xyz, dtype=np.int64).reshape(-1, 3)
    m = np.asarray(model_mats, dtype=np.uint32).reshape(-1)
    seen, keep = set(), []
    for i in range(len(v) - 1, -1, -1):
        key = tuple(v[i])
        if key not in seen:
            seen.add(key)
            keep.append(i)
    keep = np.array(sorted(keep), dtype=np.int64)
    return v[keep], m[keep]


def stamp(density, ids, origin, model_xyz, model_mats, placement, mode, value) -> int:
    """Stamps in place; placement = (offset, axis, flip).  Returns the number of voxels written."""
    offset, axis, flip = placement
    v, m = last_wins(model_xyz, model_mats)
    w = world_voxels(v, offset, axis, flip) - np.asarray(origin, dtype=np.int64)
    nz, ny, nx = density.shape
    inside = (w >= 0).all(axis=1) & (w[:, 0] < nx) & (w[:, 1] < ny) & (w[:, 2] < nz)
    w, m = w[inside], m[inside]
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    if mode == ERASE:
        density[z, y, x] = np.float32(0.0)
        ids[z, y, x] = 0
        return len(w)
    if mode == KEEP:
        empty = ~(density[z, y, x] > 0)                       # 0, negative and NaN are empty
        x, y, z, m = x[empty], y[empty], z[empty], m[empty]
    else:
        assert mode == SET
    density[z, y, x] = np.float32(value)
    ids[z, y, x] = m
    return len(x)


def clipped(model_xyz, origin, shape_zyx, placement) -> int:
    """How many of the model's (distinct) voxels land outside the box."""
    offset, axis, flip = placement
    v = np.unique(np.asarray(model_xyz, dtype=np.int64).reshape(-1, 3), axis=0)
    w = world_voxels(v, offset, axis, flip) - np.asarray(origin, dtype=np.int64)
    nz, ny, nx = shape_zyx
    inside = (w >= 0).all(axis=1) & (w[:, 0] < nx) & (w[:, 1] < ny) & (w[:, 2] < nz)
    return int((~inside).sum())


def capture(density, ids, origin, lo=None, hi=None):
    """The filled voxels of the region [lo, hi) (world voxels; both None = the whole box) as (xyz (n, 3) int32 relative to the region's
    corner, material ids), x fastest, then y, then z."""
    nz, ny, nx = density.shape
    o = np.asarray(origin, dtype=np.int64)
    l = np.zeros(3, dtype=np.int64) if lo is None else np.asarray(lo, dtype=np.int64) - o
    h = np.array([nx, ny, nz], dtype=np.int64) if hi is None else np.asarray(hi, dtype=np.int64) - o
    assert (l >= 0).all() and (h <= [nx, ny, nz]).all() and (l <= h).all()
    d = density[l[2]:h[2], l[1]:h[1], l[0]:h[0]]
    z, y, x = np.nonzero(d > 0)                               # C order of [z][y][x]: x fastest
    xyz = np.stack([x, y, z], axis=1).astype(np.int32).reshape(-1, 3)
    return xyz, ids[l[2]:h[2], l[1]:h[1], l[0]:h[0]][z, y, x].astype(np.uint32)


def cut(density, ids, origin, lo=None, hi=None):
    """Clears the region's filled voxels in place (density 0, id 0)."""
    nz, ny, nx = density.shape
    o = np.asarray(origin, dtype=np.int64)
    l = np.zeros(3, dtype=np.int64) if lo is None else np.asarray(lo, dtype=np.int64) - o
    h = np.array([nx, ny, nz], dtype=np.int64) if hi is None else np.asarray(hi, dtype=np.int64) - o
    sl = (slice(l[2], h[2]), slice(l[1], h[1]), slice(l[0], h[0]))
    f = density[sl] > 0
    density[sl][f] = np.float32(0.0)
    ids[sl][f] = 0


# ---- the models and volumes the CPU and GPU tests share -----------------------------------------------------------------------------

def small_model():
    """5 x 7 x 3 with holes, a distinct material per voxel, local coordinates on both sides of zero ([-2, 3) x [-3, 4) x [-1, 2))."""
    xyz, mats = [], []
    for z in range(-1, 2):
        for y in range(-3, 4):
            for x in range(-2, 3):
                if (x * 3 + y * 5 + z * 7) % 4 == 0 and (x, y, z) not in ((-2, -3, -1), (2, 3, 1), (-2, 3, -1)):
                    continue                                   # holes (the box corners listed stay, so the box is 5 x 7 x 3)
                xyz.append((x, y, z))
                mats.append(1000 + len(mats))
    xyz, mats = np.array(xyz, dtype=np.int32), np.array(mats, dtype=np.uint32)
    assert tuple(xyz.min(axis=0)) == (-2, -3, -1) and tuple(xyz.max(axis=0)) == (2, 3, 1) and len(xyz) < 5 * 7 * 3
    return xyz, mats


def large_model():
    """70 x 9 x 21 over [-37, 33) x [-4, 5) x [-9, 12): several bricks and 16-cells, three tree levels, negative local coordinates, holes."""
    x, y, z = np.meshgrid(np.arange(-37, 33), np.arange(-4, 5), np.arange(-9, 12), indexing="ij")
    x, y, z = x.ravel(), y.ravel(), z.ravel()
    h = (x * 73856093) ^ (y * 19349663) ^ (z * 83492791)
    keep = ((h >> 3) % 5 != 0) | ((np.abs(x) == 37) | (x == 32))
    keep &= ~((x > -20) & (x < -10) & (z > -4) & (z < 6))      # a tunnel: whole bricks of the model's grid stay empty
    keep |= (x == -37) & (y == -4) & (z == -9)
    keep |= (x == 32) & (y == 4) & (z == 11)
    xyz = np.stack([x[keep], y[keep], z[keep]], axis=1).astype(np.int32)
    mats = (np.arange(len(xyz)) * 7 + 3).astype(np.uint32)
    assert tuple(xyz.min(axis=0)) == (-37, -4, -9) and tuple(xyz.max(axis=0)) == (32, 4, 11)
    return xyz, mats


# six orientations for the large model: every permutation class occurs, every axis is flipped in at least one
LARGE_ORIENTATIONS = [((0, 1, 2), 0), ((0, 2, 1), 1), ((1, 0, 2), 2), ((1, 2, 0), 4), ((2, 0, 1), 7), ((2, 1, 0), 5)]
assert {a for a, _ in LARGE_ORIENTATIONS} == set(itertools.permutations((0, 1, 2)))
assert all(any((f >> k) & 1 for _, f in LARGE_ORIENTATIONS) for k in range(3))
