"""A plain model of the resident volume and of the tree a rebuild must derive from it — TESTS ONLY, numpy alone (no product library).

The tree of a dense box is a pure function of the box (blok_amd/csrc/hip/tree.h): root first, every level in ascending key order, `base` =
index of the first child, bricks carry the offset of their first material id.  `reference_tree` restates the host builder
(tree_build.cpp: build_tree) in array form; tests/test_volume_tree_reference_cpu.py pins it to that builder byte for byte, and the
model's brush to the oracle's ChunkManager."""
from __future__ import annotations

import numpy as np


def box_levels(shape_xyz) -> int:
    """Levels of the tree over a box: the smallest L >= 1 with 4^L >= the largest extent."""
    levels = 1
    while 4 ** levels < max(int(v) for v in shape_xyz):
        levels += 1
    return levels


def reference_tree(filled: np.ndarray, ids: np.ndarray, levels: int):
    """filled, ids: [z][y][x] over the box, coordinates box-local from 0.  Returns (nodes (n, 4) uint32, materials uint32).
    Nothing filled: one all-zero node and no materials (a tree of one level, whatever `levels` says)."""
    filled = np.asarray(filled, dtype=bool)
    ids = np.asarray(ids, dtype=np.uint32)
    assert filled.shape == ids.shape and filled.ndim == 3
    z, y, x = (c.astype(np.uint64) for c in np.nonzero(filled))
    if len(x) == 0:
        return np.zeros((1, 4), dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    assert max(filled.shape) <= 4 ** levels, "the box does not fit the tree"
    key = np.zeros(len(x), dtype=np.uint64)
    for l in range(levels):                                   # one 6-bit digit per level, least significant level first
        s = np.uint64(2 * l)
        digit = ((x >> s) & np.uint64(3)) | (((y >> s) & np.uint64(3)) << np.uint64(2)) | (((z >> s) & np.uint64(3)) << np.uint64(4))
        key |= digit << np.uint64(6 * l)
    order = np.argsort(key, kind="stable")
    cur = key[order]
    materials = ids[filled][order]                            # ids[filled] is in the same (z, y, x) order as np.nonzero
    per_level = [None] * (levels + 1)
    for l in range(1, levels + 1):                            # level l groups the entities of level l - 1 by key >> 6
        parent, bit = cur >> np.uint64(6), cur & np.uint64(63)
        first = np.flatnonzero(np.concatenate([[True], parent[1:] != parent[:-1]]))
        mask = np.bitwise_or.reduceat(np.uint64(1) << bit, first)
        nodes = np.zeros((len(first), 4), dtype=np.uint32)
        nodes[:, 0] = (mask & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        nodes[:, 1] = (mask >> np.uint64(32)).astype(np.uint32)
        nodes[:, 2] = first.astype(np.uint32)
        per_level[l] = nodes
        cur = parent[first]
    assert len(per_level[levels]) == 1
    start, at = [0] * (levels + 1), 0
    for l in range(levels, 0, -1):                            # root first
        start[l] = at
        at += len(per_level[l])
    for l in range(2, levels + 1):
        per_level[l][:, 2] += np.uint32(start[l - 1])
    return np.concatenate([per_level[l] for l in range(levels, 0, -1)]), materials


def brick_table(filled: np.ndarray, ids: np.ndarray):
    """{brick coordinate (bx, by, bz): (mask, ids of its voxels in bit order as bytes, material offset)} of the non-empty bricks, from the
    voxels alone — for counting, between two states, the bricks whose content stays while their offset moves (tests of the state a
    volume carries across rebuilds).  The offset is the number of filled voxels of lower key; key order compares the most significant
    digit first, i.e. the interleaved (z, y, x) digit triples from the top."""
    z, y, x = np.nonzero(filled)
    if len(x) == 0:
        return {}
    digits = 1
    while 4 ** digits < max(filled.shape):
        digits += 1
    key = np.zeros(len(x), dtype=np.uint64)
    for l in range(digits):
        key |= (((x >> (2 * l)) & 3) | (((y >> (2 * l)) & 3) << 2) | (((z >> (2 * l)) & 3) << 4)).astype(np.uint64) << np.uint64(6 * l)
    order = np.argsort(key, kind="stable")
    key, mats = key[order], np.asarray(ids, dtype=np.uint32)[z, y, x][order]
    bx, by, bz = x[order] >> 2, y[order] >> 2, z[order] >> 2
    brick = key >> np.uint64(6)
    first = np.flatnonzero(np.concatenate([[True], brick[1:] != brick[:-1]]))
    ends = np.concatenate([first[1:], [len(brick)]])
    masks = np.bitwise_or.reduceat(np.uint64(1) << (key & np.uint64(63)), first)
    return {(int(bx[a]), int(by[a]), int(bz[a])): (int(m), mats[a:b].tobytes(), int(a)) for a, b, m in zip(first, ends, masks)}


class OutsideBox(Exception):
    """An edit that leaves the box: refused, nothing written."""


class DenseModel:
    """density (float32) and ids (uint32), [z][y][x] over the box `shape_xyz` at world voxel `origin`."""

    def __init__(self, origin, shape_xyz):
        self.origin = tuple(int(v) for v in origin)
        self.shape_xyz = tuple(int(v) for v in shape_xyz)
        nx, ny, nz = self.shape_xyz
        self.density = np.zeros((nz, ny, nx), dtype=np.float32)
        self.ids = np.zeros((nz, ny, nx), dtype=np.uint32)

    @property
    def filled(self) -> np.ndarray:
        return self.density > 0                               # NaN, zeros of either sign and negative densities are empty

    def upload(self, density=None, ids=None):
        self.density = np.zeros_like(self.density) if density is None else np.array(density, dtype=np.float32).reshape(self.density.shape)
        self.ids = np.zeros_like(self.ids) if ids is None else np.array(ids, dtype=np.uint32).reshape(self.ids.shape)

    def set_voxels(self, xyz, ids=None, density=None):
        """World coordinates; the last write of a voxel wins; density defaults to 1.0, id to 0."""
        xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
        n = len(xyz)
        if n == 0:
            return
        local = xyz - np.asarray(self.origin, dtype=np.int64)
        if (local < 0).any() or (local >= np.asarray(self.shape_xyz, dtype=np.int64)).any():
            raise OutsideBox("set_voxels: voxel outside the box")
        ids = np.zeros(n, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32).reshape(n)
        density = np.ones(n, dtype=np.float32) if density is None else np.asarray(density, dtype=np.float32).reshape(n)
        nx, ny, _ = self.shape_xyz
        flat = local[:, 0] + (local[:, 2] * ny + local[:, 1]) * nx
        _, at = np.unique(flat[::-1], return_index=True)      # first occurrence in the reversed list = last write
        keep = n - 1 - at
        self.density.reshape(-1)[flat[keep]] = density[keep]
        self.ids.reshape(-1)[flat[keep]] = ids[keep]

    def brush(self, center, radius, value, mode):
        """The sphere brush (reference blok/src/brush.cpp:13-63), every operation rounded to float32.  mode 0 = add, 1 = subtract."""
        f = np.float32
        c = [f(v) for v in center]
        radius, value = f(radius), f(value)
        lo = [int(np.floor(c[a] - radius)) for a in range(3)]
        hi = [int(np.floor(c[a] + radius)) + 1 for a in range(3)]
        for a in range(3):
            if lo[a] < self.origin[a] or hi[a] > self.origin[a] + self.shape_xyz[a]:
                raise OutsideBox("brush: bounding box leaves the box")
        gx, gy, gz = (np.arange(lo[a], hi[a], dtype=np.int64) for a in range(3))
        dx = ((gx.astype(f) + f(0.5)) - c[0])[None, None, :]   # voxel centre = coordinate + 0.5 (exact: |coordinate| <= 32768)
        dy = ((gy.astype(f) + f(0.5)) - c[1])[None, :, None]
        dz = ((gz.astype(f) + f(0.5)) - c[2])[:, None, None]
        dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
        assert dist.dtype == np.float32
        sl = tuple(slice(lo[a] - self.origin[a], hi[a] - self.origin[a]) for a in (2, 1, 0))
        d = self.density[sl]
        new = np.where(d < value, value, d) if mode == 0 else np.where(value < d, value, d)
        self.density[sl] = np.where(dist > radius, d, new)
