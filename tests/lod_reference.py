"""The contract of blok_hip_volume_reduce / blok_hip_volume_lod_model (include/blok_hip.h) as a numpy model — TESTS ONLY, no GPU, written
without looking at csrc/common/lod_core.h: exposure from a padded boolean array, every level by plain loops over its cells and their eight
children, the vote through np.unique.  Also the case tables of tests/test_lod_cpu.py and tests/test_lod_gpu.py."""
from __future__ import annotations

import itertools

import numpy as np

from blok_amd import _ffi
from tests import limit_cases as LC

VOTE_EXPOSED = 1
MAX_LEVELS = 5


def local_region(shape_zyx, origin, lo, hi):
    nz, ny, nx = shape_zyx
    l = [0, 0, 0] if lo is None else [int(lo[a]) - int(origin[a]) for a in range(3)]
    h = [nx, ny, nz] if hi is None else [int(hi[a]) - int(origin[a]) for a in range(3)]
    assert all(0 <= l[a] <= h[a] <= (nx, ny, nz)[a] for a in range(3))
    return l, h


def exposure(density):
    """(filled, exposed) of a whole box: a cell outside the box counts as filled."""
    filled = np.asarray(density) > 0
    p = np.pad(filled, 1, constant_values=True)
    buried = p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    return filled, filled & ~buried


def vote(weights, ids):
    """The id with the largest sum of weights among the pairs with a weight, the smallest on a tie; 0 without a voter."""
    weights, ids = np.asarray(weights, np.int64), np.asarray(ids, np.uint32)
    if not (weights > 0).any():
        return 0
    values, inverse = np.unique(ids[weights > 0], return_inverse=True)      # sorted: argmax takes the first, the smallest id
    sums = np.zeros(len(values), np.int64)
    np.add.at(sums, inverse, weights[weights > 0])
    return int(values[int(np.argmax(sums))])


def level_above(n0, e0, id0, clo0, clo1, cext1, flags):
    """One halving: the planes [z][y][x] of the grid at clo1 with cext1 cells from the planes of the grid at clo0 below it."""
    n1, e1 = np.zeros(cext1[::-1], np.uint16), np.zeros(cext1[::-1], np.uint16)
    id1 = np.zeros(cext1[::-1], np.uint32)
    nz, ny, nx = n0.shape
    for cz, cy, cx in itertools.product(range(cext1[2]), range(cext1[1]), range(cext1[0])):
        ns, es, ids = [], [], []
        for dz, dy, dx in itertools.product(range(2), range(2), range(2)):
            x, y, z = 2 * (clo1[0] + cx) + dx - clo0[0], 2 * (clo1[1] + cy) + dy - clo0[1], 2 * (clo1[2] + cz) + dz - clo0[2]
            if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz:
                ns.append(int(n0[z, y, x])); es.append(int(e0[z, y, x])); ids.append(int(id0[z, y, x]))
        n, e = sum(ns), sum(es)
        if n == 0:
            continue                                # no voter: (0, 0, 0)
        n1[cz, cy, cx], e1[cz, cy, cx] = n, e
        id1[cz, cy, cx] = vote(es if (flags & VOTE_EXPOSED) and e > 0 else ns, ids)
    return n1, e1, id1


def reduce(density, ids, origin, lo=None, hi=None, levels=1, flags=0):
    """(levels, info): per level 1..K the planes (n, e, id) shaped [z][y][x], and one _ffi.LOD_INFO record."""
    d, m = np.asarray(density), np.asarray(ids)
    l, h = local_region(d.shape, origin, lo, hi)
    ext = [h[a] - l[a] for a in range(3)]
    info = np.zeros(1, dtype=_ffi.LOD_INFO)
    info["version"], info["flags"], info["levels"] = 1, flags, levels
    info["lo"][0] = [origin[a] + l[a] for a in range(3)]
    info["ext"][0] = ext
    empty = not all(ext)
    filled, exposed = exposure(d)
    cut = (slice(l[2], h[2]), slice(l[1], h[1]), slice(l[0], h[0]))
    n0, e0, id0 = filled[cut].astype(np.uint16), exposed[cut].astype(np.uint16), m[cut].astype(np.uint32)
    clo0 = [origin[a] + l[a] for a in range(3)]
    whi = [origin[a] + h[a] for a in range(3)]
    out = []
    for j in range(1, levels + 1):
        clo1 = [(origin[a] + l[a]) >> j for a in range(3)]
        chi1 = [(whi[a] + (1 << j) - 1) >> j for a in range(3)]
        cext1 = [0, 0, 0] if empty else [chi1[a] - clo1[a] for a in range(3)]
        n1, e1, id1 = level_above(n0, e0, id0, clo0, clo1, cext1, flags)
        L = info["level"][0][j - 1]
        L["clo"], L["cext"], L["n_cells"] = clo1, cext1, cext1[0] * cext1[1] * cext1[2]
        L["n_filled"], L["n_exposed"], L["sum_n"], L["sum_e"] = int((n1 > 0).sum()), int((e1 > 0).sum()), int(n1.sum(dtype=np.int64)), int(e1.sum(dtype=np.int64))
        out.append((n1, e1, id1))
        n0, e0, id0, clo0 = n1, e1, id1, clo1
    return out, info


def model_voxels(level_planes, min_count):
    """(xyz, ids) of the model blok_hip_volume_lod_model makes of a level: the cells with n >= min_count, relative to the grid's corner, in
    index order."""
    n, _, ids = level_planes
    z, y, x = np.nonzero(n >= min_count)
    return np.stack([x, y, z], axis=1).astype(np.int32), ids[z, y, x].astype(np.uint32)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
# every case: dict(name, origin, shape (x, y, z), d, m, lo, hi, levels, flags)
def case(name, origin, d, m, lo, hi, levels, flags):
    return dict(name=name, origin=tuple(origin), shape=d.shape[::-1], d=d, m=m, lo=lo, hi=hi, levels=levels, flags=flags)


def model_of(c):
    return reduce(c["d"], c["m"], c["origin"], c["lo"], c["hi"], c["levels"], c["flags"])


NOISE_ORIGIN, NOISE_SHAPE = (-5, -3, -2), (13, 10, 7)
NOISE_IDS = np.array([0, 1, 2, 3, 0xFFFFFFFF], np.uint32)      # few ids: ties are common; 0 is the id of filled cells too


def noise(fill, seed=23):
    rng = np.random.default_rng(seed)
    nx, ny, nz = NOISE_SHAPE
    d = np.where(rng.random((nz, ny, nx)) < fill, rng.choice(np.array([0.25, 1.0, 3.5], np.float32), (nz, ny, nx)), np.float32(0)).astype(np.float32)
    empty = ~(d > 0)
    d[empty & (rng.random(d.shape) < 0.2)] = np.float32(-1.0)      # empty cells that are not zero
    d[empty & (rng.random(d.shape) < 0.1)] = np.float32(np.nan)
    m = rng.choice(NOISE_IDS, d.shape).astype(np.uint32)
    return np.ascontiguousarray(d), np.ascontiguousarray(m)


def noise_regions():
    """The whole box, regions off the brick grid and off the 2^K grid (the box's origin is off both too), a one-cell region, an empty one."""
    return [(None, None), ((-4, -2, -1), (7, 6, 4)), ((-3, -3, 0), (4, 7, 5)), ((1, 2, 3), (2, 3, 4)), ((0, 0, 0), (0, 4, 4))]


def noise_cases():
    out = []
    for fill in (0.05, 0.5):
        d, m = noise(fill)
        for r, (lo, hi) in enumerate(noise_regions()):
            for levels in range(1, MAX_LEVELS + 1):
                flags = VOTE_EXPOSED if (levels + r) % 2 else 0
                out.append(case(f"noise {fill} {lo}..{hi} K {levels} flags {flags}", NOISE_ORIGIN, d, m, lo, hi, levels, flags))
    return out


SEAMS = (0, 1, 3, 4, 63, 64, 255, 256, 298, 299)   # travel positions: the seams of a brick, of a wave's 128 voxels, of a block's rows, and both ends
SEAM_LENGTH = 300
SEAM_ORIGIN = (7, -150, -3)


def seam_box(axis):
    """5 x 300 x 6 (axis 1) and its permutations: filled cells at the SEAMS along the axis and their neighbours on the two other axes, in
    the column (2, 3) and, alone, in the column (0, 0)."""
    shape = [0, 0, 0]
    shape[axis], shape[(axis + 1) % 3], shape[(axis + 2) % 3] = SEAM_LENGTH, 5, 6
    d, m = np.zeros(shape[::-1], np.float32), np.zeros(shape[::-1], np.uint32)
    dm, mm = np.moveaxis(d, 2 - axis, -1), np.moveaxis(m, 2 - axis, -1)      # views: [..][..][along]
    for k, t in enumerate(SEAMS):
        for du, dv in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            dm[2 + du, 3 + dv, t], mm[2 + du, 3 + dv, t] = 0.5 + k, 1 + (k + du + 2 * dv) % 3
        dm[0, 0, t], mm[0, 0, t] = 1.0, 7
    m[m == 0] = 99                                  # ids under empty cells: never reported
    return d, m


def seam_cases():
    out = []
    for axis in range(3):
        d, m = seam_box(axis)
        lo, hi = list(SEAM_ORIGIN), [SEAM_ORIGIN[a] + d.shape[2 - a] for a in range(3)]
        lo[axis] += 1; hi[axis] -= 1               # cells 1 .. 298: the region cuts the first and the last coarse cell
        out.append(case(f"seams axis {axis}", SEAM_ORIGIN, d, m, None, None, 2, VOTE_EXPOSED))
        out.append(case(f"seams 1..298 axis {axis}", SEAM_ORIGIN, d, m, tuple(lo), tuple(hi), 1, 0))
    return out


def limit_case(which):
    """LC.SHAPE at an end of the lattice: a slab with a one-cell skin of another id, holes, and the box's corners."""
    nx, ny, nz = LC.SHAPE
    rng = np.random.default_rng(29)
    y = np.arange(ny)[None, :, None]
    d = np.where((y < 40) & (rng.random((nz, ny, nx)) < 0.97), np.float32(1.0), np.float32(0)).astype(np.float32)
    m = np.where(y == 39, 1, 2).astype(np.uint32) * np.ones((nz, 1, nx), np.uint32)
    d[0, 0, 0] = d[-1, -1, -1] = 1.0
    m[-1, -1, -1] = 0xFFFFFFFF
    return case(f"limit {which}", LC.limit_origin(which, LC.SHAPE), np.ascontiguousarray(d), np.ascontiguousarray(m), None, None, 2, VOTE_EXPOSED)


# ---- the long boxes: isolated voxels in closed form -------------------------------------------------------------------------------------------
LONG_LEVELS = 2


def long_filled(box):
    """(t, u, v) -> filled, as arrays that broadcast to the box: at most one voxel in every world-aligned 4^3 cell Q, at an offset that turns
    with Q, and none where (qx + 3 qy + 5 qz) % 7 == 0 — no two of them touch a common level-2 cell, and every one is exposed (its cell's
    other 63 voxels are empty, and no extent of a long box is 1)."""
    nx, ny, nz = box.shape
    w = [box.origin[a] + g for a, g in enumerate((np.arange(nx, dtype=np.int64)[None, None, :], np.arange(ny, dtype=np.int64)[None, :, None],
                                                  np.arange(nz, dtype=np.int64)[:, None, None]))]
    q = [c >> 2 for c in w]
    keep = (q[0] + 3 * q[1] + 5 * q[2]) % 7 != 0
    return keep & ((w[0] & 3) == (q[0] + q[1]) % 4) & ((w[1] & 3) == (q[1] + q[2]) % 4) & ((w[2] & 3) == (q[2] + q[0]) % 4)


def long_fill(box):
    t, u, v = box.tuv()
    filled = long_filled(box)
    d = np.where(filled, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    ids = np.where((t + u) % 11 == 0, 0xFFFFFFFF, (7 * t + u + 3 * v) % 5).astype(np.uint32)
    return np.ascontiguousarray(d), np.ascontiguousarray(np.broadcast_to(ids, d.shape))


def long_expected(box, d, m):
    """The planes of levels 1 and 2 of the whole box, from long_filled's property alone: every filled voxel is the one voter of its cells."""
    filled, exposed = exposure(d)
    z, y, x = np.nonzero(filled)
    w = [x + box.origin[0], y + box.origin[1], z + box.origin[2]]
    out = []
    for j in (1, 2):
        clo = [box.origin[a] >> j for a in range(3)]
        cext = [((box.hi[a] + (1 << j) - 1) >> j) - clo[a] for a in range(3)]
        n, e, ids = np.zeros(cext[::-1], np.uint16), np.zeros(cext[::-1], np.uint16), np.zeros(cext[::-1], np.uint32)
        at = ((w[2] >> j) - clo[2], (w[1] >> j) - clo[1], (w[0] >> j) - clo[0])
        np.add.at(n, at, 1)
        np.add.at(e, at, exposed[z, y, x].astype(np.uint16))
        ids[at] = m[z, y, x]
        assert int(n.max()) <= 1
        out.append((n, e, ids))
    return out
