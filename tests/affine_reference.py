"""A plain model of resampling a model into a voxel volume through an affine map — TESTS ONLY, numpy and Python integers alone, written
from the contract in include/blok_hip.h (blok_hip_volume_stamp_affine), not from the product's shared header and independent of both C++
builds.

A record is a mapping with "anchor" (3 ints, a world voxel), "m" (3 x 3 ints, world -> model, 2^-16 model voxel per world voxel) and "t"
(3 ints, the model-space position of the centre of world voxel anchor, 2^-16 model voxel).  For a world voxel w
    P_k(w) = t_k + sum_j m[k][j] * (w_j - anchor_j),    v_k = P_k >> 16 (a floor),
and w is touched iff it lies in the region and the model has a voxel at v.  Arrays are [z][y][x] over a box whose voxel (0, 0, 0) sits at
world `origin`; a voxel is filled iff density > 0."""
from __future__ import annotations

import math

import numpy as np

from tests.stamp_reference import ERASE, KEEP, SET, large_model, last_wins, small_model  # noqa: F401

ONE = 1 << 16


def record(anchor, m, t, model=0):
    return {"model": int(model), "anchor": [int(c) for c in anchor], "m": [[int(c) for c in row] for row in m], "t": [int(c) for c in t]}


def fields(rec):
    """A record of any kind (a mapping, or one element of a structured array with these field names) as a mapping of Python ints."""
    if isinstance(rec, dict):
        return rec
    r = np.asarray(rec).reshape(-1)[0]
    return record(r["anchor"].tolist(), r["m"].tolist(), r["t"].tolist(), int(r["model"]))


def sample_exact(rec, w):
    """v of one world voxel in unbounded Python integers: (P, v), three each."""
    r = fields(rec)
    P = [int(r["t"][k]) + sum(int(r["m"][k][j]) * (int(w[j]) - int(r["anchor"][j])) for j in range(3)) for k in range(3)]
    return P, [p >> 16 for p in P]


def sample_grid(rec, lo, hi):
    """v of every world voxel of [lo, hi): three int64 arrays [z][y][x]."""
    r = fields(rec)
    z, y, x = np.meshgrid(np.arange(lo[2], hi[2], dtype=np.int64), np.arange(lo[1], hi[1], dtype=np.int64), np.arange(lo[0], hi[0], dtype=np.int64),
                          indexing="ij")
    w = (x - r["anchor"][0], y - r["anchor"][1], z - r["anchor"][2])
    return [(np.int64(r["t"][k]) + np.int64(r["m"][k][0]) * w[0] + np.int64(r["m"][k][1]) * w[1] + np.int64(r["m"][k][2]) * w[2]) >> 16 for k in range(3)]


class Dense:
    """The model's voxels as a dense array of its box: filled, material."""

    def __init__(self, model_xyz, model_mats):
        v, m = last_wins(model_xyz, model_mats)
        self.lo, self.hi = v.min(axis=0), v.max(axis=0) + 1
        ex = self.hi - self.lo
        self.filled = np.zeros((ex[2], ex[1], ex[0]), dtype=bool)
        self.material = np.zeros((ex[2], ex[1], ex[0]), dtype=np.uint32)
        c = v - self.lo
        self.filled[c[:, 2], c[:, 1], c[:, 0]] = True
        self.material[c[:, 2], c[:, 1], c[:, 0]] = m

    def lookup(self, v):
        """(hit, material) arrays for the voxel arrays v = [vx, vy, vz]."""
        inside = np.ones(v[0].shape, dtype=bool)
        for k in range(3):
            inside &= (v[k] >= self.lo[k]) & (v[k] < self.hi[k])
        c = [np.where(inside, v[k] - self.lo[k], 0) for k in range(3)]
        return inside & self.filled[c[2], c[1], c[0]], self.material[c[2], c[1], c[0]]


_dense_cache = {}


def dense_of(model_xyz, model_mats) -> Dense:
    key = (id(model_xyz), id(model_mats))
    if key not in _dense_cache:
        _dense_cache[key] = (Dense(model_xyz, model_mats), model_xyz, model_mats)      # (the arrays are kept alive: their ids stay theirs)
    return _dense_cache[key][0]


def region_of(density, origin, lo, hi):
    nz, ny, nx = density.shape
    o = np.asarray(origin, dtype=np.int64)
    l = o.copy() if lo is None else np.asarray(lo, dtype=np.int64)
    h = o + [nx, ny, nz] if hi is None else np.asarray(hi, dtype=np.int64)
    assert (l >= o).all() and (h <= o + [nx, ny, nz]).all() and (l <= h).all()
    return l, h


def stamp(density, ids, origin, model_xyz, model_mats, rec, lo, hi, mode, value) -> int:
    """Applies one record in place over the region [lo, hi) (world voxels; both None = the whole box).  Returns the cells written."""
    l, h = region_of(density, origin, lo, hi)
    if (l >= h).any():
        return 0
    hit, mat = dense_of(model_xyz, model_mats).lookup(sample_grid(rec, l, h))
    o = np.asarray(origin, dtype=np.int64)
    sl = (slice(l[2] - o[2], h[2] - o[2]), slice(l[1] - o[1], h[1] - o[1]), slice(l[0] - o[0], h[0] - o[0]))
    d, i = density[sl], ids[sl]                               # views
    if mode == ERASE:
        d[hit] = np.float32(0.0)
        i[hit] = 0
        return int(hit.sum())
    if mode == KEEP:
        hit = hit & ~(d > 0)                                  # 0, negative and NaN are empty
    else:
        assert mode == SET
    d[hit] = np.float32(value)
    i[hit] = mat[hit]
    return int(hit.sum())


# ---- which way a wave of the kernel goes, from the rule alone ------------------------------------------------------------------------

def tile_classes(rec, origin, shape_xyz, lo, hi, model_xyz, model_mats):
    """Counts, over the 64 x 4 x 4 tiles (counted from the box's corner) of the region, of the ways a tile can go: found from the sampled
    voxels themselves, tile by tile, with no interval arithmetic.
      outside: no axis-aligned box around the tile's voxels meets the model's box;   cut: it meets the box, not every cell lies inside it;
      empty cell: all voxels share one cell of the model's 4-ary grid (counted from the tree's corner) that holds no voxel;
      one voxel: all cells sample one filled voxel;   far apart: the voxels of one row of 64 cells spread over more than 64 bricks' width;
      row skipped: the tile meets the box, one of its rows alone does not."""
    dense = dense_of(model_xyz, model_mats)
    l, h = region_of(np.zeros(tuple(shape_xyz)[::-1], dtype=np.float32), origin, lo, hi)
    v = sample_grid(rec, l, h)
    corner = dense.lo // 16 * 16                              # the tree's corner (tree_build: floor_to(lo, 16))
    out = {"outside": 0, "cut": 0, "empty cell": 0, "one voxel": 0, "far apart": 0, "row skipped": 0, "tiles": 0}
    o = np.asarray(origin, dtype=np.int64)
    t0, t1 = (l - o) // [64, 4, 4], (h - 1 - o) // [64, 4, 4]
    for tz in range(t0[2], t1[2] + 1):
        for ty in range(t0[1], t1[1] + 1):
            for tx in range(t0[0], t1[0] + 1):
                c0 = np.maximum(o + [tx * 64, ty * 4, tz * 4], l) - l
                c1 = np.minimum(o + [tx * 64 + 64, ty * 4 + 4, tz * 4 + 4], h) - l
                sl = (slice(c0[2], c1[2]), slice(c0[1], c1[1]), slice(c0[0], c1[0]))
                tv = [a[sl] for a in v]
                out["tiles"] += 1
                vmin, vmax = [int(a.min()) for a in tv], [int(a.max()) for a in tv]
                meets = all(vmax[k] >= dense.lo[k] and vmin[k] < dense.hi[k] for k in range(3))
                if not meets:
                    out["outside"] += 1
                    continue
                inside = all(vmin[k] >= dense.lo[k] and vmax[k] < dense.hi[k] for k in range(3))
                out["cut"] += 0 if inside else 1
                rows_meet = [all(tv[k][z, y].max() >= dense.lo[k] and tv[k][z, y].min() < dense.hi[k] for k in range(3))
                             for z in range(tv[0].shape[0]) for y in range(tv[0].shape[1])]
                out["row skipped"] += 0 if all(rows_meet) else 1
                hit, _ = dense.lookup(tv)
                if vmin == vmax and hit.all():
                    out["one voxel"] += 1
                if any(int((tv[k][z, y].max() - tv[k][z, y].min())) > 256 for k in range(3) for z in range(tv[0].shape[0]) for y in range(tv[0].shape[1])):
                    out["far apart"] += 1
                # the smallest cell of the 4-ary grid that holds every voxel of the tile
                rel_lo, rel_hi = [vmin[k] - int(corner[k]) for k in range(3)], [vmax[k] - int(corner[k]) for k in range(3)]
                if min(rel_lo) >= 0:
                    level = 0
                    while any((rel_lo[k] >> (2 * level)) != (rel_hi[k] >> (2 * level)) for k in range(3)):
                        level += 1
                    cell_lo = [((rel_lo[k] >> (2 * level)) << (2 * level)) + int(corner[k]) for k in range(3)]
                    size = 1 << (2 * level)
                    a = [max(cell_lo[k], int(dense.lo[k])) - int(dense.lo[k]) for k in range(3)]
                    b = [min(cell_lo[k] + size, int(dense.hi[k])) - int(dense.lo[k]) for k in range(3)]
                    if level >= 1 and (min(b[k] - a[k] for k in range(3)) <= 0 or not dense.filled[a[2]:b[2], a[1]:b[1], a[0]:b[0]].any()):
                        out["empty cell"] += 1
    return out


# ---- the models and the matrix table the CPU and GPU tests share --------------------------------------------------------------------

def block_model():
    """12^3 with holes over [-5, 7)^3: two tree levels."""
    g = np.arange(-5, 7)
    x, y, z = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    keep = ((x * 5 + y * 3 + z * 7) % 6 != 0) | ((np.abs(x + 0.5) > 5) & (np.abs(y + 0.5) > 5) & (np.abs(z + 0.5) > 5))
    xyz = np.stack([x[keep], y[keep], z[keep]], axis=1).astype(np.int32)
    assert tuple(xyz.min(axis=0)) == (-5, -5, -5) and tuple(xyz.max(axis=0)) == (6, 6, 6)
    return xyz, (np.arange(len(xyz)) * 3 + 11).astype(np.uint32)


def sparse_model():
    """Extent 256 over [-96, 160)^3, about 4000 scattered voxels and a few solid 16-cells: four tree levels, most of its space empty."""
    rng = np.random.default_rng(41)
    pts = [rng.integers(-96, 160, size=(4000, 3)), [[-96, -96, -96], [159, 159, 159]]]
    g = np.arange(16)
    cell = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    for c in ((0, 0, 0), (64, 32, -48), (-80, 112, 96)):
        pts.append(cell + np.asarray(c))
    xyz = np.unique(np.concatenate(pts).astype(np.int32), axis=0)
    return xyz, (np.arange(len(xyz)) % 900 + 1).astype(np.uint32)


MODELS = {"small": small_model(), "block": block_model(), "large": large_model(), "sparse": sparse_model()}      # 1, 2, 3 and 4 tree levels
LEVELS = {"small": 1, "block": 2, "large": 3, "sparse": 4}

ORIGIN, SHAPE = (-40, -44, -24), (96, 80, 64)
ODD_ORIGIN, ODD_SHAPE = (-33, -41, -17), (97, 78, 61)


def rot(yaw=0.0, pitch=0.0, roll=0.0):
    """Ry(yaw) Rx(pitch) Rz(roll), degrees."""
    y, p, r = (math.radians(a) for a in (yaw, pitch, roll))
    ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]])
    return ry @ rx @ rz


def forward(linear, translation):
    return np.concatenate([np.asarray(linear, dtype=np.float64), np.asarray(translation, dtype=np.float64).reshape(3, 1)], axis=1)


# name -> (model, ("matrix", forward 3 x 4) or ("record", record), region (lo, hi) or None for the whole box).  The matrices are inverted
# by the product's own helper (blok_affine_from_matrix); the singular ones cannot be and are written as records.
CASES = {
    "yaw 30": ("large", ("matrix", forward(rot(30), (8.3, -4.2, 6.7))), None),
    "compound rotation, scale 1.5": ("large", ("matrix", forward(1.5 * rot(40, 25, -15), (5.0, -3.0, 4.0))), None),
    "scale 0.5": ("large", ("matrix", forward(0.5 * np.eye(3), (3.5, 2.0, 1.0))), None),
    "scale 2.75": ("large", ("matrix", forward(2.75 * np.eye(3), (10.0, -5.0, 9.0))), None),
    "scale 1/64, sparse": ("sparse", ("matrix", forward(np.eye(3) / 64.0, (2.5, 1.5, 3.5))), None),
    "scale 0.25, sparse": ("sparse", ("matrix", forward(0.25 * rot(10), (-4.0, -12.0, 0.0))), None),
    "scale 16, sparse": ("sparse", ("matrix", forward(16.0 * np.eye(3), (24.0, 4.0, 8.0))), None),
    "mirror": ("large", ("matrix", forward(rot(20) @ np.diag([-1.0, 1.0, 1.0]), (6.0, -2.0, 3.0))), None),
    "shear": ("large", ("matrix", forward([[1, 0.5, 0], [0, 1, 0.25], [0, 0, 1]], (4.0, -6.0, 2.0))), None),
    "rank 2": ("large", ("record", record((3, -2, 1), [[ONE, 0, 0], [0, ONE, 0], [0, 0, 0]], [ONE // 2, ONE // 2, ONE // 2])), None),
    "rank 0, on a voxel": ("small", ("record", record((0, 0, 0), [[0] * 3] * 3, [ONE + ONE // 2, ONE // 2, ONE // 2])), ((-10, -10, -10), (23, 7, 5))),
    "rank 0, on a hole": ("small", ("record", record((0, 0, 0), [[0] * 3] * 3, [ONE // 2, ONE // 2, ONE // 2])), ((-10, -10, -10), (23, 7, 5))),
    "scale 8": ("small", ("matrix", forward(8.0 * np.eye(3), (-12.0, -20.0, -8.0))), None),
    "scale 8, a region 8 cells wide": ("small", ("matrix", forward(8.0 * np.eye(3), (-12.0, -20.0, -8.0))), ((-12, -44, -24), (-4, 36, 40))),
    "scale 12, every side": ("block", ("matrix", forward(12.0 * np.eye(3), (8.0, -4.0, 8.0))), None),
    # each model enlarged or turned so that it hangs out of the box on every side
    "scale 48, small, every side": ("small", ("matrix", forward(48.0 * np.eye(3), (0.0, 0.0, 0.0))), None),
    "scale 12 turned, large, every side": ("large", ("matrix", forward(12.0 * rot(15, 10, 0), (0.0, 0.0, 0.0))), None),
    "yaw 20, sparse, every side": ("sparse", ("matrix", forward(rot(20), (0.0, 0.0, 0.0))), None),
    "one cell": ("large", ("matrix", forward(rot(30), (8.3, -4.2, 6.7))), ((9, -3, 7), (10, -2, 8))),
    "x ends at 63": ("large", ("matrix", forward(rot(30), (8.3, -4.2, 6.7))), ((-40, -30, -10), (23, 21, 30))),
    "x ends at 64": ("large", ("matrix", forward(rot(30), (8.3, -4.2, 6.7))), ((-40, -30, -10), (24, 22, 31))),
    "x ends at 65": ("large", ("matrix", forward(rot(30), (8.3, -4.2, 6.7))), ((-40, -30, -10), (25, 23, 29))),
}
assert (0, 0, 0) not in {tuple(v) for v in MODELS["small"][0]} and (1, 0, 0) in {tuple(v) for v in MODELS["small"][0]}
