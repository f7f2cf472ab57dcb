"""A plain model of the column field and of scatter — TESTS ONLY, numpy alone, written from the contract in include/blok_hip.h
(blok_hip_volume_column_field, blok_hip_volume_scatter_models), not from the product's shared header — and the case tables the CPU and the
GPU tests share.

Arrays are [z][y][x] over a box whose voxel (0, 0, 0) sits at world `origin`; a cell is filled iff density > 0.  A field is the triple
(top uint16, material uint32, info _ffi.COLUMNS_INFO), the planes flat in column order cp + ext[p] * cq (p < q the axes other than the
field's)."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi

NONE = 0xFFFF
FROM_LOW = 1
ANY_MATERIAL, ROTATE, MIRROR = 1, 2, 4
NO_LIMIT = 0xFFFF
SEED = 0x5EED0003                                   # the default seed: test_columns_cpu.py asserts that it makes the scatter cases hard


# ---- the field ---------------------------------------------------------------------------------------------------------------------------
def local_region(shape_zyx, origin, lo, hi):
    nz, ny, nx = shape_zyx
    l = [0, 0, 0] if lo is None else [int(lo[a]) - int(origin[a]) for a in range(3)]
    h = [nx, ny, nz] if hi is None else [int(hi[a]) - int(origin[a]) for a in range(3)]
    assert all(0 <= l[a] <= h[a] <= (nx, ny, nz)[a] for a in range(3))
    return l, h


def field(density, ids, origin, lo=None, hi=None, axis=1, flags=0):
    """(top, material, info) of the region [lo, hi) (world voxels; both None = the whole box) along `axis`: argmax over density > 0."""
    d, m = np.asarray(density), np.asarray(ids)
    l, h = local_region(d.shape, origin, lo, hi)
    ext = [h[a] - l[a] for a in range(3)]
    info = np.zeros(1, dtype=_ffi.COLUMNS_INFO)
    info["version"], info["flags"], info["axis"] = 1, flags, axis
    info["lo"][0] = [int(origin[a]) + l[a] for a in range(3)]
    info["ext"][0] = ext
    info["min_top"], info["max_top"] = NONE, 0
    if not all(ext):
        return np.zeros(0, np.uint16), np.zeros(0, np.uint32), info
    with np.errstate(invalid="ignore"):
        f = d[l[2]:h[2], l[1]:h[1], l[0]:h[0]] > 0
    g = np.moveaxis(f, 2 - axis, -1)               # [cq][cp][along]
    gi = np.moveaxis(m[l[2]:h[2], l[1]:h[1], l[0]:h[0]], 2 - axis, -1)
    n = g.shape[-1]
    hit = g.any(axis=-1)
    first = g.argmax(axis=-1) if flags & FROM_LOW else n - 1 - g[..., ::-1].argmax(axis=-1)
    top = np.where(hit, first, NONE).astype(np.uint16)
    material = np.where(hit, np.take_along_axis(gi, first[..., None], axis=-1)[..., 0], 0).astype(np.uint32)
    info["n_columns"], info["n_hit"] = top.size, int(hit.sum())
    if hit.any():
        info["min_top"], info["max_top"] = int(first[hit].min()), int(first[hit].max())
    return np.ascontiguousarray(top).reshape(-1), np.ascontiguousarray(material).reshape(-1), info


# ---- scatter -------------------------------------------------------------------------------------------------------------------------------
def fmix32(h):
    h = h ^ (h >> np.uint32(16)); h = h * np.uint32(0x85EBCA6B); h = h ^ (h >> np.uint32(13)); h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def hash3(x, y, z, s):
    """The terrain's hash, in numpy uint32 arithmetic (wrapping products)."""
    with np.errstate(over="ignore"):
        x, y, z, s = (np.asarray(v).astype(np.int64).astype(np.uint32) for v in (x, y, z, s))
        return fmix32(x * np.uint32(0x9E3779B1) ^ y * np.uint32(0x85EBCA77) ^ z * np.uint32(0xC2B2AE3D) ^ s)


def params(**kw):
    """One _ffi.SCATTER_PARAMS record; the defaults reject nothing."""
    p = np.zeros(1, dtype=_ffi.SCATTER_PARAMS)
    base = dict(seed=SEED, flags=0, cell_log2=0, probability=65536, surface_material=0, min_y=-(1 << 31), max_y=(1 << 31) - 1, radius=0, max_rise=NO_LIMIT,
                max_drop=NO_LIMIT)
    base.update(kw)
    for k, v in base.items():
        p[k] = v
    return p


def entries(rows):
    """_ffi.SCATTER_ENTRY records from (model, weight, anchor, sink) rows."""
    e = np.zeros(len(rows), dtype=_ffi.SCATTER_ENTRY)
    for i, (model, weight, anchor, sink) in enumerate(rows):
        e[i] = (model, weight, tuple(anchor), sink)
    return e


FLIP_OF_ROTATION = (0, 4, 5, 1)


def scatter(top, material, info, p, ent, trace=None):
    """(table of _ffi.INSTANCE sorted by column, info _ffi.SCATTER_INFO) of a field along +y from the top: a plain loop over the cells.
    trace, a list, receives (X, Z, verdict, entry, rotation, mirror, window cut by the region) per counted cell; verdict 0 = placed,
    1..5 = the test that failed."""
    p = np.asarray(p).reshape(1)[0]
    info = np.asarray(info).reshape(1)[0]
    assert int(info["axis"]) == 1 and not int(info["flags"]) & FROM_LOW
    lo, ext = [int(v) for v in info["lo"]], [int(v) for v in info["ext"]]
    c, seed, flags, radius = int(p["cell_log2"]), int(p["seed"]), int(p["flags"]), int(p["radius"])
    S = 1 << c
    out = np.zeros(1, dtype=_ffi.SCATTER_INFO)
    out["version"], out["flags"] = 1, flags
    rows = []
    if all(ext):
        t2 = np.asarray(top).reshape(ext[2], ext[0]).astype(np.int64)
        m2 = np.asarray(material).reshape(ext[2], ext[0])
        cxs = np.arange(lo[0] >> c, ((lo[0] + ext[0] - 1) >> c) + 1, dtype=np.int64)
        czs = np.arange(lo[2] >> c, ((lo[2] + ext[2] - 1) >> c) + 1, dtype=np.int64)
        gx, gz = np.meshgrid(cxs, czs, indexing="ij")
        h1s, h2s = hash3(gx, 0x5CA70001, gz, seed), hash3(gx, 0x5CA70002, gz, seed)
        weights = [int(w) for w in ent["weight"]]
        W = sum(weights)
        for i, cx in enumerate(cxs.tolist()):
            for j, cz in enumerate(czs.tolist()):
                h1, h2 = int(h1s[i, j]), int(h2s[i, j])
                X, Z = (cx << c) + (h1 & (S - 1)), (cz << c) + ((h1 >> 8) & (S - 1))
                x, z = X - lo[0], Z - lo[2]
                if not (0 <= x < ext[0] and 0 <= z < ext[2]):
                    continue
                out["n_cells"] += 1
                t = int(t2[z, x])
                cut = x < radius or z < radius or x + radius >= ext[0] or z + radius >= ext[2]
                failed = 0
                if not (h1 >> 16) < int(p["probability"]):
                    failed = 1
                elif t == NONE:
                    failed = 2
                elif not int(p["min_y"]) <= lo[1] + t <= int(p["max_y"]):
                    failed = 3
                elif not (flags & ANY_MATERIAL or int(m2[z, x]) == int(p["surface_material"])):
                    failed = 4
                else:
                    w = t2[max(z - radius, 0):z + radius + 1, max(x - radius, 0):x + radius + 1]
                    rise, drop = int(p["max_rise"]), int(p["max_drop"])
                    if (rise != NO_LIMIT and not (w <= t + rise).all()) or (drop != NO_LIMIT and not ((w != NONE) & (w + drop >= t)).all()):
                        failed = 5
                pick = (h2 & 0xFFFF) % W
                e = next(k for k in range(len(weights)) if sum(weights[:k + 1]) > pick)
                r = (h2 >> 16) & 3 if flags & ROTATE else 0
                m = (h2 >> 18) & 1 if flags & MIRROR else 0
                if trace is not None:
                    trace.append((X, Z, failed, e, r, m, cut))
                if failed:
                    out["n_rejected"][0][failed - 1] += 1
                    continue
                out["n_placed"] += 1
                axis = (2, 1, 0) if r & 1 else (0, 1, 2)
                flip = FLIP_OF_ROTATION[r] ^ m
                T = (X, lo[1] + t + 1 - int(ent["sink"][e]), Z)
                offset = [0, 0, 0]
                for k in range(3):
                    A = axis[k]
                    offset[A] = T[A] + 1 + int(ent["anchor"][e][k]) if (flip >> k) & 1 else T[A] - int(ent["anchor"][e][k])
                rows.append((x + ext[0] * z, (int(ent["model"][e]), tuple(offset), axis, flip, (0, 0, 0))))
    rows.sort(key=lambda row: row[0])
    assert len({row[0] for row in rows}) == len(rows)
    table = np.zeros(len(rows), dtype=_ffi.INSTANCE)
    for i, (_, rec) in enumerate(rows):
        table[i] = rec
    return table, out


def anchor_lands_on(instance, anchor):
    """The world voxel of the model voxel `anchor` under the header's record-back rule."""
    w = [0, 0, 0]
    for k in range(3):
        a = int(instance["axis"][k])
        w[a] = int(instance["offset"][a]) - 1 - int(anchor[k]) if (int(instance["flip"]) >> k) & 1 else int(instance["offset"][a]) + int(anchor[k])
    return tuple(w)


# ---- field cases -----------------------------------------------------------------------------------------------------------------------------
# every case: dict(name, origin, shape (x, y, z), d, m, lo, hi, axis, flags); `hard`: test_columns_cpu.py asserts the hardness properties on it
def case(name, origin, d, m, lo, hi, axis, flags, hard=False):
    return dict(name=name, origin=tuple(origin), shape=d.shape[::-1], d=d, m=m, lo=lo, hi=hi, axis=axis, flags=flags, hard=hard)


def model_of(c):
    return field(c["d"], c["m"], c["origin"], c["lo"], c["hi"], c["axis"], c["flags"])


NOISE_ORIGIN, NOISE_SHAPE = (-5, -3, -2), (13, 10, 7)


def noise(fill, seed=11):
    rng = np.random.default_rng(seed)
    nx, ny, nz = NOISE_SHAPE
    d = np.where(rng.random((nz, ny, nx)) < fill, rng.choice(np.array([0.25, 1.0, 3.5], np.float32), (nz, ny, nx)), np.float32(0)).astype(np.float32)
    empty = ~(d > 0)
    d[empty & (rng.random(d.shape) < 0.2)] = np.float32(-1.0)      # empty cells that are not zero
    d[empty & (rng.random(d.shape) < 0.1)] = np.float32(np.nan)
    m = rng.integers(1, 250, d.shape).astype(np.uint32)
    return np.ascontiguousarray(d), m


def noise_regions():
    """The whole box, regions off the brick grid (the box's origin is off it too), a one-cell region, an empty region."""
    return [(None, None), ((-4, -2, -1), (7, 6, 4)), ((-2, -3, 0), (3, 7, 5)), ((1, 2, 3), (2, 3, 4)), ((0, 0, 0), (0, 4, 4))]


def noise_cases():
    out = []
    for fill in (0.05, 0.5):
        d, m = noise(fill)
        for lo, hi in noise_regions():
            for axis in range(3):
                for flags in (0, FROM_LOW):
                    out.append(case(f"noise {fill} {lo}..{hi} axis {axis} flags {flags}", NOISE_ORIGIN, d, m, lo, hi, axis, flags))
    return out


SEAMS = (0, 1, 3, 4, 63, 64, 255, 256, 298, 299)   # travel positions of the one filled cell of a column: the seams of a brick, of a group of 4, 16 and 64 bricks, and both ends twice
SEAM_LENGTH = 300


def axes_shape(axis, along, p_ext, q_ext):
    shape = [0, 0, 0]
    shape[axis], shape[1 if axis == 0 else 0], shape[1 if axis == 2 else 2] = along, p_ext, q_ext
    return tuple(shape)


def seam_box(axis):
    """5 x 300 x 6 (axis 1) and its permutations: column k (k < 10) holds one filled cell at SEAMS[k]; the others hold none."""
    shape = axes_shape(axis, SEAM_LENGTH, 5, 6)
    d, m = np.zeros(shape[::-1], np.float32), np.zeros(shape[::-1], np.uint32)
    dm, mm = np.moveaxis(d, 2 - axis, -1), np.moveaxis(m, 2 - axis, -1)      # views: [cq][cp][along]
    for k, t in enumerate(SEAMS):
        column = 2 * k + 1
        dm[column // 5, column % 5, t], mm[column // 5, column % 5, t] = 0.5 + k, 10 + k
    m[m == 0] = 99                                  # ids under empty cells: never reported
    assert int((d > 0).sum()) == len(SEAMS)
    return d, m


def seam_cases():
    out = []
    for axis in range(3):
        d, m = seam_box(axis)
        origin = (7, -150, -3)
        lo, hi = list(origin), [origin[a] + d.shape[2 - a] for a in range(3)]
        lo[axis] += 1; hi[axis] -= 1               # cells 1 .. 298: the region cuts the first and the last brick
        for flags in (0, FROM_LOW):
            out.append(case(f"seams axis {axis} flags {flags}", origin, d, m, None, None, axis, flags))
            out.append(case(f"seams 1..298 axis {axis} flags {flags}", origin, d, m, tuple(lo), tuple(hi), axis, flags, hard=True))
    return out


STEPS = (63, 64, 65, 255, 256)


def stair_box(long_axis):
    """300 x 5 x 5 and its permutations: more than 64 and more than 256 columns side by side.  A staircase over the long coordinate s: every
    cell at or below (number of STEPS <= s) + w mod 5 along either short axis is filled (w: the other short coordinate), with a hole under
    some tops."""
    shape = [5, 5, 5]
    shape[long_axis] = 300
    nx, ny, nz = shape
    g = [np.arange(nx)[None, None, :], np.arange(ny)[None, :, None], np.arange(nz)[:, None, None]]
    s = g[long_axis]
    a, b = [k for k in range(3) if k != long_axis]
    level = sum((s >= t).astype(np.int64) for t in STEPS)
    d = np.zeros((nz, ny, nx), np.float32)
    # filled where the coordinate along a is at most (level + b coordinate) % 5: a field along a sees the staircase, one along b its transpose
    d[np.broadcast_to(g[a] <= (level + g[b]) % 5, d.shape)] = 1.0
    d[np.broadcast_to((g[a] == 1) & (s % 7 == 3), d.shape)] = 0.0
    m = (1 + (g[0] + 3 * g[1] + 7 * g[2]) % 200).astype(np.uint32)
    return np.ascontiguousarray(d), np.ascontiguousarray(np.broadcast_to(m, d.shape))


def stair_cases():
    out = []
    for long_axis in range(3):
        d, m = stair_box(long_axis)
        for axis in range(3):
            if axis != long_axis:
                for flags in (0, FROM_LOW):
                    out.append(case(f"stairs long {long_axis} axis {axis} flags {flags}", (-150, -2, 40), d, m, None, None, axis, flags))
    return out


def planted_noise_case(axis, flags):
    """The noise box over a region off the brick grid, with three columns planted: one filled in the region's first cell along the axis, one
    in its last, one empty."""
    d, m = (a.copy() for a in noise(0.3, seed=5))
    lo, hi = (-4, -2, -1), (6, 6, 4)
    l, h = local_region(d.shape, NOISE_ORIGIN, lo, hi)
    col = np.moveaxis(d, 2 - axis, -1)              # [q][p][along], box-local
    p, q = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    col[l[q], l[p], :] = 0.0
    col[l[q], l[p], l[axis]] = 2.0
    col[l[q], l[p] + 1, :] = 0.0
    col[l[q], l[p] + 1, h[axis] - 1] = 2.0
    col[l[q] + 1, l[p], :] = 0.0
    # filled cells just outside the region along the axis must not be seen
    col[l[q] + 1, l[p], l[axis] - 1] = 1.0
    col[l[q] + 1, l[p], h[axis]] = 1.0
    return case(f"planted noise axis {axis} flags {flags}", NOISE_ORIGIN, d, m, lo, hi, axis, flags, hard=True)


def hard_cases():
    return [c for c in seam_cases() if c["hard"]] + [planted_noise_case(axis, flags) for axis in range(3) for flags in (0, FROM_LOW)]


def limit_case(which, axis, flags):
    from tests import limit_cases as LC
    rng = np.random.default_rng(21)
    nx, ny, nz = LC.DISTANCE_SHAPE
    d = (rng.random((nz, ny, nx)) < 0.08).astype(np.float32) * np.float32(1.5)
    d[0, 0, 0] = d[-1, -1, -1] = 1.0               # the box's corners, on the lattice's ends
    m = rng.integers(1, 250, d.shape).astype(np.uint32)
    return case(f"limit {which} axis {axis} flags {flags}", LC.limit_origin(which, LC.DISTANCE_SHAPE), d, m, None, None, axis, flags)


# ---- the long boxes: a surface in closed form ----------------------------------------------------------------------------------------------
def long_cells(box, u, v):
    """The filled cells of column (u, v) of a LongBox along its long axis: none where (u + v) % 5 == 0, both ends at (1, 0), else two."""
    n = box.length
    if (u, v) == (1, 0):
        return [0, n - 1]
    if (u + v) % 5 == 0:
        return []
    return sorted({(37 * u + 101 * v + 5) * 13 % n, n - 1 - (53 * u + 211 * v) * 29 % (n // 2)})


def long_fill(box):
    d, m = box.zeros(np.float32), box.zeros(np.uint32)
    m[...] = 77                                    # ids under empty cells
    for u in range(box.nu):
        for v in range(box.nv):
            for t in long_cells(box, u, v):
                box.column(d, u, v)[t] = 1.0
                box.column(m, u, v)[t] = 1 + (7 * t + u) % 200
    return d, m


def long_expected(box, flags):
    """(top, material) of the field of the whole LongBox along its long axis, from long_cells alone."""
    p, q = (1 if box.axis == 0 else 0), (1 if box.axis == 2 else 2)
    ext = box.shape
    top, material = np.full((ext[q], ext[p]), NONE, np.uint16), np.zeros((ext[q], ext[p]), np.uint32)
    for u in range(box.nu):
        for v in range(box.nv):
            cells = long_cells(box, u, v)
            if cells:
                c = {box.u_axis: u, box.v_axis: v}
                t = cells[0] if flags & FROM_LOW else cells[-1]
                top[c[q], c[p]], material[c[q], c[p]] = t, 1 + (7 * t + u) % 200
    return top.reshape(-1), material.reshape(-1)


# ---- the scatter scene ---------------------------------------------------------------------------------------------------------------------
SCENE_ORIGIN, SCENE_SHAPE = (-20, -7, 13), (96, 40, 80)
GRASS, SAND, ROCK, SOIL = 1, 2, 3, 9
MAX_RISE, MAX_DROP = 2, 2


def scene():
    """A 96 x 40 x 80 height field: gentle ground of three surface materials, a cliff 9 cells high at x >= 60, a pit down to height 2, an
    overhang (a slab floating at y 30..31) and a strip z in 70..73 with nothing in it."""
    nx, ny, nz = SCENE_SHAPE
    x, z = np.arange(nx)[None, :], np.arange(nz)[:, None]
    h = 14 + (x // 6 + z // 5) % 3 + np.where(x >= 60, 9, 0)
    h = np.where((x >= 20) & (x < 26) & (z >= 30) & (z < 36), 2, h)
    y = np.arange(ny)[None, :, None]
    filled = y <= h[:, None, :]
    filled |= (y >= 30) & (y <= 31) & ((x >= 40) & (x < 46) & (z >= 10) & (z < 16))[:, None, :]
    filled &= ~((z >= 70) & (z < 74))[:, None, :]
    d = np.where(filled, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    d[~filled & ((np.arange(nx)[None, None, :] + y) % 9 == 0)] = np.float32(-0.0)
    d[~filled & ((np.arange(nz)[:, None, None] + y) % 13 == 0)] = np.float32(np.nan)
    surface = np.where(z < 40, GRASS, np.where(x < 30, SAND, ROCK))
    m = np.full((nz, ny, nx), SOIL, np.uint32)
    zi, xi = np.nonzero(np.ones_like(h, dtype=bool))
    m[zi, h[zi, xi], xi] = np.broadcast_to(surface, h.shape)[zi, xi]
    m[(y >= 30) & np.broadcast_to(filled, m.shape)] = ROCK
    return np.ascontiguousarray(d), np.ascontiguousarray(m)


ENTRIES3 = [(0, 5, (0, 0, 0), 0), (1, 2, (1, 0, 2), 1), (0, 1, (-1, 2, 0), -2)]      # (model, weight, anchor, sink); the GPU tests set the model ids


def scene_params(**kw):
    """The main parameter set over the scene: every one of the five tests rejects some candidate."""
    o = SCENE_ORIGIN
    base = dict(flags=ROTATE | MIRROR, cell_log2=0, probability=30000, surface_material=GRASS, min_y=o[1] + 10, max_y=o[1] + 20, radius=3, max_rise=MAX_RISE,
                max_drop=MAX_DROP)
    base.update(kw)
    return params(**base)


def main_scatter_cases():
    """[(name, lo, hi, params, entries)]: the cases on which test_columns_cpu.py asserts the hardness properties."""
    o = SCENE_ORIGIN
    return [("cells of 1", None, None, scene_params(), entries(ENTRIES3)),
            ("cells of 4, off the cell grid", (o[0] + 1, o[1], o[2] + 2), (o[0] + 95, o[1] + 40, o[2] + 79), scene_params(cell_log2=1, probability=50000, radius=2),
             entries(ENTRIES3))]


def sweep_scatter_cases():
    """cell_log2 x radius x probability over the whole scene and over a region off the cell grid; 1 and 16 entries."""
    o = SCENE_ORIGIN
    off = ((o[0] + 3, o[1] + 2, o[2] + 5), (o[0] + 90, o[1] + 38, o[2] + 77))
    out = []
    for c in (0, 2, 5):
        for radius in (0, 3, 8):
            for probability in (0, 30000, 65536):
                lo, hi = off if (c + radius + probability) % 2 else (None, None)
                out.append((f"c {c} radius {radius} p {probability}", lo, hi, scene_params(cell_log2=c, radius=radius, probability=probability), entries(ENTRIES3)))
    out.append(("1 entry", None, None, scene_params(), entries(ENTRIES3[:1])))
    sixteen = [(k % 2, 1 + 4000 * k, (k % 3 - 1, k % 2, 1 - k % 3), k % 4 - 1) for k in range(16)]
    out.append(("16 entries", *off, scene_params(flags=ROTATE), entries(sixteen)))
    out.append(("any material, no limits", None, None, scene_params(flags=ANY_MATERIAL | MIRROR, max_rise=NO_LIMIT, max_drop=NO_LIMIT, radius=8), entries(ENTRIES3)))
    out.append(("rise only", None, None, scene_params(max_drop=NO_LIMIT, max_rise=0, radius=1), entries(ENTRIES3)))
    out.append(("drop only", None, None, scene_params(max_rise=NO_LIMIT, max_drop=0, radius=1), entries(ENTRIES3)))
    return out
