"""Independent reference of blok_hip_volume_label_components / blok_components_label (include/blok_hip.h), written from the contract with
numpy: a restatement of "the label of a component is the smallest index among its voxels", not of the product's union-find.  Labels come
from repeated minimum-propagation over the six shifts until nothing changes; records from np.unique, bincount and per-label minima and
maxima.  Also the shared shapes of the CPU and GPU tests.

Arrays are [z][y][x] over the whole box, whose voxel (0, 0, 0) sits at world `origin`; regions are world voxels, half open."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi
from tests.distance_reference import moved

EMPTY = 0xFFFFFFFF


def region_slices(shape_zyx, origin, lo, hi):
    nz, ny, nx = shape_zyx
    if lo is None:
        lo, hi = tuple(origin), (origin[0] + nx, origin[1] + ny, origin[2] + nz)
    l = [int(lo[a]) - int(origin[a]) for a in range(3)]
    h = [int(hi[a]) - int(origin[a]) for a in range(3)]
    assert all(0 <= l[a] <= h[a] <= (nx, ny, nz)[a] for a in range(3))
    return tuple(int(c) for c in lo), tuple(int(c) for c in hi), (slice(l[2], h[2]), slice(l[1], h[1]), slice(l[0], h[0]))


def label(density, origin=(0, 0, 0), lo=None, hi=None):
    """(labels, records): the label array of the region's cells in index order (uint32) and the COMPONENT records sorted by label."""
    lo, hi, sl = region_slices(density.shape, origin, lo, hi)
    with np.errstate(invalid="ignore"):
        filled = np.asarray(density)[sl] > 0                   # NaN > 0 is False
    rz, ry, rx = filled.shape
    n = rz * ry * rx
    big = np.int64(1) << 40
    lab = np.where(filled, np.arange(n, dtype=np.int64).reshape(filled.shape), big)
    while n:
        new = lab.copy()
        for axis in range(3):
            for step in (1, -1):
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[axis] = slice(0, -1) if step == 1 else slice(1, None)
                dst[axis] = slice(1, None) if step == 1 else slice(0, -1)
                np.minimum(new[tuple(dst)], lab[tuple(src)], out=new[tuple(dst)])
        new[~filled] = big
        if (new == lab).all():
            break
        lab = new
    flat = lab.reshape(-1)
    labels = np.where(flat == big, EMPTY, flat).astype(np.uint32)
    roots, inverse, counts = np.unique(flat[flat != big], return_inverse=True, return_counts=True)
    records = np.zeros(len(roots), dtype=_ffi.COMPONENT)
    if len(roots):
        z, y, x = np.nonzero(filled)
        records["label"] = roots
        records["n_voxels"] = counts
        touches = np.zeros(len(roots), dtype=np.uint32)
        for a, (c, ext) in enumerate(((x, rx), (y, ry), (z, rz))):
            mn = np.full(len(roots), 1 << 40, dtype=np.int64)
            mx = np.full(len(roots), -1, dtype=np.int64)
            np.minimum.at(mn, inverse, c)
            np.maximum.at(mx, inverse, c)
            records["lo"][:, a] = mn + lo[a]
            records["hi"][:, a] = mx + 1 + lo[a]
            touches |= (mx == ext - 1).astype(np.uint32) << (2 * a)
            touches |= (mn == 0).astype(np.uint32) << (2 * a + 1)
        records["touches"] = touches
    return labels, records


def members(density, material_ids, origin, labels, record):
    """The list blok_hip_volume_capture_component is defined by: {(w - rec.lo, ids[w]) : label[w] == label, density[w] > 0} over the
    CURRENT arrays, for a label array of the region (lo, hi) given as (labels, lo, hi).  x fastest, as blok_capture_voxels lists."""
    lab, lo, hi = labels
    lo, hi, sl = region_slices(density.shape, origin, lo, hi)
    with np.errstate(invalid="ignore"):
        mask = (lab.reshape(density[sl].shape) == record["label"]) & (np.asarray(density)[sl] > 0)
    z, y, x = np.nonzero(mask)
    xyz = np.stack([x + lo[0] - record["lo"][0], y + lo[1] - record["lo"][1], z + lo[2] - record["lo"][2]], axis=1).astype(np.int32)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(material_ids[sl][mask].astype(np.uint32)), mask


def clear_members(density, material_ids, origin, labels, record):
    """BLOK_COMPONENT_CUT on the reference arrays."""
    lab, lo, hi = labels
    _, _, mask = members(density, material_ids, origin, labels, record)
    _, _, sl = region_slices(density.shape, origin, lo, hi)
    density[sl][mask] = 0.0
    material_ids[sl][mask] = 0


# ---- shapes shared by the CPU and GPU tests -----------------------------------------------------------------------------------------

ORIGIN, SHAPE = (-40, -44, -24), (96, 80, 64)                  # the box of the GPU cases: (nx, ny, nz) at ORIGIN


def empty_box(shape_xyz=SHAPE):
    nx, ny, nz = shape_xyz
    return np.zeros((nz, ny, nx), dtype=np.float32), np.zeros((nz, ny, nx), dtype=np.uint32)


def put(d, m, voxels, value=1.0):
    """Box-local (x, y, z) voxels filled; the id is a function of the position, so a wrong voxel shows in a captured model."""
    for x, y, z in voxels:
        d[z, y, x] = value
        m[z, y, x] = 1 + (x * 7 + y * 13 + z * 29) % 200


def border_cases():
    """Box-local pieces of two voxels in the box SHAPE, as (voxels, components the piece must form): bars across each of the six brick
    faces at brick, 16- and 64-voxel boundaries (in the keyed layout the brick index jumps there), the same with a one-voxel gap, and pairs
    touching only by an edge or a corner across a brick border.  Pieces keep at least two empty voxels between each other: bars along x at
    z = 2, bars along y at x = 2, bars along z at x >= 70, the diagonal pairs around z = 59."""
    pieces = []
    k = [0, 0, 0]
    for axis in range(3):
        for boundary in (4, 8, 16, 32, 48, 64):
            if boundary + 2 > SHAPE[axis]:
                continue
            for gap in (0, 1):
                site = {0: (0, 2 + 3 * k[0], 2), 1: (2, 0, 8 + 3 * k[1]), 2: (70 + 3 * (k[2] % 4), 50 + 3 * (k[2] // 4), 0)}[axis]
                a, b = list(site), list(site)
                a[axis], b[axis] = boundary - 1, boundary + gap
                pieces.append(([tuple(a), tuple(b)], 1 + gap))
                k[axis] += 1
    for i, (dx, dy, dz) in enumerate(((1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 0), (1, -1, -1))):
        for bx in (8, 16):
            by = 8 * (1 + i)
            a = (bx - 1, by - 1 if dy >= 0 else by, 60 if dz < 0 else 59)
            pieces.append(([a, (a[0] + dx, a[1] + dy, a[2] + dz)], 2))
    # one voxel at (3, 3, 1) of its brick, bit 31 of the mask, under an empty upper half: a mask handled as two signed 32-bit halves
    # would spill into the upper one
    pieces.append(([(43, 75, 5)], 1))
    return pieces


def boustrophedon(ext):
    """One path, one voxel thick, through every second row and layer of a region of extents ext (x, y, z): rows along x joined at
    alternating ends, layers joined at alternating ends.  Region-local voxels in path order; the first is (0, 0, 0), the lowest index."""
    ex, ey, ez = ext
    path = []
    forward_y, forward_x = True, True
    for z in range(0, ez, 2):
        ys = list(range(0, ey, 2))
        if not forward_y:
            ys.reverse()
        for yi, y in enumerate(ys):
            xs = list(range(ex)) if forward_x else list(range(ex - 1, -1, -1))
            path += [(x, y, z) for x in xs]
            if yi + 1 < len(ys):
                path.append((xs[-1], (y + ys[yi + 1]) // 2, z))
            forward_x = not forward_x
        if z + 2 < ez:
            path.append((path[-1][0], path[-1][1], z + 1))
        forward_y = not forward_y
    return path


def boustrophedon_from_the_middle(ext):
    """Two such paths side by side along x, one voxel column apart, joined through their first voxels: the lowest index, (0, 0, 0), lies
    in the middle of the path instead of at one end."""
    ex, ey, ez = ext
    half = ex // 2
    left = boustrophedon((half, ey, ez))
    right = [(x + half + 1, y, z) for x, y, z in boustrophedon((ex - half - 1, ey, ez))]
    return left[::-1] + [(half, 0, 0)] + right


def comb(n_arms, arm_length, pitch=4):
    """A comb whose back lies FAR from the lowest index: arms along +y, `pitch` apart in x, joined only by a back at their far end, one
    voxel thick.  With pitch 4 every arm starts in a brick of its own, so each arm has its own in-brick minimum and its own tree before
    the back joins them; with two arms it is a "U".  Region-local voxels."""
    voxels = []
    for k in range(n_arms):
        voxels += [(k * pitch, y, 0) for y in range(arm_length)]
    voxels += [(x, arm_length, 0) for x in range((n_arms - 1) * pitch + 1)]
    return voxels


# ---- the cases of the GPU tests, which the host build is checked on as well: name -> (density, ids, region lo, region hi), world regions
# in the box SHAPE at ORIGIN (None, None = the whole box).  Built once; nothing changes them.

RAGGED_LO, RAGGED_EXT = (3, 5, 2), (53, 41, 37)                # box-local: a corner that is (3, 1, 2) mod 4, extents no multiple of 4 or 64
PATH_LO, PATH_EXT = (7, 9, 6), (40, 24, 24)
CHECKER_LO, SOLID_LO, SOLID_EXT = (11, 6, 9), (5, 3, 2), (70, 50, 40)
RANDOM_LO, RANDOM_EXT = (27, 17, 10), (40, 36, 44)
RANDOM_P = (0.15, 0.3116, 0.5)
N_ARMS = 9


def world(local, ext=None):
    lo = tuple(ORIGIN[a] + local[a] for a in range(3))
    return lo if ext is None else (lo, tuple(lo[a] + ext[a] for a in range(3)))


def shifted(voxels, by):
    return [(x + by[0], y + by[1], z + by[2]) for x, y, z in voxels]


def prior_with_empties(shape_xyz=SHAPE, seed=3, thin=False):
    """Sparse random content (a tenth filled) plus negative and NaN densities, as the stamp and quad tests build theirs; thin: fewer of
    them (one cell in 91 instead of one in 17), so that a fill at the percolation threshold still percolates."""
    rng = np.random.default_rng(seed)
    shape = tuple(shape_xyz)[::-1]
    d = np.where(rng.random(shape) < 0.1, rng.uniform(0.1, 2.0, shape), 0.0).astype(np.float32)
    m = np.where(d > 0, rng.integers(5, 9, shape), 0).astype(np.uint32)
    if thin:
        d[::5, ::4, ::7] = -0.5
        d[1::7, ::5, ::6] = np.nan
    else:
        d[::3, ::2, ::5] = -0.5
        d[1::7, ::3, ::2] = np.nan
    return np.ascontiguousarray(d), np.ascontiguousarray(m)


_cases = {}


def cases(origin=ORIGIN):
    """The cases over the box SHAPE at `origin`: the same arrays, the regions translated with the box."""
    origin = tuple(origin)
    if origin in _cases:
        return _cases[origin]
    if origin != ORIGIN:                                        # the arrays are box-local: shared with the box at ORIGIN, the regions moved
        _cases[origin] = {name: (d, m, *moved([(lo, hi)], origin, ORIGIN)[0]) for name, (d, m, lo, hi) in cases().items()}
        return _cases[origin]
    from tests.conftest import SEED
    out = {}
    d, m = empty_box()
    for voxels, _ in border_cases():
        put(d, m, voxels)
    out["brick borders"] = (d, m, None, None)
    d, m = prior_with_empties()
    m[(d > 0.9) & (d < 1.4)] = 0                                # a filled voxel with id 0 is a filled voxel
    d[20:30, 20:40, 30:60] = np.where(d[20:30, 20:40, 30:60] > 0, d[20:30, 20:40, 30:60], 0.25)      # and a lump, so not every piece is small
    out["ragged region"] = (d, m, *world(RAGGED_LO, RAGGED_EXT))
    out["whole box"] = (d, m, None, None)
    z, y, x = (int(v[0]) for v in np.nonzero(d > 0))
    out["one voxel"] = (d, m, *world((x, y, z), (1, 1, 1)))
    z, y, x = (int(v[0]) for v in np.nonzero(~(d > 0)))
    out["one empty voxel"] = (d, m, *world((x, y, z), (1, 1, 1)))
    out["empty region"] = (d, m, *world((9, 9, 9), (5, 0, 7)))
    d, m = empty_box()
    d[:, :, :] = 1.0; m[:, :, :] = 3
    out["a brick's interior"] = (d, m, *world((9, 5, 13), (2, 2, 2)))
    # pieces inside the region that only voxels directly outside each of its six sides would join, lying in each outer layer
    d, m = empty_box()
    lo, ext = (13, 10, 7), (18, 15, 21)
    hi = tuple(lo[a] + ext[a] for a in range(3))
    for axis in range(3):
        for side, layer, beyond in ((0, lo[axis], lo[axis] - 1), (1, hi[axis] - 1, hi[axis])):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            for k in (0, 2):                                   # two voxels in the outer layer, one apart, and the bridge beyond it
                p = [0, 0, 0]
                p[axis], p[u], p[v] = layer, lo[u] + 4 + k + 3 * side, lo[v] + 5 + 6 * side
                put(d, m, [tuple(p)])
                p[axis] = beyond
                put(d, m, [tuple(p)])
            p[u] -= 1
            put(d, m, [tuple(p)])
    out["bridges outside the region"] = (d, m, *world(lo, ext))
    for name, path in (("path from one end", boustrophedon(PATH_EXT)), ("path from the middle", boustrophedon_from_the_middle(PATH_EXT))):
        d, m = empty_box()
        put(d, m, shifted(path, PATH_LO))
        out[name] = (d, m, *world(PATH_LO, PATH_EXT))
    d, m = empty_box()
    put(d, m, shifted(comb(2, 30), (10, 8, 5)))               # a "U"
    put(d, m, shifted(comb(N_ARMS, 41), (20, 12, 30)))
    put(d, m, shifted([(y, x, z) for x, y, z in comb(N_ARMS, 41, pitch=8)], (9, 4, 50)))      # arms along x: rows of 64 indices run along them
    out["combs"] = (d, m, None, None)
    d, m = empty_box()
    zz, yy, xx = np.indices(d.shape)
    d[(xx + yy + zz) % 2 == 0] = 0.5
    m[d > 0] = 9
    out["checkerboard"] = (d, m, *world(CHECKER_LO, (32, 32, 32)))
    d, m = empty_box()
    s = tuple(slice(SOLID_LO[a], SOLID_LO[a] + SOLID_EXT[a]) for a in (2, 1, 0))
    d[s] = 2.0; m[s] = 4
    out["solid box"] = (d, m, None, None)
    out["empty volume"] = (*empty_box(), None, None)
    d, m = empty_box()
    d[::2] = -1.0; d[1::4, ::3] = np.nan; d[3::4, 1::2] = -0.0
    m[:] = 6
    out["nothing filled"] = (d, m, None, None)
    for p in RANDOM_P:
        d, m = prior_with_empties(seed=5, thin=True)
        d[np.isfinite(d) & (d == 0)] = 1.0                      # the larger box around the region is filled, but for the NaN and negative cells
        m[d > 0] = 2
        rng = np.random.default_rng(SEED + int(p * 10000))
        s = tuple(slice(RANDOM_LO[a], RANDOM_LO[a] + RANDOM_EXT[a]) for a in (2, 1, 0))
        fill = rng.random(d[s].shape) < p
        with np.errstate(invalid="ignore"):
            keep_empty = ~(d[s] >= 0)                           # NaN and negative cells stay as they are
        d[s] = np.where(keep_empty, d[s], np.where(fill, rng.uniform(0.1, 2.0, fill.shape), 0.0)).astype(np.float32)
        m[s] = np.where(d[s] > 0, rng.integers(1, 250, fill.shape), 0)
        d[s][0, 0, 0], m[s][0, 0, 0] = 1.0, 77                  # the region's lowest corner cell is filled: some component touches the corner
        out[f"random {p}"] = (np.ascontiguousarray(d), np.ascontiguousarray(m), *world(RANDOM_LO, RANDOM_EXT))
    _cases[origin] = out
    return out


_expected = {}


def expected(name, origin=ORIGIN):
    """The reference's (labels, records) of a case over the box at `origin`, computed once."""
    key = (name, tuple(origin))
    if key not in _expected:
        d, _, lo, hi = cases(origin)[name]
        _expected[key] = label(d, origin, lo, hi)
    return _expected[key]
