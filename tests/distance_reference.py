"""The contract of blok_hip_volume_distance_field / blok_hip_volume_edit_by_distance (include/blok_hip.h) restated in numpy — TESTS ONLY, no
product library.  `field_brute` is the definition (a minimum over every offset of the ball), `field` the separable form the builders
use, on an array padded with the outside state; tests/test_distance_cpu.py pins one to the other and both to hand-written cases.
`single_source` is the closed form for a lone source, for boxes too large for either.  Arrays are [z][y][x]; regions are world voxels,
half open, both None = the whole box."""
from __future__ import annotations

import itertools

import numpy as np

TO_EMPTY, BOX_IS_SOLID = 1, 2
FAR = 0xFFFF
GROW, SHRINK, HOLLOW = 0, 1, 2
ALL_FLAGS = (0, TO_EMPTY, BOX_IS_SOLID, TO_EMPTY | BOX_IS_SOLID)
INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("max_radius", "<u4"), ("reserved", "<u4"),
                 ("n_zero", "<u8"), ("n_near", "<u8"), ("n_far", "<u8")])


def region_of(shape_zyx, origin, lo, hi):
    """Box-local (lo, ext) of a world region."""
    nz, ny, nx = shape_zyx
    if lo is None and hi is None:
        return (0, 0, 0), (nx, ny, nz)
    l = tuple(int(lo[a]) - int(origin[a]) for a in range(3))
    e = tuple(int(hi[a]) - int(lo[a]) for a in range(3))
    assert all(v >= 0 for v in l + e) and all(l[a] + e[a] <= (nx, ny, nz)[a] for a in range(3)), "the region lies in the box"
    return l, e


def sources_padded(d, flags, pad, lo, ext):
    """Bool [z][y][x]: the sources over the region widened by `pad` on every side; cells outside the box carry the outside state."""
    filled = np.asarray(d, dtype=np.float32) > 0                  # NaN, zeros of either sign and negative densities are empty
    nz, ny, nx = filled.shape
    state = np.full((ext[2] + 2 * pad, ext[1] + 2 * pad, ext[0] + 2 * pad), bool(flags & BOX_IS_SOLID))
    # the part of the box that the widened region covers
    src, dst = [], []
    for a, n in ((2, nz), (1, ny), (0, nx)):
        w0 = lo[a] - pad                                          # box coordinate of the window's first cell
        b0, b1 = max(w0, 0), min(w0 + ext[a] + 2 * pad, n)
        src.append(slice(b0, max(b1, b0))); dst.append(slice(b0 - w0, max(b1, b0) - w0))
    state[tuple(dst)] = filled[tuple(src)]
    return ~state if flags & TO_EMPTY else state


def make_info(origin, lo, ext, R, flags, dist):
    info = np.zeros(1, dtype=INFO)
    info["version"], info["flags"], info["max_radius"] = 1, flags, R
    info["lo"][0] = [int(origin[a]) + lo[a] for a in range(3)]
    info["ext"][0] = ext
    info["n_zero"] = int((dist == 0).sum())
    info["n_far"] = int((dist == FAR).sum())
    info["n_near"] = dist.size - int(info["n_zero"][0]) - int(info["n_far"][0])
    return info


def field_brute(d, origin, lo, hi, R, flags):
    """The definition: D(c) = the least |v|^2 <= R^2 over the offsets v of the ball with c + v a source, FAR when there is none."""
    lo, ext = region_of(np.shape(d), origin, lo, hi)
    src = sources_padded(d, flags, R, lo, ext)
    out = np.full((ext[2], ext[1], ext[0]), FAR, np.uint32)
    for dz, dy, dx in itertools.product(range(-R, R + 1), repeat=3):
        d2 = dx * dx + dy * dy + dz * dz
        if d2 > R * R:
            continue
        s = src[R + dz:R + dz + ext[2], R + dy:R + dy + ext[1], R + dx:R + dx + ext[0]]
        out = np.where(s, np.minimum(out, d2), out)
    out = out.astype(np.uint16)
    return out, make_info(origin, lo, ext, R, flags, out)


def field(d, origin, lo, hi, R, flags, pad=None):
    """The separable model: three capped min-plus passes over the region padded by 2 R + 2 with the outside state (a shift brings FAR in
    at the array's end; with that much padding it never reaches the region).  pad = 0 is allowed for the whole box with flags 0 alone:
    there the outside holds no source, which is what FAR says, so a long thin box needs no padding R cells wide on every side."""
    whole = lo is None and hi is None
    lo, ext = region_of(np.shape(d), origin, lo, hi)
    assert pad is None or (pad == 0 and whole and flags == 0)
    pad = 2 * R + 2 if pad is None else pad
    g = np.where(sources_padded(d, flags, pad, lo, ext), 0, FAR).astype(np.int32)
    for ax in (2, 1, 0):
        best = np.full(g.shape, FAR, np.int32)                    # (what a shift leaves uncovered at the array's end stays FAR)
        n = g.shape[ax]
        for k in range(-R, R + 1):
            if abs(k) >= n:                                       # (only without padding: a shift by the whole extent covers nothing)
                continue
            sl, dl = [slice(None)] * 3, [slice(None)] * 3
            if k >= 0:
                sl[ax], dl[ax] = slice(k, n), slice(0, n - k)
            else:
                sl[ax], dl[ax] = slice(0, n + k), slice(-k, n)
            c = g[tuple(sl)] + k * k                              # best(i) takes g(i + k) + k^2 ...
            c[c > R * R] = FAR                                    # ... capped: FAR + k^2 is above R^2 <= 65025 too
            np.minimum(best[tuple(dl)], c, out=best[tuple(dl)])
        g = best
    out = g[pad:pad + ext[2], pad:pad + ext[1], pad:pad + ext[0]].astype(np.uint16)
    return out, make_info(origin, lo, ext, R, flags, out)


def single_source(shape_xyz, s, R):
    """[z][y][x] over a box of `shape_xyz` with the one source s = (x, y, z), box-local (it may lie anywhere, also outside a region cut
    from the result): dx^2 + dy^2 + dz^2, FAR above R^2.  To-filled, outside empty."""
    return from_sources(shape_xyz, [s], R)


def from_sources(shape_xyz, sources, R):
    """The same for a handful of sources: the minimum of their closed forms."""
    nx, ny, nz = shape_xyz
    x, y, z = np.arange(nx, dtype=np.int64)[None, None, :], np.arange(ny, dtype=np.int64)[None, :, None], np.arange(nz, dtype=np.int64)[:, None, None]
    out = np.full((nz, ny, nx), FAR, np.int64)
    for s in sources:
        out = np.minimum(out, (x - s[0]) ** 2 + (y - s[1]) ** 2 + (z - s[2]) ** 2)
    return np.where(out > R * R, FAR, out).astype(np.uint16)


def edit(d, m, dist, info, op, d2, density=1.0, material=0, origin=(0, 0, 0)):
    """Applies an edit to the [z][y][x] arrays of a box at world `origin`, in place, judged against them as they are NOW; returns the number
    of cells written."""
    flags, R = int(info["flags"][0]), int(info["max_radius"][0])
    assert op in (GROW, SHRINK, HOLLOW) and bool(flags & TO_EMPTY) == (op != GROW) and d2 <= R * R
    ext = [int(v) for v in info["ext"][0]]
    if 0 in ext:
        return 0
    l = [int(info["lo"][0][a]) - int(origin[a]) for a in range(3)]
    sl = (slice(l[2], l[2] + ext[2]), slice(l[1], l[1] + ext[1]), slice(l[0], l[0] + ext[0]))
    dist = np.asarray(dist).reshape(ext[2], ext[1], ext[0]).astype(np.int64)
    now = d[sl] > 0
    if op == GROW:
        w = (dist >= 1) & (dist <= d2) & ~now
    elif op == SHRINK:
        w = (dist >= 1) & (dist <= d2) & now
    else:
        w = (dist > d2) & now
    d[sl] = np.where(w, np.float32(density if op == GROW else 0.0), d[sl])
    m[sl] = np.where(w, np.uint32(material if op == GROW else 0), m[sl])
    return int(w.sum())


# ---- the shapes the GPU tests use (tests/test_distance_gpu.py), pinned on the CPU in tests/test_distance_cpu.py --------------------------------
NOISE_ORIGIN, NOISE_SHAPE = (-5, -3, -2), (13, 10, 7)
NOISE_REGIONS = [(None, None), ((-4, -1, -2), (7, 4, 5)), ((-2, -3, -1), (3, 7, 2)), ((0, 1, 1), (1, 2, 2))]
NOISE_RADII = (0, 1, 3, 4, 5)


def noise(fill=0.01, seed=5):
    """Sparse by default, so that every radius up to 5 leaves FAR cells and pairs at exactly R^2 (tests/test_distance_cpu.py asserts it)."""
    rng = np.random.default_rng(seed)
    s = NOISE_SHAPE[::-1]
    d = np.where(rng.random(s) < fill, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    d[rng.random(s) < 0.05] = -1.0
    d[rng.random(s) < 0.03] = np.nan
    d[rng.random(s) < 0.03] = -0.0
    return d, np.where(d > 0, 2, 0).astype(np.uint32)


SCENE_ORIGIN, SCENE_SHAPE = (3, -8, 10), (40, 36, 33)
# regions that touch each face of the box and one strictly inside; ends off and on the 4- and 16-voxel grid
_SCENE_REGIONS = [(None, None), ((3, -8, 10), (20, 9, 27)), ((26, 8, 23), (43, 28, 43)), ((8, -3, 15), (37, 21, 38)), ((7, -4, 14), (19, 8, 30))]
SCENE_RADII = (8, 16)


def moved(regions, origin, base=None):
    """World regions [(lo, hi)] given for a box at `base` (default SCENE_ORIGIN) as the same box-local cells of the box at `origin`; a
    None corner stays None.  The one helper by which the reference modules move their case tables with a box."""
    base = SCENE_ORIGIN if base is None else base
    move = lambda c: None if c is None else tuple(c[a] - base[a] + origin[a] for a in range(3))
    return [(move(lo), move(hi)) for lo, hi in regions]


def scene_regions(origin=SCENE_ORIGIN):
    return moved(_SCENE_REGIONS, origin)


SCENE_REGIONS = scene_regions()


def scene(seed=11):
    """A block, a plate, a diagonal staircase and scattered voxels."""
    nx, ny, nz = SCENE_SHAPE
    d = np.zeros((nz, ny, nx), np.float32)
    m = np.zeros((nz, ny, nx), np.uint32)
    d[1:19, 1:19, 1:19] = 1.0; m[1:19, 1:19, 1:19] = 1              # the block, 18^3: its 2^3 middle cells are 9 from empty space
    d[24:26, 2:21, 1:26] = 0.5; m[24:26, 2:21, 1:26] = 2            # the plate, two cells thick
    for k in range(12):                                             # the staircase, out of the block towards the far corner (which stays far from everything)
        d[18 + k, 6 + k:9 + k, 14 + k:16 + k] = 1.5; m[18 + k, 6 + k:9 + k, 14 + k:16 + k] = 3
    rng = np.random.default_rng(seed)
    dots = rng.random(d.shape) < 0.0008
    dots[14:, 18:, 22:] = False
    dots[1:19, 1:19, 1:19] = False
    d[dots] = 2.0; m[dots] = 4
    d[0, 0, 0] = 1.0; m[0, 0, 0] = 4                                # a corner of the box
    d[(d <= 0) & (rng.random(d.shape) < 0.01)] = -1.0               # empty cells that are not zero
    m[(d <= 0) & (rng.random(d.shape) < 0.01)] = 9                  # ids left behind under empty cells
    return d, m


_scene_fields = {}


def scene_cases(origin=SCENE_ORIGIN):
    """(lo, hi, R, flags) over the scene in the box at `origin`: the whole box in all four flag combinations, each region in one of them,
    the far corner in two."""
    regions = scene_regions(origin)
    cases = [(None, None, radius, flags) for radius in SCENE_RADII for flags in ALL_FLAGS]
    for i, (lo, hi) in enumerate(regions[1:], 1):
        cases += [(lo, hi, radius, ALL_FLAGS[i % 4]) for radius in SCENE_RADII]
    return cases + [(*regions[2], radius, 0) for radius in SCENE_RADII]


def scene_field(lo, hi, R, flags, origin=SCENE_ORIGIN):
    """The model's field over the scene in the box at `origin`, computed once per case (the scene is never changed)."""
    key = (lo, hi, R, flags, tuple(origin))
    if key not in _scene_fields:
        _scene_fields[key] = field(scene()[0], origin, lo, hi, R, flags)
    return _scene_fields[key]


LINE_SHAPE = (600, 5, 3)


def line_cases():
    """(name, sources, region) on the 600 x 5 x 3 box, box-local, along x; the tests permute the axes onto y and z.  One source with cells
    255 and 256 away; the same with the source outside the region; sources 63, 64 and 65 apart (the seams of a 64-bit row word and of a
    64-lane wave)."""
    return [("one", [(300, 2, 1)], (None, None)),
            ("outside", [(40, 2, 1)], ((41, 0, 0), (600, 5, 3))),
            ("seams", [(0, 0, 0), (63, 0, 0), (128, 4, 2), (192, 4, 2), (256, 1, 1), (321, 1, 1)], (None, None))]


def permuted(shape, sources, region, axis):
    """The line case with its long axis moved from x onto `axis`."""
    p = {0: (0, 1, 2), 1: (1, 0, 2), 2: (2, 1, 0)}[axis]           # new[a] = old[p[a]]
    t = lambda v: tuple(v[p[a]] for a in range(3))
    return t(shape), [t(s) for s in sources], (None, None) if region[0] is None else (t(region[0]), t(region[1]))


def volume_with(shape_xyz, sources, value=1.0, material=1):
    nx, ny, nz = shape_xyz
    d, m = np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.uint32)
    for x, y, z in sources:
        d[z, y, x], m[z, y, x] = value, material
    return d, m


SEAM_SHAPE = (150, 140, 130)


def seam_sources(row_cells, tile_x, tile_rows, chunk_rows):
    """Eight lone sources next to and across the builder's tile borders (the extents come from blok_amd/distance.py)."""
    assert row_cells < 2 * 150 and tile_x < 150 and 4 * tile_rows <= 130 and chunk_rows < 130
    return [(tile_x - 1, tile_rows - 1, tile_rows - 1), (tile_x, tile_rows, tile_rows), (2 * tile_x - 1, 2 * tile_rows, 3 * tile_rows - 1),
            (2 * tile_x, 3 * tile_rows - 1, 2 * tile_rows), (0, chunk_rows - 1, chunk_rows), (149, chunk_rows, chunk_rows - 1),
            (row_cells // 2 - 1, 139, 0), (row_cells // 2, 0, 129)]
