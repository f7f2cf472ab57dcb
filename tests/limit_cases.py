"""The boxes and closed-form cases of the volume tests at the lattice's limits — TESTS ONLY, numpy alone, no GPU.

Limit boxes: the shapes the feature tests already use, translated so that the box touches the ends of the int16 lattice [-32768, 32768)
(include/blok_hip.h: a box is any [origin, origin + ext) inside it).  The scenes are box-local arrays, so the existing builders serve; the
regions and placements move with the box (the `origin` argument of the reference modules' case tables).

Long boxes: L = 16384 cells on one axis (the largest extent, 7 tree levels, always the general brick layout), a few cells on the other
two, in all three permutations, one flush against each end of the lattice and one across zero.  What fills them is written as a function
of the cell (t, u, v) — t along the long axis, u and v along the two that follow it cyclically — so that what the feature must return is
known in closed form where the iterative references (components_reference.label, distance_reference.field_brute) would take too long;
tests/test_volume_limits_cpu.py pins each closed form to its reference at LENGTH_PINNED cells."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi

LATTICE_LO, LATTICE_HI = -32768, 32768

# ---- limit boxes ------------------------------------------------------------------------------------------------------------------------
SHAPE = (96, 80, 64)                       # stamp, components, sweep, bricks, quads, terrain
DISTANCE_SHAPE = (40, 36, 33)
REBUILD_SHAPE = (70, 37, 130)              # the rebuild's boundary sequence
MIXED_Z = 1001                             # not a multiple of 4
LIMITS = ("LOW", "HIGH", "MIXED")


def limit_origin(which, shape):
    return {"LOW": (LATTICE_LO, LATTICE_LO, LATTICE_LO), "HIGH": tuple(LATTICE_HI - n for n in shape),
            "MIXED": (LATTICE_LO, LATTICE_HI - shape[1], MIXED_Z)}[which]


# (hits, misses) per camera of the rebuild tests' 96 x 64 = 6144 rays, at about 0.7 of what the oracle alone reports for the final states of
# the boundary sequence in the LOW and HIGH boxes (tests/test_volume_limits_cpu.py prints them): (799, 5345) (4520, 1624) (1615, 4529) in
# both — the counts of the same sequence in the box at (-7, 3, -20), since the cameras move with the box and every coordinate near 32768 is
# a float with fraction bits to spare
FRAME_FLOORS = {"LOW": [(560, 3740), (3160, 1135), (1130, 3170)], "HIGH": [(560, 3740), (3160, 1135), (1130, 3170)]}


def box_hi(origin, shape):
    return tuple(o + n for o, n in zip(origin, shape))


# ---- long boxes -------------------------------------------------------------------------------------------------------------------------
L = 16384
LENGTH_PINNED = 600                        # where the closed forms are pinned to the iterative references
EMPTY_LABEL = 0xFFFFFFFF


class LongBox:
    """axis: the long one.  (t, u, v) are the box-local coordinates along axis, axis + 1 and axis + 2 (cyclically)."""

    def __init__(self, name, axis, origin, shape):
        self.name, self.axis, self.origin, self.shape = name, axis, tuple(origin), tuple(shape)
        self.u_axis, self.v_axis = (axis + 1) % 3, (axis + 2) % 3
        self.length, self.nu, self.nv = shape[axis], shape[self.u_axis], shape[self.v_axis]

    def shortened(self, length=LENGTH_PINNED):
        shape = list(self.shape)
        shape[self.axis] = length
        return LongBox(self.name, self.axis, self.origin, shape)

    @property
    def hi(self):
        return box_hi(self.origin, self.shape)

    def cell(self, t, u, v):
        """Box-local (x, y, z) of (t, u, v)."""
        p = [0, 0, 0]
        p[self.axis], p[self.u_axis], p[self.v_axis] = int(t), int(u), int(v)
        return tuple(p)

    def world(self, t, u, v):
        return tuple(o + c for o, c in zip(self.origin, self.cell(t, u, v)))

    def index(self, t, u, v):
        x, y, z = self.cell(t, u, v)
        return x + self.shape[0] * (y + self.shape[1] * z)

    def tuv(self):
        """Open grids (t, u, v) that broadcast to the [z][y][x] array."""
        nx, ny, nz = self.shape
        g = (np.arange(nx, dtype=np.int64)[None, None, :], np.arange(ny, dtype=np.int64)[None, :, None], np.arange(nz, dtype=np.int64)[:, None, None])
        return g[self.axis], g[self.u_axis], g[self.v_axis]

    def zeros(self, dtype):
        return np.zeros(self.shape[::-1], dtype=dtype)

    def column(self, array, u, v):
        """The view of the [z][y][x] array along the long axis at (u, v)."""
        sl = [None, None, None]
        sl[2 - self.axis], sl[2 - self.u_axis], sl[2 - self.v_axis] = slice(None), int(u), int(v)
        return array[tuple(sl)]


# the short extents lie between 3 and 16 and are no multiples of 4; at most 2^21 cells; the long axis on [16384, 32768), on
# [-32768, -16384) and across zero; the short axes touch both ends of the lattice too
LONG_BOXES = [LongBox("along-x", 0, (16384, LATTICE_LO, LATTICE_HI - 13), (L, 7, 13)),
              LongBox("along-y", 1, (LATTICE_HI - 5, LATTICE_LO, -7), (5, L, 14)),
              LongBox("along-z", 2, (-6, 101, -9001), (11, 9, L))]
for _b in LONG_BOXES:
    assert all(3 <= n <= 16 and n % 4 for a, n in enumerate(_b.shape) if a != _b.axis) and int(np.prod(_b.shape)) <= 1 << 21
    assert all(LATTICE_LO <= o and h <= LATTICE_HI for o, h in zip(_b.origin, _b.hi))
LONG_IDS = [b.name for b in LONG_BOXES]


# ---- rebuild: a sparse fill ---------------------------------------------------------------------------------------------------------------
def sparse_fill(box):
    """One cell in 97 filled and the cells u = v of both end layers, densities 0.5, 0.75 and 1.0; empty cells hold -0.0 and NaN here and
    there; every cell an id in 1 .. 250."""
    t, u, v = box.tuv()
    k = 7 * t + 3 * u + 5 * v
    d = np.where((k % 97 == 0) | (((t == 0) | (t == box.length - 1)) & (u == v)), 0.5 + 0.25 * ((t + u) % 3), 0.0).astype(np.float32)
    d = np.where((k % 97 == 1) & (t % 2 == 0), np.float32(-0.0), d)
    d = np.where(k % 97 == 2, np.float32(np.nan), d).astype(np.float32)
    ids = (1 + (t + 11 * u + 17 * v) % 250).astype(np.uint32)
    return np.ascontiguousarray(d), np.ascontiguousarray(np.broadcast_to(ids, d.shape))


def end_brushes(box):
    """[(centre, radius, value, mode, refused)]: brushes whose boxes end exactly on the faces at the far and at the near end of the long
    axis and on the low faces of the short ones (floor(c - r) and floor(c + r) + 1 of float32 sums next to 32768), and one a voxel further."""
    far = [o + 2.5 for o in box.origin]
    far[box.axis] = box.hi[box.axis] - 2.5
    near = [o + 2.5 for o in box.origin]
    return [(tuple(far), 2.49, 1.0, 0, False), (tuple(far), 2.5, 1.0, 0, True), (tuple(near), 2.49, 0.0, 1, False), (tuple(near), 2.51, 0.0, 1, True)]


def end_voxels(box):
    """World voxels at both ends of the long axis and in between, on the faces of the short axes."""
    n = box.length
    return np.array([box.world(0, 0, 0), box.world(n - 1, box.nu - 1, box.nv - 1), box.world(n - 1, 0, box.nv - 1), box.world(0, box.nu - 1, 0),
                     box.world(n // 2, 1, 1), box.world(n - 64, 2, 2), box.world(63, 2, 2)], dtype=np.int32)


# ---- quads ---------------------------------------------------------------------------------------------------------------------------------
SEAM_RUNS = ((0, 63, 1), (63, 64, 2), (64, 65, 3), (65, 70, 4), (72, 128, 5), (128, 129, 6), (-65, -64, 7), (-64, -1, 8), (-1, None, 9))      # [t0, t1) of material; negative: from the end


def quads_fill(box, case):
    """"slab": the layer v = 0 filled with one material: its two large faces are one quad each, `length` cells long.  "seams": one row
    along the long axis at (2, 2) of runs told apart by their material, which start and end at cells 63, 64 and 65 and in the row's last
    word of 64 cells."""
    d, m = box.zeros(np.float32), box.zeros(np.uint32)
    if case == "slab":
        t, u, v = box.tuv()
        d[np.broadcast_to(v == 0, d.shape)] = 1.0
        m[d > 0] = 7
    else:
        col_d, col_m = box.column(d, 2, 2), box.column(m, 2, 2)
        for t0, t1, material in SEAM_RUNS:
            col_d[t0:t1] = 0.5 + material
            col_m[t0:t1] = material
    return d, m


def seam_runs(box):
    """[(first cell, last cell, material)] of the "seams" row, box-local along the long axis."""
    n = box.length
    return [(t0 % n, (n if t1 is None else t1 % n) - 1, material) for t0, t1, material in SEAM_RUNS]


# ---- components ----------------------------------------------------------------------------------------------------------------------------
BAR_AT, BROKEN_AT = (1, 1), (3, 3)                                  # (u, v) of the whole bar and of the broken one
GAPS = (3, 4, 63, 64, 127, 200, 256, 4095, 4096, -64, -5)           # empty cells of the broken bar: next to brick and 64-cell boundaries; negative: from the end


def bar_pieces(box):
    """[(u, v, t0, t1)]: the whole bar, then the pieces the gaps leave of the broken one, half open along the long axis."""
    n = box.length
    gaps = sorted({g % n for g in GAPS if -n <= g < n})
    pieces, start = [(*BAR_AT, 0, n)], 0
    for g in gaps + [n]:
        if g > start:
            pieces.append((*BROKEN_AT, start, g))
        start = g + 1
    return pieces


def components_fill(box):
    d, m = box.zeros(np.float32), box.zeros(np.uint32)
    for u, v, t0, t1 in bar_pieces(box):
        box.column(d, u, v)[t0:t1] = 1.0 + u
        box.column(m, u, v)[t0:t1] = 1 + (np.arange(t0, t1) * 7 + u) % 200      # the id is a function of the position: a wrong voxel shows in a captured model
    return d, m


def components_expected(box):
    """(labels, records) of components_fill over the whole box, in closed form: every piece lies in a column of its own kind, so a piece is
    a component, its label the index of its first cell, its bounds its ends."""
    pieces = bar_pieces(box)
    labels = np.full(box.shape[::-1], EMPTY_LABEL, dtype=np.uint32)
    records = np.zeros(len(pieces), dtype=_ffi.COMPONENT)
    ext = box.shape
    for k, (u, v, t0, t1) in enumerate(pieces):
        box.column(labels, u, v)[t0:t1] = box.index(t0, u, v)
        lo, hi = box.cell(t0, u, v), box.cell(t1 - 1, u, v)
        records[k]["label"], records[k]["n_voxels"] = box.index(t0, u, v), t1 - t0
        records[k]["lo"] = [box.origin[a] + lo[a] for a in range(3)]
        records[k]["hi"] = [box.origin[a] + hi[a] + 1 for a in range(3)]
        records[k]["touches"] = sum(((hi[a] == ext[a] - 1) << (2 * a)) | ((lo[a] == 0) << (2 * a + 1)) for a in range(3))
    return labels.reshape(-1), records[np.argsort(records["label"])]


# ---- sweep ---------------------------------------------------------------------------------------------------------------------------------
FAR = 0xFFFFFFFF
OBSTACLE_AT, CLEAR_AT = (2, 2), (0, 0)                              # (u, v): a column with an obstacle near each end, and one that holds nothing


def sweep_fill(box):
    """Empty but for one filled cell near each end of the column OBSTACLE_AT (cells 2 and length - 3), and empty cells that are not zero."""
    d = box.zeros(np.float32)
    t, u, v = box.tuv()
    d[np.broadcast_to((t + u + v) % 11 == 0, d.shape)] = -1.0
    box.column(d, *CLEAR_AT)[:] = 0.0
    box.column(d, *CLEAR_AT)[5::7] = np.nan
    col = box.column(d, *OBSTACLE_AT)
    col[:] = 0.0
    col[2] = col[box.length - 3] = 1.0
    return d


def sweep_cases(box):
    """[(tag, model name of sweep_reference.models(), placement, direction, max_distance, flags, (n_overlap, travel, blocked))]: a voxel
    that crosses the whole box to the obstacle at the other end, towards + and towards -; one that leaves through the end face of a
    clear column, stopped by nothing or by the wall; the travel as the limit, and one more."""
    from tests.sweep_reference import BOX_IS_SOLID
    n = box.length
    ident = ((0, 1, 2), 0)
    out = []
    for step in (1, -1):
        direction = 2 * box.axis + (step < 0)
        start = 10 if step > 0 else n - 11
        to_obstacle = n - 3 - 10 - 1                                # cells strictly between the start and the obstacle, either way
        place = (box.world(start, *OBSTACLE_AT), *ident)
        for max_distance in (FAR, to_obstacle + 1, to_obstacle, 16000):
            out.append((f"across {step} {max_distance}", "one voxel", place, direction, max_distance, 0,
                        (0, min(to_obstacle, max_distance), int(to_obstacle < max_distance))))
        out.append((f"across {step} solid", "one voxel", place, direction, FAR, BOX_IS_SOLID, (0, to_obstacle, 1)))
        start = 5 if step > 0 else n - 6
        to_wall = n - 1 - 5
        place = (box.world(start, *CLEAR_AT), *ident)
        out.append((f"clear {step}", "one voxel", place, direction, FAR, 0, (0, FAR, 0)))
        out.append((f"clear {step} 20000", "one voxel", place, direction, 20000, 0, (0, 20000, 0)))
        out.append((f"wall {step}", "one voxel", place, direction, FAR, BOX_IS_SOLID, (0, to_wall, 1)))
        out.append((f"wall {step} exact", "one voxel", place, direction, to_wall, BOX_IS_SOLID, (0, to_wall, 0)))
        # from the obstacle itself: the start cell is not looked at
        place = (box.world(2 if step > 0 else n - 3, *OBSTACLE_AT), *ident)
        out.append((f"from the obstacle {step}", "one voxel", place, direction, FAR, 0, (1, n - 3 - 2 - 1, 1)))
    return out


# ---- bricks --------------------------------------------------------------------------------------------------------------------------------
def bricks_fill(box):
    """A stored cell in every brick along the long axis at (1, 1) — length / 4 records in one brick row —, a second one with another
    density and id in every second brick (payload entries), NaN, -0.0 and bare ids at places."""
    d, m = box.zeros(np.float32), box.zeros(np.uint32)
    n = box.length
    t = np.arange(n)
    a, b = box.column(d, 1, 1), box.column(m, 1, 1)
    a[1::4], b[1::4] = 1.0, 5
    a[2::8], b[2::8] = 0.25, 6
    a[t % 64 == 7] = np.nan
    a[t % 128 == 11] = -0.0
    b[t % 64 == 15] = 9                                             # an id under density 0
    a, b = box.column(d, 2, 2), box.column(m, 2, 2)
    a[n - 8:], b[n - 8:] = 1.5, 3                                   # a solid piece in the last two bricks: kind 3 where it is alone
    return d, m


def bricks_regions(box):
    """The whole box; a region that starts one cell off the brick grid on the long axis; one that also ends off it."""
    lo, hi = list(box.origin), list(box.hi)
    off = list(lo); off[box.axis] += 1
    end = list(hi); end[box.axis] -= 2
    return [(None, None), (tuple(off), tuple(hi)), (tuple(off), tuple(end))]


# ---- distance ------------------------------------------------------------------------------------------------------------------------------
def distance_sources(box):
    """Box-local (x, y, z): sources at both ends and in the middle of the long axis, and a pair 64 cells apart across the middle of a
    row word."""
    n = box.length
    return [box.cell(0, 0, 0), box.cell(n - 1, box.nu - 1, box.nv - 1), box.cell(n // 2, 1, 2), box.cell(n // 4 + 31, 2, 0), box.cell(n // 4 + 95, 2, 0)]


def rod_fill(box):
    """A rod of 3 x 3 cells along the whole long axis at u, v in 1 .. 3, cut through at cells 64 .. 66 and near the far end: something with
    an inside for SHRINK and HOLLOW."""
    d, m = box.zeros(np.float32), box.zeros(np.uint32)
    for u in (1, 2, 3):
        for v in (1, 2, 3):
            box.column(d, u, v)[:] = 1.0
            box.column(m, u, v)[:] = 2 + u
            box.column(d, u, v)[64:67] = 0.0
            box.column(d, u, v)[box.length - 9] = -1.0
    m[~(d > 0)] = 0
    return d, m


# ---- voxelize ------------------------------------------------------------------------------------------------------------------------------
SEGMENT = 2000                                                      # cells of a prism's segment along the long axis: a triangle spans at most 2048 voxels


def prism(box):
    """(positions, triangles, (lo, hi) box-local cells the prism's closed cubes meet): a closed box-shaped prism along the whole long axis,
    its faces on half-integer planes, its four long sides cut into segments of SEGMENT cells; no inner walls."""
    n = box.length
    t0, t1 = 1.5, n - 1.5
    u0, u1, v0, v1 = 0.5, box.nu - 1.5, 1.5, box.nv - 0.5
    cuts = [t0] + [float(c) + 0.5 for c in range(SEGMENT, n - 2, SEGMENT)] + [t1]
    pos, tri = [], []

    def vertex(t, u, v):
        p = [0.0, 0.0, 0.0]
        p[box.axis], p[box.u_axis], p[box.v_axis] = t + box.origin[box.axis], u + box.origin[box.u_axis], v + box.origin[box.v_axis]
        pos.append(p)
        return len(pos) - 1

    def quad(a, b, c, d):
        tri.extend([(a, b, c), (a, c, d)])
    rings = [[vertex(t, u0, v0), vertex(t, u1, v0), vertex(t, u1, v1), vertex(t, u0, v1)] for t in cuts]
    for r0, r1 in zip(rings, rings[1:]):
        for k in range(4):
            quad(r0[k], r0[(k + 1) % 4], r1[(k + 1) % 4], r1[k])
    quad(*rings[0][::-1])
    quad(*rings[-1])
    lo = box.cell(1, 0, 1)
    hi = box.cell(n - 2, box.nu - 2, box.nv - 1)
    return np.array(pos, dtype=np.float32), np.array(tri, dtype=np.uint32), (lo, hi)


def prism_expected(box, solid):
    """Filled cells [z][y][x] of the prism in closed form: its faces lie on half-integer planes, so the surface is the outer layer of the
    cells [lo, hi] and the solid is all of them."""
    _, _, (lo, hi) = prism(box)
    f = box.zeros(bool)
    f[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    if not solid:
        f[lo[2] + 1:hi[2], lo[1] + 1:hi[1], lo[0] + 1:hi[0]] = False
    return f


def face_box_mesh(lo, hi):
    """A closed box with its faces exactly on the integer planes lo and hi (world), 12 triangles, outward normals."""
    c = [(x, y, z) for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])]
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    tri = [t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))]
    return np.array(c, dtype=np.float32), np.array(tri, dtype=np.uint32)


# ---- what the limit boxes need beyond their translated scenes ------------------------------------------------------------------------------
def faces_filled(density):
    """Per face 0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z: the outermost layer of the [z][y][x] array holds a filled cell."""
    with np.errstate(invalid="ignore"):
        f = np.asarray(density) > 0
    return [bool(f[:, :, -1].any()), bool(f[:, :, 0].any()), bool(f[:, -1, :].any()), bool(f[:, 0, :].any()), bool(f[-1].any()), bool(f[0].any())]


def distance_scene():
    """distance_reference.scene() with a filled cell on each of the two faces (+Y, +Z) on which it has none."""
    from tests import distance_reference as DR
    d, m = (a.copy() for a in DR.scene())
    for x, y, z in ((5, DISTANCE_SHAPE[1] - 1, 4), (6, 30, DISTANCE_SHAPE[2] - 1)):
        d[z, y, x], m[z, y, x] = 1.0, 4
    return d, m


def terrain_params(floor_y, flags, amplitude=48, **kw):
    """The contract's quoted parameter set with its base height 24 above `floor_y`: the terrain is a function of the world coordinate, and
    the surface crosses a box standing on that floor.  Returns (TerrainParams, dict)."""
    from tests.terrain_cases import params
    return params(base_height=floor_y + 24, amplitude=amplitude, flags=flags, **kw)


def long_terrain_params(box, flags):
    """The surface inside the box's y range: a quarter of the way up, over a quarter of the height (at least 2)."""
    ny = box.shape[1]
    from tests.terrain_cases import params
    return params(base_height=box.origin[1] + ny // 4, amplitude=max(ny // 4, 2), flags=flags)


def stamp_flush(model_xyz, end):
    """For each of the 48 orientations the placement whose world box ends exactly at 32768 on every axis (end = +1) or starts exactly at
    -32768 (end = -1)."""
    from tests.stamp_reference import ORIENTATIONS, world_voxels
    out = []
    for axis, flip in ORIENTATIONS:
        w = world_voxels(model_xyz, (0, 0, 0), axis, flip)
        offset = (LATTICE_HI - 1 - w.max(axis=0)) if end > 0 else (LATTICE_LO - w.min(axis=0))
        out.append((tuple(int(c) for c in offset), axis, flip))
    return out


def stamp_flush_in(model_xyz, origin, shape):
    """For each of the 48 orientations the placement inside the box that lies flush against every end of the lattice that the box touches,
    and in the middle of the box on the other axes."""
    from tests.stamp_reference import ORIENTATIONS, world_voxels
    out = []
    for axis, flip in ORIENTATIONS:
        w = world_voxels(model_xyz, (0, 0, 0), axis, flip)
        lo, hi = w.min(axis=0), w.max(axis=0)
        offset = [LATTICE_LO - int(lo[a]) if origin[a] == LATTICE_LO else LATTICE_HI - 1 - int(hi[a]) if origin[a] + shape[a] == LATTICE_HI
                  else origin[a] + shape[a] // 2 for a in range(3)]
        out.append((tuple(offset), axis, flip))
    return out


def stamp_clipped(origin, shape):
    """For each of the 48 orientations a placement with its offset on a corner of the box, at the faces that are not the lattice's end: the
    small model has voxels on both sides of zero along every local axis, so the box clips it on all three axes."""
    from tests.stamp_reference import ORIENTATIONS
    corner = tuple(origin[a] if origin[a] > LATTICE_LO else origin[a] + shape[a] for a in range(3))
    assert all(LATTICE_LO + 8 < c < LATTICE_HI - 8 for c in corner)
    return [(corner, axis, flip) for axis, flip in ORIENTATIONS]


def stamp_beyond(model_xyz, end):
    """stamp_flush moved one voxel out of the lattice, along the axis k % 3 for orientation k."""
    out = []
    for k, (offset, axis, flip) in enumerate(stamp_flush(model_xyz, end)):
        offset = list(offset)
        offset[k % 3] += end
        out.append((tuple(offset), axis, flip))
    return out


def world_box(model_xyz, place):
    """(lo, hi) of the placed model's world voxels, half open."""
    from tests.stamp_reference import world_voxels
    w = world_voxels(model_xyz, *place)
    return tuple(int(c) for c in w.min(axis=0)), tuple(int(c) + 1 for c in w.max(axis=0))


def rod_model(length=70):
    """A rod along local x, `length` cells, 2 x 2 across with holes, ids by position: long enough to span bricks and 64-cell borders."""
    xyz = np.array([(x, y, z) for x in range(length) for y in range(2) for z in range(2) if (x + 2 * y + 3 * z) % 5], dtype=np.int32)
    return xyz, (1 + np.arange(len(xyz)) % 250).astype(np.uint32)


def long_stamp_places(box):
    """The rod along the long axis: flush against each end of the box, hanging out of each end (inside the lattice or not at all:
    where the end is the lattice's the placement stays flush), and across the middle; both signs."""
    a, u, v = box.axis, box.u_axis, box.v_axis
    axis = (a, u, v)
    out = []
    for flip in (0, 1, 6):
        for t in (0, box.length - 70, box.length // 2 - 35, -20, box.length - 50, 63 * 64 - 3):
            lo = min(max(box.origin[a] + t, LATTICE_LO), LATTICE_HI - 70)      # the rod's first world cell along the long axis
            offset = [0, 0, 0]
            offset[a], offset[u], offset[v] = lo + (70 if flip & 1 else 0), box.origin[u] + 1 + (2 if flip & 2 else 0), box.origin[v] + 2 + (2 if flip & 4 else 0)
            out.append((tuple(offset), axis, flip))
    return out


def limit_mesh(which):
    """((positions, triangles), lo, hi): a box-shaped mesh of 20 cells in the corner of the limit box SHAPE, three of its faces exactly on
    the planes of the lattice's end that the box touches there."""
    origin = limit_origin(which, SHAPE)
    hi = box_hi(origin, SHAPE)
    lo_m = [origin[a] if origin[a] == LATTICE_LO else hi[a] - 20 for a in range(3)]
    hi_m = [lo_m[a] + 20 for a in range(3)]
    return face_box_mesh(lo_m, hi_m), lo_m, hi_m


def limit_terrain_cases(origin):
    """[(tag, TerrainParams, dict)] for a limit box SHAPE at `origin`: solid, SHELL | CLOSE_SIDES, ADD | SHELL (over prior content), and a
    taller solid terrain some of whose columns the box's top cuts off — the one that writes voxels on the +Y face."""
    out = [(f"flags {flags}", *terrain_params(origin[1], flags)) for flags in (0, 3, 5)]
    return out + [("tall", *terrain_params(origin[1], 0, amplitude=96))]


LONG_TERRAIN_FLAGS = (0, 3, 5)


def components_at_lattice_ends(records, origin, shape):
    """[(face, record)]: for each face of the box that lies on an end of the lattice, the largest component of more than one voxel whose
    bounds reach it (face numbering 0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z, the bit of `touches` for a whole-box labelling)."""
    out = []
    for a in range(3):
        for face, on_end in ((2 * a, origin[a] + shape[a] == LATTICE_HI), (2 * a + 1, origin[a] == LATTICE_LO)):
            if on_end:
                mine = records[((records["touches"] >> face) & 1 == 1) & (records["n_voxels"] > 1)]
                if len(mine):
                    out.append((face, mine[np.argmax(mine["n_voxels"])]))
    return out


def voxelized_over(d0, m0, filled, ids, density):
    """The arrays after a voxelization over prior content: written voxels get `density` and their id, the others are untouched."""
    return np.where(filled, np.float32(density), d0).astype(np.float32), np.where(filled, ids, m0).astype(np.uint32)
