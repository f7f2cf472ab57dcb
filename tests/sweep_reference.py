"""A plain model of sweeping a placed model against a voxel volume — TESTS ONLY, numpy alone, written from the contract in
include/blok_hip.h (blok_hip_volume_sweep_models), not from the product's shared header: the voxel list is mapped with index arithmetic,
and for each voxel the boolean array density > 0 is sliced along the axis and searched with argmax; cells outside the box follow the
outside rule.  Also the shapes and scenes the CPU and GPU tests share.

Arrays are [z][y][x] over a box whose voxel (0, 0, 0) sits at world `origin`.  Placement = (offset, axis, flip) as in stamp_reference.py.
Directions: 0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z."""
from __future__ import annotations

import functools

import numpy as np

from tests.stamp_reference import ORIENTATIONS, small_model, world_voxels  # noqa: F401
from tests.terrain_cases import prior

BOX_IS_SOLID = 1
ORIGIN, SHAPE = (-40, -44, -24), (96, 80, 64)                  # the stamp tests' box: (nx, ny, nz) at ORIGIN
IDENTITY = ((0, 1, 2), 0)


def filled_cells(density):
    with np.errstate(invalid="ignore"):
        return np.asarray(density) > 0                         # NaN > 0 is False


def free_along(column, p, step, max_distance, solid):
    """free(v') for one voxel: `column` the filled cells of the box along the axis through the voxel (None: the column misses the box in
    a perpendicular axis), p the voxel's own coordinate there (any integer), step +1 or -1."""
    if column is None:
        return 0 if solid and max_distance > 0 else max_distance
    n = len(column)
    if step < 0:
        column, p = column[::-1], n - 1 - p                    # the mirror image moves towards +
    empty = 0                                                  # cells known empty so far, from p + 1 on
    c = p + 1
    if c < 0:                                                  # in front of the box
        if solid:
            return 0
        empty, c = -c, 0
    if c < n:
        ahead = column[c:]
        if ahead.any():
            return min(empty + int(np.argmax(ahead)), max_distance)
        empty += n - c
    return min(empty, max_distance) if solid else max_distance


def per_voxel(density, origin, model_xyz, placement, direction, max_distance, flags=0):
    """(overlaps (n,) bool, free (n,) int) for the distinct voxels of the list, in np.unique's order, and those voxels."""
    offset, axis, flip = placement
    f = filled_cells(density)
    nz, ny, nx = f.shape
    dims = (nx, ny, nz)
    a, step = direction // 2, (-1 if direction & 1 else 1)
    solid = bool(flags & BOX_IS_SOLID)
    v = np.unique(np.asarray(model_xyz, dtype=np.int64).reshape(-1, 3), axis=0)
    w = world_voxels(v, offset, axis, flip) - np.asarray(origin, dtype=np.int64)
    overlaps = np.zeros(len(w), dtype=bool)
    free = np.zeros(len(w), dtype=object)
    for i, (x, y, z) in enumerate(w.tolist()):
        inside = [0 <= (x, y, z)[k] < dims[k] for k in range(3)]
        overlaps[i] = bool(f[z, y, x]) if all(inside) else solid
        if not all(inside[k] for k in range(3) if k != a):
            column = None
        else:
            column = f[:, y, x] if a == 2 else (f[z, :, x] if a == 1 else f[z, y, :])
        free[i] = free_along(column, (x, y, z)[a], step, int(max_distance), solid)
    return overlaps, free, v


def sweep(density, origin, model_xyz, placement, direction, max_distance, flags=0):
    """(n_overlap, travel, blocked) of one placement."""
    overlaps, free, _ = per_voxel(density, origin, model_xyz, placement, direction, max_distance, flags)
    travel = min([int(max_distance)] + [int(k) for k in free])
    return int(overlaps.sum()), travel, int(travel < max_distance)


def model_levels(model_xyz):
    """Levels of the 64-tree model_create builds: its corner is the voxels' lower corner rounded down to 16, and 4^levels covers the extent
    from there (so its 4^3 bricks are the cells floor(v / 4) of the local lattice)."""
    v = np.asarray(model_xyz, dtype=np.int64).reshape(-1, 3)
    corner = (v.min(axis=0) // 16) * 16
    extent = int((v.max(axis=0) - corner + 1).max())
    levels = 1
    while 4 ** levels < extent:
        levels += 1
    return levels


def in_brick_predecessor(model_xyz, placement, direction):
    """Per distinct voxel (np.unique's order): the model holds the voxel one step AGAINST the direction, and it lies in the same 4^3 brick
    of the local lattice."""
    _, axis, flip = placement
    a, step = direction // 2, (-1 if direction & 1 else 1)
    k = list(axis).index(a)                                    # the local axis along the world axis
    local_step = -step if (flip >> k) & 1 else step
    v = np.unique(np.asarray(model_xyz, dtype=np.int64).reshape(-1, 3), axis=0)
    have = {tuple(p) for p in v.tolist()}
    out = np.zeros(len(v), dtype=bool)
    for i, p in enumerate(v.tolist()):
        q = list(p)
        q[k] -= local_step
        out[i] = tuple(q) in have and all(q[j] // 4 == p[j] // 4 for j in range(3))
    return out


# ---- models -------------------------------------------------------------------------------------------------------------------------

def _xyz(voxels):
    return np.array(voxels, dtype=np.int32).reshape(-1, 3)


def comb_model():
    """A back along x at y = 9 and five teeth hanging down to y = 1 at x = 0, 4, 8, 12, 16: every tooth in a brick column of its own."""
    return _xyz([(x, 9, 0) for x in range(17)] + [(x, y, 0) for x in (0, 4, 8, 12, 16) for y in range(1, 9)])


def cup_model():
    """A cup inside one brick: a 3 x 3 floor at y = 0, walls around it at y = 1 and 2."""
    return _xyz([(x, 0, z) for x in range(3) for z in range(3)] +
                [(x, y, z) for y in (1, 2) for x in range(3) for z in range(3) if (x, z) != (1, 1)])


def models():
    g = range(2)
    ell = [(x, -1, 0) for x in range(-3, 6)] + [(-3, y, 0) for y in range(0, 7)] + [(-3, -1, z) for z in (-2, -1, 1)]
    bar = [(x, 0, 0) for x in range(0, 70, 3)]                 # sparse, 0 .. 69
    return {"one voxel": _xyz([(0, 0, 0)]), "cube": _xyz([(x, y, z) for x in g for y in g for z in g]), "ell": _xyz(ell),
            "comb": comb_model(), "cup": cup_model(), "bar": _xyz(bar), "small": small_model()[0]}


# ---- scenes: name -> density [z][y][x] over SHAPE.  Built once; nothing changes them. ------------------------------------------------

def prior_with_empties(shape_xyz=SHAPE):
    """terrain_cases.prior plus negative and NaN densities, as test_stamp_gpu.py builds it."""
    d0, m0 = prior(tuple(shape_xyz)[::-1])
    d0[::3, ::2, ::5] = -0.5
    d0[1::7, ::3, ::2] = np.nan
    return np.ascontiguousarray(d0), np.ascontiguousarray(m0)


def world(local, origin=ORIGIN):
    return tuple(origin[a] + local[a] for a in range(3))


def at(local, orientation=IDENTITY, origin=ORIGIN):
    """The placement that puts local voxel (0, 0, 0) of an unflipped model on the box-local cell `local` of the box at `origin`."""
    return (world(local, origin), orientation[0], orientation[1])


LATTICE = (-32768, 32768)                                      # a placement's world box lies in [LATTICE[0], LATTICE[1]) on every axis


def in_lattice(place, model_xyz, mirror_in=None):
    """`place` moved by the least offset that brings the model's world box into the lattice: a placement that hung out of a face of the
    box hangs out of it still where the lattice goes on, and lies flush against the lattice's end where the face is that end.  With
    mirror_in = (origin, shape) an axis on which the box leaves the lattice is first mirrored about the box's middle (a model far outside
    one side of the box becomes one as far outside the other).  In the box at ORIGIN nothing moves."""
    offset, axis, flip = place
    offset = list(offset)
    for _ in range(2 if mirror_in else 1):
        w = world_voxels(model_xyz, offset, axis, flip)
        lo, hi = w.min(axis=0), w.max(axis=0) + 1
        for a in range(3):
            out = int(hi[a]) > LATTICE[1] or int(lo[a]) < LATTICE[0]
            if out and mirror_in:
                origin, shape = mirror_in
                offset[a] = 2 * origin[a] + shape[a] - 1 - offset[a]
            elif out:
                offset[a] += min(LATTICE[1] - int(hi[a]), 0) + max(LATTICE[0] - int(lo[a]), 0)
        mirror_in = None
    return (tuple(offset), axis, flip)


# obstacles whose first filled cell is bit 0 and bit 3 of its brick along each axis, behind 4-, 16- and (where the box has one) 64-voxel
# boundaries; every obstacle in a column of its own: (axis, step, start cell, obstacle coordinate along the axis)
def obstacle_runs():
    runs = []
    for axis in range(3):
        n = SHAPE[axis]
        marks = [c for c in (4, 7, 16, 19, 64, 67) if c + 2 < n]
        for step in (1, -1):
            for i, c in enumerate(marks):
                start = [0, 0, 0]
                u, v = (axis + 1) % 3, (axis + 2) % 3
                # u = 2, v = 1 mod 3, and the line aside at u + 1 = 0 mod 3: no column or line of one axis meets one of another
                start[u], start[v] = 5 + 3 * i, 10 + 6 * (step < 0) + 21 * axis
                start[axis] = 2 if step > 0 else (70 if n > 70 else n - 3)
                runs.append((axis, step, tuple(start), c))
    return runs


COMB_AT, COMB_TIE_AT = (30, 30, 20), (30, 30, 44)
CUP_AT = (60, 40, 30)

_scenes = None


def scenes():
    global _scenes
    if _scenes is not None:
        return _scenes
    out = {}
    d, _ = prior_with_empties()
    out["prior"] = d
    # the prior with its middle thinned to one cell in 150: room to travel, and something to meet in every direction
    d = out["prior"].copy()
    rng = np.random.default_rng(29)
    core = (slice(8, 56), slice(10, 70), slice(12, 84))
    d[core] = np.where(rng.random(d[core].shape) < 1.0 / 150.0, np.float32(0.75), np.float32(0.0))
    out["thinned"] = np.ascontiguousarray(d)
    # an empty box with the obstacle runs: the obstacle, a filled cell directly behind the start, and a filled line one column aside
    d = np.zeros(SHAPE[::-1], dtype=np.float32)
    for axis, step, start, c in obstacle_runs():
        p = list(start); p[axis] = c
        d[p[2], p[1], p[0]] = 1.0
        p[axis] = start[axis] - step
        d[p[2], p[1], p[0]] = 2.0
        p = list(start); p[(axis + 1) % 3] += 1
        line = [slice(p[2], p[2] + 1), slice(p[1], p[1] + 1), slice(p[0], p[0] + 1)]
        line[2 - axis] = slice(None)
        d[tuple(line)] = 0.5
    out["runs"] = d
    # a plate under two combs and a cup: a bump under the middle tooth of the first comb, equal bumps under three teeth of the second;
    # a cell inside the cup's wall, and for its twin a cell at the top of the wall
    d = np.zeros(SHAPE[::-1], dtype=np.float32)
    d[:, 20, :] = 1.0
    d[COMB_AT[2], 25, COMB_AT[0] + 8] = 1.0
    for x in (4, 8, 12):
        d[COMB_TIE_AT[2], 27, COMB_TIE_AT[0] + x] = 1.0
    d[CUP_AT[2], CUP_AT[1] + 1, CUP_AT[0]] = 1.0
    d[CUP_AT[2] + 8, CUP_AT[1] + 2, CUP_AT[0]] = 1.0
    d[1::5, 3::4, ::3] = np.where(d[1::5, 3::4, ::3] > 0, d[1::5, 3::4, ::3], np.float32(-1.0))
    d[5, 5, 5] = np.nan
    out["plate"] = d
    _scenes = out
    return out


# ---- cases: scene -> [(tag, model name, placement, direction, max_distance, flags)] --------------------------------------------------

FAR = 0xFFFFFFFF
# offsets that put the small model ([-2, 3) x [-3, 4) x [-1, 2)) across each face of the box, box-local
FACE_OFFSETS = {"-x": (0, 30, 20), "+x": (95, 30, 20), "-y": (40, 1, 20), "+y": (40, 78, 20), "-z": (40, 30, 0), "+z": (40, 30, 63)}
OUTSIDE_OFFSETS = ((130, 30, 20), (40, -60, 20), (40, 30, 30000), (-30000, 30, 20), (40, 30, -9))

_cases = {}


def cases(origin=ORIGIN):
    """The cases over the box SHAPE at `origin`: the same box-local placements; where the box touches the lattice's end a placement that
    would leave the lattice is moved by in_lattice (none is at ORIGIN)."""
    origin = tuple(origin)
    if origin in _cases:
        return _cases[origin]
    m = models()
    put = functools.partial(at, origin=origin)                 # every placement below is in the box at `origin`
    out = {name: [] for name in scenes()}
    # simple shapes, every direction, in the prior and the thinned scene
    for scene in ("prior", "thinned"):
        for name, local in (("one voxel", (41, 33, 29)), ("cube", (43, 39, 31)), ("ell", (47, 36, 33)), ("bar", (13, 41, 30)), ("cup", (50, 22, 18))):
            for direction in range(6):
                for max_distance in (0, 7, 300):
                    out[scene].append((f"{name} {direction} {max_distance}", name, put(local), direction, max_distance, 0))
        out[scene].append(("bar rotated", "bar", put((50, 6, 30), ((1, 0, 2), 0)), 0, 50, 0))
        out[scene].append(("bar flipped along z", "bar", put((50, 40, 62), ((2, 1, 0), 1)), 3, 50, BOX_IS_SOLID))
    # all 48 orientations x 6 directions
    for axis, flip in ORIENTATIONS:
        for direction in range(6):
            out["thinned"].append((f"small {axis} {flip} {direction}", "small", put((48, 40, 32), (axis, flip)), direction, 40, 0))
    # the obstacle runs: one voxel, then the cube (its leading face meets the obstacle; the trailing one the cell behind the start)
    for axis, step, start, c in obstacle_runs():
        direction = 2 * axis + (step < 0)
        for max_distance in (100, abs(c - start[axis]) - 1, abs(c - start[axis])):
            out["runs"].append((f"run {axis} {step} {c} {max_distance}", "one voxel", put(start), direction, max_distance, 0))
        out["runs"].append((f"run {axis} {step} {c} far", "one voxel", put(start), direction, FAR, BOX_IS_SOLID))
    # hanging out of each face, wholly outside, leaving the box during travel; with and without the flag
    for flags in (0, BOX_IS_SOLID):
        for face, local in FACE_OFFSETS.items():
            for k, direction in enumerate(range(6)):
                axis, flip = ORIENTATIONS[(7 * k + 5 * len(out["prior"])) % 48]
                out["prior"].append((f"face {face} {direction} {flags}", "small", put(local, (axis, flip)), direction, 200, flags))
        for local in OUTSIDE_OFFSETS:
            for direction in range(6):
                out["prior"].append((f"outside {local} {direction} {flags}", "small", put(local), direction, FAR if direction < 2 else 500, flags))
        for direction in range(6):                             # a clear run out of the thinned core and the box: the plate scene's empty top
            out["plate"].append((f"leaving {direction} {flags}", "cube", put((70, 60, 50)), direction, 1000, flags))
    # the combs, the cup and its twin
    for max_distance in (0, 3, 5, 6, 100, FAR):
        out["plate"].append((f"comb {max_distance}", "comb", put(COMB_AT), 3, max_distance, 0))
        out["plate"].append((f"comb tie {max_distance}", "comb", put(COMB_TIE_AT), 3, max_distance, 0))
    out["plate"].append(("comb up", "comb", put(COMB_AT), 2, 100, BOX_IS_SOLID))
    out["plate"].append(("cup", "cup", put(CUP_AT), 3, 100, 0))
    out["plate"].append(("cup twin", "cup", put((CUP_AT[0], CUP_AT[1], CUP_AT[2] + 8)), 3, 100, 0))
    for scene in out:
        out[scene] = [(tag, name, in_lattice(place, m[name], (origin, SHAPE) if tag.startswith("outside") else None), direction, max_distance, flags)
                      for tag, name, place, direction, max_distance, flags in out[scene]]
    _cases[origin] = out
    return out


_expected = {}


def expected(scene, origin=ORIGIN):
    """[(n_overlap, travel, blocked)] of a scene's cases over the box at `origin`, computed once."""
    key = (scene, tuple(origin))
    if key not in _expected:
        d, m = scenes()[scene], models()
        _expected[key] = [sweep(d, origin, m[name], place, direction, max_distance, flags)
                          for _, name, place, direction, max_distance, flags in cases(origin)[scene]]
    return _expected[key]


# ---- a box whose extents are no multiples of 4: the last brick along every axis is partial ------------------------------------------
# 97 = 24 bricks + 1 cell, 78 = 19 bricks + 2 cells, 61 = 15 bricks + 1 cell.  A walk towards + leaves the box out of a partial brick,
# a walk towards - from behind the box enters it through one.

ODD_ORIGIN, ODD_SHAPE = (-33, -41, -17), (97, 78, 61)
# per axis: columns (the two coordinates across, in the order of the axes left) that hold nothing, and columns with one obstacle each in
# the last partial brick or next to it: (across, obstacle coordinate along the axis)
ODD_CLEAR = {0: ((10, 9), (77, 60), (40, 31)), 1: ((12, 9), (96, 60), (50, 31)), 2: ((14, 9), (96, 77), (50, 41))}
ODD_OBSTACLES = {0: (((20, 12), 96), ((24, 12), 95), ((28, 12), 92)),
                 1: (((22, 14), 77), ((26, 14), 76), ((30, 14), 75), ((34, 14), 72)),
                 2: (((22, 22), 60), ((26, 22), 59), ((30, 22), 56))}


def odd_cell(axis, across, c):
    """The box-local cell at c along the axis in the column `across`."""
    p = [None, None, None]
    p[axis] = c
    rest = [k for k in range(3) if k != axis]
    p[rest[0]], p[rest[1]] = across
    return tuple(p)


def odd_world(local):
    return tuple(ODD_ORIGIN[a] + local[a] for a in range(3))


def odd_at(local, orientation=IDENTITY):
    return (odd_world(local), orientation[0], orientation[1])


_odd_scenes = None


def odd_scenes():
    global _odd_scenes
    if _odd_scenes is not None:
        return _odd_scenes
    out = {}
    d = np.zeros(ODD_SHAPE[::-1], dtype=np.float32)
    for axis, columns in ODD_OBSTACLES.items():
        for across, c in columns:
            x, y, z = odd_cell(axis, across, c)
            d[z, y, x] = 1.0
    d[2::5, 1::4, ::3] = np.where(d[2::5, 1::4, ::3] > 0, d[2::5, 1::4, ::3], np.float32(-1.0))
    d[3, 3, 3] = np.nan
    out["odd lines"] = d
    # the prior over the odd box, thinned to one cell in 150 right up to the far walls
    d, _ = prior_with_empties(ODD_SHAPE)
    rng = np.random.default_rng(31)
    core = (slice(6, None), slice(8, None), slice(10, None))
    d[core] = np.where(rng.random(d[core].shape) < 1.0 / 150.0, np.float32(0.75), np.float32(0.0))
    out["odd thinned"] = np.ascontiguousarray(d)
    _odd_scenes = out
    return out


_odd_cases = None


def odd_cases():
    """scene -> [(tag, model name, placement, direction, max_distance, flags)] over the odd box."""
    global _odd_cases
    if _odd_cases is not None:
        return _odd_cases
    out = {name: [] for name in odd_scenes()}
    lines = out["odd lines"]
    for axis in range(3):
        n = ODD_SHAPE[axis]
        for flags in (0, BOX_IS_SOLID):
            # a model reaches the far wall, or the near one, along a clear column: one voxel from every position of the last two bricks and
            # from outside on both sides, at distances below, at and beyond the wall
            for across in ODD_CLEAR[axis]:
                for p in (n - 1, n - 2, n - 3, n - 4, n - 5, n - 6, n - 9, 40, 5, 4, 3, 2, 1, 0, -1, -7, n, n + 1, n + 6):
                    for step in (1, -1):
                        to_wall = max(n - 1 - p, 0) if step > 0 else max(p, 0)
                        for max_distance in sorted({FAR, 200, 2, to_wall, to_wall + 1, max(to_wall - 1, 0)}):
                            lines.append((f"wall {axis} {across} {p} {step} {max_distance} {flags}", "one voxel",
                                          odd_at(odd_cell(axis, across, p)), 2 * axis + (step < 0), max_distance, flags))
            # an obstacle in the last partial brick, in the bit before it and in the brick before: met from inside, and from behind the box
            for across, c in ODD_OBSTACLES[axis]:
                for p, step in ((n - 10, 1), (c - 1, 1), (c - 5, 1), (2, 1), (-4, 1), (n + 5, -1), (n, -1), (n - 1, -1), (c, 1), (c, -1), (c + 1, -1)):
                    for max_distance in (FAR, 300, abs(c - p), max(abs(c - p) - 1, 0)):
                        lines.append((f"obstacle {axis} {c} {p} {step} {max_distance} {flags}", "one voxel",
                                      odd_at(odd_cell(axis, across, p)), 2 * axis + (step < 0), max_distance, flags))
            # larger models against the far and the near wall: the cube and the cup (in-brick skips) from the last bricks
            for name in ("cube", "cup", "ell"):
                for back in (2, 3, 4, 5, 7, 11):
                    local = list(odd_cell(axis, ODD_CLEAR[axis][2], n - back))
                    for direction in range(6):
                        lines.append((f"{name} {axis} {back} {direction} {flags}", name, odd_at(tuple(local)), direction, FAR, flags))
    # every orientation and direction near the far corner of the thinned box, where a travel may end at a wall, and across the far faces
    thinned = out["odd thinned"]
    for flags in (0, BOX_IS_SOLID):
        for axis, flip in ORIENTATIONS:
            for direction in range(6):
                thinned.append((f"small {axis} {flip} {direction} {flags}", "small", at_odd_corner(axis, flip), direction, 60, flags))
        for local in ((96, 40, 30), (50, 77, 30), (50, 40, 60), (95, 76, 59), (0, 1, 0)):
            for k, direction in enumerate(range(6)):
                axis, flip = ORIENTATIONS[(11 * k + 5 * len(thinned)) % 48]
                thinned.append((f"face {local} {direction} {flags}", "small", odd_at(local, (axis, flip)), direction, 200, flags))
        for direction in range(6):
            thinned.append((f"bar {direction} {flags}", "bar", odd_at((25, 70, 55)), direction, FAR, flags))
    _odd_cases = out
    return out


def at_odd_corner(axis, flip):
    return odd_at((88, 69, 54), (axis, flip))


_odd_expected = {}


def odd_expected(scene):
    """[(n_overlap, travel, blocked)] of an odd scene's cases, computed once."""
    if scene not in _odd_expected:
        d, m = odd_scenes()[scene], models()
        _odd_expected[scene] = [sweep(d, ODD_ORIGIN, m[name], place, direction, max_distance, flags)
                                for _, name, place, direction, max_distance, flags in odd_cases()[scene]]
    return _odd_expected[scene]
