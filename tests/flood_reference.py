"""The contract of blok_hip_volume_flood_field / blok_hip_volume_edit_by_flood (include/blok_hip.h) restated in numpy — TESTS ONLY, no
product library.  `field` is repeated frontier dilation (a queue is what the host build uses: the two share nothing), `edit` holds the four
predicates, `claims` measures what makes a case hard for a builder that works brick by brick; tests/test_flood_cpu.py pins the model to
hand-written cases.  The shapes the GPU tests run are generated here, so that the host build sees every one of them too.  Arrays are
[z][y][x]; regions and seeds are world voxels, regions half open, both corners None = the whole box."""
from __future__ import annotations

import heapq

import numpy as np

THROUGH_FILLED, SAME_MATERIAL = 1, 2
FAR = 0xFFFF
MAX_STEPS = 65534
FILL, FILL_UNREACHED, PAINT, CLEAR = 0, 1, 2, 3
INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("max_steps", "<u4"), ("farthest", "<u4"),
                 ("n_seed", "<u8"), ("n_reached", "<u8"), ("n_unreached", "<u8")])


def seed_face(f):
    return 1 << (8 + f)


ALL_FACES = sum(seed_face(f) for f in range(6))


def region_of(shape_zyx, origin, lo, hi):
    """Box-local (lo, ext) of a world region."""
    nz, ny, nx = shape_zyx
    if lo is None and hi is None:
        return (0, 0, 0), (nx, ny, nz)
    l = tuple(int(lo[a]) - int(origin[a]) for a in range(3))
    e = tuple(int(hi[a]) - int(lo[a]) for a in range(3))
    assert all(v >= 0 for v in l + e) and all(l[a] + e[a] <= (nx, ny, nz)[a] for a in range(3)), "the region lies in the box"
    return l, e


def passable(d, m, lo, ext, flags, material):
    """Bool [z][y][x] over the region."""
    cut = (slice(lo[2], lo[2] + ext[2]), slice(lo[1], lo[1] + ext[1]), slice(lo[0], lo[0] + ext[0]))
    filled = np.asarray(d, dtype=np.float32)[cut] > 0             # NaN, zeros of either sign and negative densities are empty
    if not flags & THROUGH_FILLED:
        return ~filled
    if flags & SAME_MATERIAL:
        return filled & (np.asarray(m)[cut] == material)
    return filled


def seed_mask(origin, lo, ext, seeds, flags):
    """Bool [z][y][x] over the region: the listed cells and the flagged faces' layers (passable or not)."""
    s = np.zeros((ext[2], ext[1], ext[0]), bool)
    for x, y, z in np.asarray(seeds if seeds is not None else [], dtype=np.int64).reshape(-1, 3):
        p = (int(x) - origin[0] - lo[0], int(y) - origin[1] - lo[1], int(z) - origin[2] - lo[2])
        assert all(0 <= p[a] < ext[a] for a in range(3)), "a listed seed lies in the region"
        s[p[2], p[1], p[0]] = True
    for f in range(6):
        if flags & seed_face(f):
            index = [slice(None)] * 3
            index[2 - f // 2] = 0 if f & 1 else -1                # face 2 a is the high side of axis a, 2 a + 1 the low side
            s[tuple(index)] = True
    return s


def make_info(origin, lo, ext, K, flags, steps, p):
    info = np.zeros(1, dtype=INFO)
    info["version"], info["flags"], info["max_steps"] = 1, flags, K
    info["lo"][0] = [int(origin[a]) + lo[a] for a in range(3)]
    info["ext"][0] = ext
    near = steps[steps != FAR]
    info["farthest"] = int(near.max()) if near.size else 0
    info["n_seed"] = int((steps == 0).sum())
    info["n_reached"] = int(((steps != 0) & (steps != FAR)).sum())
    info["n_unreached"] = int((p & (steps == FAR)).sum())
    return info


def dilate(p, start, K):
    """uint16 [z][y][x]: the steps from the cells `start` (bool, taken where passable) through the passable cells `p`, FAR above K: the
    frontier of step k is every passable cell without a value next to the frontier of step k - 1."""
    steps = np.full(p.shape, FAR, np.uint16)
    flat, pf = steps.reshape(-1), p.reshape(-1)
    nz, ny, nx = p.shape
    frontier = np.flatnonzero(start.reshape(-1) & pf)
    flat[frontier] = 0
    k = 0
    while frontier.size and k < K:
        k += 1
        x, y, z = frontier % nx, (frontier // nx) % ny, frontier // (nx * ny)
        near = np.concatenate([frontier[x > 0] - 1, frontier[x < nx - 1] + 1, frontier[y > 0] - nx, frontier[y < ny - 1] + nx,
                               frontier[z > 0] - nx * ny, frontier[z < nz - 1] + nx * ny])
        near = np.unique(near)
        frontier = near[pf[near] & (flat[near] == FAR)]
        flat[frontier] = k
    return steps


def field(d, m, origin, lo, hi, seeds, K, flags, material=0):
    """(steps, info) of the contract."""
    assert 0 <= K <= MAX_STEPS and not (flags & SAME_MATERIAL and not flags & THROUGH_FILLED)
    lo, ext = region_of(np.shape(d), origin, lo, hi)
    p = passable(d, m, lo, ext, flags, material)
    steps = dilate(p, seed_mask(origin, lo, ext, seeds, flags), K)
    return steps, make_info(origin, lo, ext, K, flags, steps, p)


def edit(density, ids, steps, info, op, d, value, material, origin):
    """The edit of the contract on the [z][y][x] arrays, in place; returns the number of cells written."""
    lo = [int(info["lo"][0][a]) - int(origin[a]) for a in range(3)]
    ext = [int(e) for e in info["ext"][0]]
    through_filled = bool(int(info["flags"][0]) & THROUGH_FILLED)
    assert through_filled == (op in (PAINT, CLEAR)) and (op == FILL_UNREACHED or d <= int(info["max_steps"][0]))
    cut = (slice(lo[2], lo[2] + ext[2]), slice(lo[1], lo[1] + ext[1]), slice(lo[0], lo[0] + ext[0]))
    filled_now = density[cut] > 0
    steps = np.asarray(steps).reshape(ext[2], ext[1], ext[0])
    if op == FILL:
        w = (steps <= d) & ~filled_now
    elif op == FILL_UNREACHED:
        w = (steps == FAR) & ~filled_now
    else:
        w = (steps <= d) & filled_now
    if op in (FILL, FILL_UNREACHED):
        density[cut][w] = value
        ids[cut][w] = material
    elif op == PAINT:
        ids[cut][w] = material
    else:
        density[cut][w] = 0.0
        ids[cut][w] = 0
    return int(w.sum())


def claims(p, start, lo=(0, 0, 0)):
    """What makes a case hard for a builder that owns the field brick by brick, from the model alone.  p, start: bool [z][y][x] over the
    region, whose corner is box-local `lo` (bricks are counted from the box's origin).  Returns
      crossing_gap: over the reached cells, the largest (fewest brick-face crossings among the SHORTEST chains) - (fewest crossings among
        ALL chains): a cell with a gap is first written through few bricks and lowered in a later round;
      longest_in_brick: the largest spread of steps inside one brick: sweeps of a wave that never leave its tile."""
    nz, ny, nx = p.shape
    brick = lambda x, y, z: ((x + lo[0]) // 4, (y + lo[1]) // 4, (z + lo[2]) // 4)

    def dijkstra(order):
        """Lexicographic shortest chains by (steps, crossings) or (crossings, steps)."""
        best = {}
        heap = [((0, 0), (int(x), int(y), int(z))) for z, y, x in zip(*np.nonzero(start & p))]
        heapq.heapify(heap)
        while heap:
            cost, c = heapq.heappop(heap)
            if c in best:
                continue
            best[c] = cost
            for a in range(3):
                for s in (-1, 1):
                    n = list(c); n[a] += s; n = tuple(n)
                    if not (0 <= n[0] < nx and 0 <= n[1] < ny and 0 <= n[2] < nz) or not p[n[2], n[1], n[0]] or n in best:
                        continue
                    cross = int(brick(*n) != brick(*c))
                    step = (1, cross) if order == 0 else (cross, 1)
                    heapq.heappush(heap, ((cost[0] + step[0], cost[1] + step[1]), n))
        return best

    by_steps, by_crossings = dijkstra(0), dijkstra(1)
    gap = max((by_steps[c][1] - by_crossings[c][0] for c in by_steps), default=0)
    steps = dilate(p, start, MAX_STEPS)
    spread = 0
    for bz in range((lo[2]) // 4, (lo[2] + nz - 1) // 4 + 1):
        for by in range((lo[1]) // 4, (lo[1] + ny - 1) // 4 + 1):
            for bx in range((lo[0]) // 4, (lo[0] + nx - 1) // 4 + 1):
                t = steps[max(4 * bz - lo[2], 0):4 * bz + 4 - lo[2], max(4 * by - lo[1], 0):4 * by + 4 - lo[1], max(4 * bx - lo[0], 0):4 * bx + 4 - lo[0]]
                t = t[t != FAR]
                if t.size:
                    spread = max(spread, int(t.max()) - int(t.min()))
    return {"crossing_gap": gap, "longest_in_brick": spread}


# ---- the shapes of the tests ---------------------------------------------------------------------------------------------------------------
NOISE_ORIGIN, NOISE_SHAPE = (-5, -3, -2), (13, 10, 7)             # ragged last bricks on every axis, a negative origin
# the whole box, regions off the brick grid, a one-cell region
NOISE_REGIONS = [(None, None), ((-4, -2, -1), (7, 6, 4)), ((-2, -3, 0), (8, 1, 5)), ((0, 0, 0), (1, 1, 1))]


def noise(passable_share=0.45, seed=7, shape=NOISE_SHAPE):
    """(density, ids) [z][y][x]: a share of the cells empty, the rest filled with ids 1..3 and varied densities."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    empty = rng.random((nz, ny, nx)) < passable_share
    d = np.where(empty, 0.0, rng.uniform(0.25, 2.0, (nz, ny, nx))).astype(np.float32)
    m = np.where(empty, 0, rng.integers(1, 4, (nz, ny, nx))).astype(np.uint32)
    return d, m


def volume_of(p_empty):
    """(density, ids) whose empty cells are the bool array p_empty; the filled ones carry id 2."""
    return np.where(p_empty, 0.0, 1.0).astype(np.float32), np.where(p_empty, 0, 2).astype(np.uint32)


def pockets(p):
    """The passable cells' 6-connected pockets as lists of flat indices, largest first."""
    left, out = p.copy(), []
    while left.any():
        start = np.zeros(p.shape, bool)
        start.reshape(-1)[np.flatnonzero(left.reshape(-1))[0]] = True
        got = dilate(left, start, MAX_STEPS) != FAR
        out.append(np.flatnonzero(got.reshape(-1)))
        left &= ~got
    return sorted(out, key=len, reverse=True)


MAZE_SHAPE, MAZE_GENERATOR_SEED = (13, 12, 11), 1


def maze():
    """13 x 12 x 11, 45 % passable, one seed in the largest pocket: (density, ids, seed xyz)."""
    d, m = noise(0.45, MAZE_GENERATOR_SEED, MAZE_SHAPE)
    nx, ny, nz = MAZE_SHAPE
    i = int(pockets(d == 0)[0][0])
    return d, m, (i % nx, (i // nx) % ny, i // (nx * ny))


def snake():
    """4 x 4 x 4, one brick: in layer z = 0 the rows y = 0 and y = 2 joined at (3, 1, 0), on to the layer's last cell (0, 3, 0) through
    (0, 2, 0)'s neighbour; (0, 3, 1) alone in layer z = 1; layer z = 2 mirrored in y, ending at (0, 0, 2).  Seed (0, 0, 0)."""
    p = np.zeros((4, 4, 4), bool)
    p[0, 0, :] = p[0, 2, :] = True
    p[0, 1, 3] = True
    p[0, 3, 0] = True
    p[1, 3, 0] = True
    p[2, 3, 0] = True
    p[2, 1, :] = p[2, 3, :] = True
    p[2, 2, 3] = True
    p[2, 0, 0] = True
    d, m = volume_of(p)
    return d, m, (0, 0, 0)


def permute(shape, cells, axis):
    """A shape and cells given along x, rotated so that x becomes `axis`."""
    def rot(c):
        out = [0, 0, 0]
        for a in range(3):
            out[(a + axis) % 3] = c[a]
        return tuple(out)
    return rot(shape), [rot(c) for c in cells]


def tunnel(length, axis, end):
    """A box of length x 5 x 3 along `axis`, filled but for its centre line; the seed at the line's low (0) or high (1) end: the only route
    crosses every brick face along the axis, in one direction.  (shape, density, ids, seed)."""
    shape, cells = permute((length, 5, 3), [(0, 2, 1), (length - 1, 2, 1)], axis)
    p = np.zeros(shape[::-1], bool)
    line = [slice(None) if a == axis else (2 if (a - axis) % 3 == 1 else 1) for a in range(3)]
    p[line[2], line[1], line[0]] = True
    d, m = volume_of(p)
    return shape, d, m, cells[end]


def line_box(axis):
    """600 x 5 x 3 along `axis`, all empty, the seed in a corner: D is the sum of the coordinate differences, up to 605."""
    shape, cells = permute((600, 5, 3), [(0, 0, 0)], axis)
    return shape, np.zeros(shape[::-1], np.float32), np.zeros(shape[::-1], np.uint32), cells[0]


def manhattan(shape, seed, K):
    nx, ny, nz = shape
    x, y, z = np.arange(nx)[None, None, :], np.arange(ny)[None, :, None], np.arange(nz)[:, None, None]
    s = np.abs(x - seed[0]) + np.abs(y - seed[1]) + np.abs(z - seed[2])
    return np.where(s <= K, s, FAR).astype(np.uint16)


SCENE_ORIGIN, SCENE_SHAPE = (3, -8, 10), (40, 36, 33)
# box-local [lo, hi) of the closed hollow box (walls one cell thick), of the box with one hole, and of the two touching blocks
CLOSED, HOLED, BLOCK_A, BLOCK_B = ((2, 2, 2), (12, 11, 10)), ((16, 3, 3), (27, 13, 12)), ((5, 18, 14), (14, 27, 22)), ((14, 20, 14), (21, 30, 25))
HOLE = (21, 8, 11)                                                # in the holed box's top wall
CLOSED_INSIDE = (CLOSED[1][0] - CLOSED[0][0] - 2) * (CLOSED[1][1] - CLOSED[0][1] - 2) * (CLOSED[1][2] - CLOSED[0][2] - 2)


def scene():
    """40 x 36 x 33: a closed hollow box (id 1), a box with one hole (id 2), two touching blocks of ids 3 and 4: (density, ids)."""
    nx, ny, nz = SCENE_SHAPE
    d, m = np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.uint32)

    def box(b, density, material):
        (x0, y0, z0), (x1, y1, z1) = b
        d[z0:z1, y0:y1, x0:x1] = density
        m[z0:z1, y0:y1, x0:x1] = material

    for b, material in ((CLOSED, 1), (HOLED, 2)):
        box(b, 1.0, material)
        box((tuple(c + 1 for c in b[0]), tuple(c - 1 for c in b[1])), 0.0, 0)
    d[HOLE[2], HOLE[1], HOLE[0]] = 0.0
    m[HOLE[2], HOLE[1], HOLE[0]] = 0
    box(BLOCK_A, 0.5, 3)
    box(BLOCK_B, 1.5, 4)
    return d, m


def world(cell, origin=SCENE_ORIGIN):
    return tuple(int(cell[a]) + origin[a] for a in range(3))


# ---- the field cases: what the host build (test_flood_cpu.py) and the device (test_flood_gpu.py) are both held to ----------------------------
def _case(name, origin, d, m, lo, hi, seeds, K, flags, material=0):
    return {"name": name, "origin": tuple(origin), "shape": d.shape[::-1], "d": d, "m": m, "lo": lo, "hi": hi, "seeds": seeds, "K": K, "flags": flags,
            "material": material}


def picked_seeds(d, m, origin, lo, hi, flags, material):
    """World cells of a region: its first and its last passable cell, the first twice, and its first impassable cell (ignored by the
    contract) — fewer where the region has none."""
    l, ext = region_of(d.shape, origin, lo, hi)
    p = passable(d, m, l, ext, flags, material).reshape(-1)
    at = lambda i: (int(i) % ext[0] + l[0] + origin[0], (int(i) // ext[0]) % ext[1] + l[1] + origin[1], int(i) // (ext[0] * ext[1]) + l[2] + origin[2])
    yes, no = np.flatnonzero(p), np.flatnonzero(~p)
    return ([at(yes[0]), at(yes[-1]), at(yes[0])] if yes.size else []) + ([at(no[0])] if no.size else [])


def noise_cases():
    out = []
    for share, generator in ((0.45, 7), (0.30, 8), (0.90, 9)):
        d, m = noise(share, generator)
        o = NOISE_ORIGIN
        for r, (lo, hi) in enumerate(NOISE_REGIONS):
            for flags, material in ((0, 0), (THROUGH_FILLED, 0), (THROUGH_FILLED | SAME_MATERIAL, 1), (THROUGH_FILLED | SAME_MATERIAL, 2), (THROUGH_FILLED | SAME_MATERIAL, 3)):
                if flags & SAME_MATERIAL and (share != 0.45 or r > 1):
                    continue
                seeds = picked_seeds(d, m, o, lo, hi, flags, material)
                for K in (3, MAX_STEPS):
                    out.append(_case(f"noise {share} region {r} flags {flags} id {material} K {K}", o, d, m, lo, hi, seeds, K, flags, material))
            if share == 0.45 and r < 3:
                for f in range(6):                                # each face alone, then all six, with and without a listed seed
                    out.append(_case(f"noise region {r} face {f}", o, d, m, lo, hi, None, MAX_STEPS, seed_face(f)))
                out.append(_case(f"noise region {r} all faces", o, d, m, lo, hi, picked_seeds(d, m, o, lo, hi, 0, 0)[:1], 5, ALL_FACES))
                out.append(_case(f"noise region {r} filled from two faces", o, d, m, lo, hi, None, MAX_STEPS, THROUGH_FILLED | seed_face(1) | seed_face(4)))
    return out


def hard_cases():
    out = []
    d, m, s = maze()
    out.append(_case("maze", (0, 0, 0), d, m, None, None, [s], MAX_STEPS, 0))
    out.append(_case("maze region", (0, 0, 0), d, m, (1, 1, 1), (12, 11, 10), picked_seeds(d, m, (0, 0, 0), (1, 1, 1), (12, 11, 10), 0, 0)[:1], 30, 0))
    d, m, s = snake()
    out.append(_case("snake", (0, 0, 0), d, m, None, None, [s], MAX_STEPS, 0))
    out.append(_case("snake capped", (0, 0, 0), d, m, None, None, [s], 13, 0))
    for axis in range(3):
        for end in range(2):
            shape, d, m, s = tunnel(12, axis, end)
            out.append(_case(f"tunnel axis {axis} end {end}", (0, 0, 0), d, m, None, None, [s], MAX_STEPS, 0))
        shape, d, m, s = line_box(axis)
        for K in (255, 599):
            out.append(_case(f"line box axis {axis} K {K}", (0, 0, 0), d, m, None, None, [s], K, 0))
    d, m = noise(0.45, 7)
    o = NOISE_ORIGIN
    empty, full = (np.zeros_like(d), np.zeros_like(m)), (np.ones_like(d), np.full_like(m, 2))
    for name, (vd, vm) in (("empty", empty), ("full", full)):
        for flags in (0, THROUGH_FILLED):
            out.append(_case(f"{name} volume flags {flags} faces", o, vd, vm, None, None, None, MAX_STEPS, flags | seed_face(3)))
            out.append(_case(f"{name} volume flags {flags} seed", o, vd, vm, None, None, [world((6, 5, 3), o)], 4, flags))
    out.append(_case("no seeds", o, d, m, None, None, None, 9, 0))
    out.append(_case("K = 0", o, d, m, None, None, picked_seeds(d, m, o, None, None, 0, 0), 0, seed_face(0)))
    return out


def corridor(axis, length=16384):
    """length x 5 x 3 along `axis`, filled but for its centre line, the seed at the line's low end, K = 65534: farthest = length - 1."""
    shape, d, m, s = tunnel(length, axis, 0)
    return _case(f"corridor axis {axis} length {length}", (0, 0, 0), d, m, None, None, [s], MAX_STEPS, 0)


_MODEL = {}


def model_of(case):
    """field() of a case, computed once."""
    if case["name"] not in _MODEL:
        _MODEL[case["name"]] = field(case["d"], case["m"], case["origin"], case["lo"], case["hi"], case["seeds"], case["K"], case["flags"], case["material"])
    return _MODEL[case["name"]]
