"""The scroll of the resident volume as a model — TESTS ONLY, numpy alone, written from include/blok_hip.h (blok_hip_volume_scroll).

plan(origin, dims, delta) is the contract's box arithmetic with Python integers; scroll(d, m, delta) the move, by slicing into zero arrays.
Arrays are [z][y][x]; origins, dims and deltas are (x, y, z).  info() puts both into one _ffi.SCROLL_INFO record to compare bytes with.
The case tables are what tests/test_scroll_cpu.py and tests/test_scroll_gpu.py run."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi


def plan(origin, dims, delta):
    """{"origin", "delta", "exposed", "leaving", "n_cells_kept"}: boxes as ((lo xyz), (hi xyz)), world voxels, half open."""
    old = [(o, o + n) for o, n in zip(origin, dims)]
    new = [(o + d, o + d + n) for o, d, n in zip(origin, delta, dims)]
    C = [(max(a[0], b[0]), min(a[1], b[1])) for a, b in zip(old, new)]
    out = {"origin": tuple(b[0] for b in new), "delta": tuple(int(d) for d in delta)}
    if any(c[1] <= c[0] for c in C):
        whole = lambda box: [(tuple(b[0] for b in box), tuple(b[1] for b in box))]
        out.update(exposed=whole(new), leaving=whole(old), n_cells_kept=0)
        return out

    def outside(box):
        boxes = []
        for a in (2, 1, 0):                                        # the z slab, the y slab, the x slab
            rest = (box[a][0], C[a][0]) if C[a][0] > box[a][0] else (C[a][1], box[a][1])      # box \ C along a: one interval, the sizes are equal
            if rest[1] <= rest[0]:
                continue
            ext = [box[k] if k < a else rest if k == a else C[k] for k in range(3)]
            boxes.append((tuple(e[0] for e in ext), tuple(e[1] for e in ext)))
        return boxes

    out.update(exposed=outside(new), leaving=outside(old), n_cells_kept=int(np.prod([c[1] - c[0] for c in C])))
    return out


def kept_slices(dims, delta):
    """(destination, source) index tuples [z][y][x] of the kept cells, or None when nothing is kept."""
    dst, src = [], []
    for n, d in zip(dims, delta):
        lo, hi = max(0, -d), min(n, n - d)                         # new-box-local cells c with 0 <= c + d < n
        if hi <= lo:
            return None
        dst.append(slice(lo, hi)); src.append(slice(lo + d, hi + d))
    return tuple(dst[::-1]), tuple(src[::-1])


def scroll(d, m, delta):
    """The arrays of the box moved by delta: kept cells bit for bit, every other cell (+0.0f, 0)."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    m = np.ascontiguousarray(m, dtype=np.uint32)
    out_d, out_m = np.zeros_like(d), np.zeros_like(m)
    k = kept_slices(d.shape[::-1], delta)
    if k is not None:
        out_d.view(np.uint32)[k[0]] = d.view(np.uint32)[k[1]]      # (as words: no NaN payload is touched)
        out_m[k[0]] = m[k[1]]
    return out_d, out_m


def filled(d):
    with np.errstate(invalid="ignore"):
        return np.asarray(d) > 0


def info(d, m, origin, delta):
    """The _ffi.SCROLL_INFO record the call returns for the box's arrays (d, m) at `origin`."""
    dims = d.shape[::-1]
    p = plan(origin, dims, delta)
    rec = np.zeros(1, dtype=_ffi.SCROLL_INFO)
    rec["origin"], rec["delta"] = p["origin"], p["delta"]
    for key in ("exposed", "leaving"):
        rec["n_" + key] = len(p[key])
        for i, (lo, hi) in enumerate(p[key]):
            rec[key][0, i]["lo"], rec[key][0, i]["hi"] = lo, hi
    rec["n_cells_kept"] = p["n_cells_kept"]
    rec["n_filled_before"] = int(filled(d).sum())
    k = kept_slices(dims, delta)
    rec["n_filled_kept"] = 0 if k is None else int(filled(d[k[1]]).sum())
    return rec


def paint(boxes, origin, dims):
    """How many of `boxes` cover each cell of the box [origin, origin + dims), [z][y][x]; cells of a box outside it raise."""
    count = np.zeros(tuple(dims)[::-1], dtype=np.int32)
    for lo, hi in boxes:
        l = [a - o for a, o in zip(lo, origin)]
        h = [a - o for a, o in zip(hi, origin)]
        assert all(0 <= a < b <= n for a, b, n in zip(l, h, dims)), (lo, hi)
        count[l[2]:h[2], l[1]:h[1], l[0]:h[0]] += 1
    return count


def inside(origin, dims, other_origin):
    """[z][y][x] bools: the cells of the box at `origin` that also lie in the box of the same dims at `other_origin`."""
    axes = [(np.arange(n) + o >= p) & (np.arange(n) + o < p + n) for o, n, p in zip(origin, dims, other_origin)]
    return axes[2][:, None, None] & axes[1][None, :, None] & axes[0][None, None, :]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
SMALL = ((13, 10, 7), (-5, -3, -2))                 # ragged on all axes: the 4-byte path
MID = ((72, 40, 24), (-20, 8, -12))                 # four levels, more than one level-2 word, the 16-byte path
AXIS_DELTAS = [(4, 0, 0), (-4, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 4), (0, 0, -4)]
MIXED_DELTAS = [(4, -4, 8), (-8, 0, 4), (0, 0, 0)]
GONE = {SMALL: (0, 12, 0), MID: (-72, 4, 0)}        # |delta| >= dims on one axis: nothing is kept
FULL_BRICK = (2, 0, 0)                              # a brick of noise() that is full in either shape


INVALID_ARG, NO_WORLD, UNSUPPORTED = -1, -4, -5
LATTICE_LO, LATTICE_HI = -32768, 32768


def refusals(origin, dims):
    """[(delta or None, flags, status)]: every refusal of the contract for the box.  Unknown flag bits and a ragged delta come before the
    lattice rule only in the message; each entry breaks one rule alone."""
    out = [(None, 0, INVALID_ARG), ((4, 0, 2), 0, INVALID_ARG), ((-3, 0, 0), 0, INVALID_ARG), ((0, 1, 0), 0, INVALID_ARG), ((4, 0, 0), 2, INVALID_ARG),
           ((0, 0, 0), 0x80000001, INVALID_ARG)]
    for a in range(3):
        up = (LATTICE_HI - (origin[a] + dims[a])) // 4 * 4 + 4         # the least multiple of 4 that takes the box's end past the lattice's
        down = -((origin[a] - LATTICE_LO) // 4 * 4 + 4)
        for step in (up, down):
            delta = [0, 0, 0]
            delta[a] = step
            out.append((tuple(delta), 0, UNSUPPORTED))
    return out


def deltas(shape_origin):
    return AXIS_DELTAS + MIXED_DELTAS + [GONE[shape_origin]]


def noise(dims, seed=5):
    """Arrays [z][y][x] with about a third of the cells filled, and among the others -0.0f, NaN with a payload, negative densities and ids
    under density 0; the brick FULL_BRICK is full."""
    rng = np.random.default_rng(seed)
    shape = tuple(dims)[::-1]
    kind = rng.integers(0, 12, size=shape)
    d = np.where(kind < 4, rng.uniform(0.25, 2.0, size=shape), 0.0).astype(np.float32)
    d[kind == 4] = np.float32(-0.0)
    d[kind == 5] = np.float32(-1.5)
    d.view(np.uint32)[kind == 6] = 0x7FC12345                     # a NaN with a payload
    d.view(np.uint32)[kind == 7] = 0xFFA00001                     # a negative signalling one
    m = rng.integers(0, 200, size=shape).astype(np.uint32)
    m[kind >= 10] = 0
    bx, by, bz = FULL_BRICK
    d[4 * bz:4 * bz + 4, 4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = 1.25
    return d, m


def brick_mask(d, bx, by, bz):
    """The 64-bit mask of a brick from the arrays: bit x + 4 y + 16 z, cells outside the box absent."""
    f = filled(d)
    nz, ny, nx = f.shape
    mask = 0
    for z in range(4):
        for y in range(4):
            for x in range(4):
                X, Y, Z = 4 * bx + x, 4 * by + y, 4 * bz + z
                if X < nx and Y < ny and Z < nz and f[Z, Y, X]:
                    mask |= 1 << (x + 4 * y + 16 * z)
    return mask
