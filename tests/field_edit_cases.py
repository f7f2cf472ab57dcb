"""The cases of tests/test_field_edit_cpu.py and tests/test_field_edit_gpu.py: every op of edit_by_distance and edit_by_flood over three
regions of one small noise volume, with what the numpy models of the two contracts (tests/distance_reference.py, tests/flood_reference.py)
say each leaves.  The regions start off the brick grid and differ in their x extent, which is what the edit kernel's waves are cut along:
65 cells are two 64-lane segments, the second with one live lane; 64 are exactly one full segment; 1 is a single cell."""
from __future__ import annotations

import functools

import numpy as np

from tests import distance_reference as DR
from tests import flood_reference as FR

ORIGIN, SHAPE = (-5, 3, -2), (72, 9, 6)
CORNER, EXT_YZ = (3, 1, 2), (3, 2)                                # the regions' box-local corner, their y and z extents
WIDTHS = (65, 64, 1)
RADIUS, D2 = 2, 2                                                 # the distance fields' radius, the distance ops' threshold
STEPS, D = 4, 2                                                   # the floods' cap, the flood ops' threshold
VALUE, MATERIAL = 0.75, 7                                         # what a written cell gets (no cell of the noise holds either)
SEED = 3
OPS = [("distance", DR.GROW, "grow"), ("distance", DR.SHRINK, "shrink"), ("distance", DR.HOLLOW, "hollow"),
       ("flood", FR.FILL, "fill"), ("flood", FR.FILL_UNREACHED, "fill-unreached"), ("flood", FR.PAINT, "paint"), ("flood", FR.CLEAR, "clear")]
CASES = [(family, op, width) for family, op, _ in OPS for width in WIDTHS]
IDS = [f"{name}-{width}" for _, _, name in OPS for width in WIDTHS]


@functools.lru_cache(maxsize=None)
def noise():
    """(density, ids) [z][y][x], read-only: blobs of a few cells with ragged edges, about half of the cells filled, ids 1..3."""
    nx, ny, nz = SHAPE
    rng = np.random.default_rng(SEED)
    coarse = rng.random((nz // 3 + 1, ny // 3 + 1, nx // 3 + 1))
    smooth = np.repeat(np.repeat(np.repeat(coarse, 3, 0), 3, 1), 3, 2)[:nz, :ny, :nx]
    value = smooth + 0.3 * (rng.random((nz, ny, nx)) - 0.5)
    filled = value > np.median(value)
    d = np.where(filled, 0.25 + 0.5 * rng.random((nz, ny, nx)), 0.0).astype(np.float32)
    m = np.where(filled, 1 + rng.integers(0, 3, (nz, ny, nx)), 0).astype(np.uint32)
    d.setflags(write=False); m.setflags(write=False)
    return d, m


def region(width):
    """World (lo, hi) of the region of that x extent."""
    lo = tuple(ORIGIN[a] + CORNER[a] for a in range(3))
    return lo, (lo[0] + width, lo[1] + EXT_YZ[0], lo[2] + EXT_YZ[1])


def field_args(family, op, width):
    """What the field of the case is taken with: (max_radius, flags) of a distance field, (seeds, max_steps, flags) of a flood.  The flood's
    one seed is the region's first cell, in index order, that the flood can pass (the corner when there is none)."""
    if family == "distance":
        return RADIUS, (0 if op == DR.GROW else DR.TO_EMPTY)
    d, m = noise()
    lo, hi = region(width)
    flags = FR.THROUGH_FILLED if op in (FR.PAINT, FR.CLEAR) else 0
    l, ext = FR.region_of(d.shape, ORIGIN, lo, hi)
    at = np.flatnonzero(FR.passable(d, m, l, ext, flags, 0).reshape(-1))
    i = int(at[0]) if at.size else 0
    seed = (lo[0] + i % ext[0], lo[1] + (i // ext[0]) % ext[1], lo[2] + i // (ext[0] * ext[1]))
    return [seed], STEPS, flags


@functools.lru_cache(maxsize=None)
def expected(family, op, width):
    """(field, info, density, ids, count) of the references: the snapshot and its info, the volume after the edit, the cells written.  Computed
    once and shared: read-only."""
    d, m = noise()
    lo, hi = region(width)
    d2, m2 = d.copy(), m.copy()
    if family == "distance":
        field, info = DR.field(d, ORIGIN, lo, hi, *field_args(family, op, width))
        n = DR.edit(d2, m2, field, info, op, D2, VALUE, MATERIAL, origin=ORIGIN)
    else:
        seeds, steps, flags = field_args(family, op, width)
        field, info = FR.field(d, m, ORIGIN, lo, hi, seeds, steps, flags)
        n = FR.edit(d2, m2, field, info, op, D, VALUE, MATERIAL, ORIGIN)
    for a in (field, info, d2, m2):
        a.setflags(write=False)
    return field, info, d2, m2, n
