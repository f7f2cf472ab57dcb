"""TEST INFRASTRUCTURE: the light grid in numpy (include/blok_hip.h, "the light grid"): for every cell, the loop over all lights with the
predicate in(L, g).  Nothing here is shared with the library."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from blok_amd._ffi import LIGHT_GRID_ITEM


def cell_ranges(lights, c: int):
    """(cmin, cmax), int64 [n, 3]: the cells of each light's emitting voxels, both ends inclusive."""
    n = len(lights)
    lo = lights["lo"].astype(np.int64)
    face = lights["face"].astype(np.int64)
    a = face >> 1
    u = np.where(a == 0, 1, 0)
    v = np.where(a == 2, 1, 2)
    i = np.arange(n)
    vmin, vmax = lo.copy(), lo.copy()
    vmin[i, a] = lo[i, a] - np.where(face & 1, 0, 1)      # a + face emits from the voxel below its plane
    vmax[i, a] = vmin[i, a]
    vmax[i, u] = lo[i, u] + lights["du"].astype(np.int64) - 1
    vmax[i, v] = lo[i, v] + lights["dv"].astype(np.int64) - 1
    return vmin >> c, vmax >> c


def listed(cmin, cmax, reach: int, g) -> np.ndarray:
    """in(L, g) for every light: g in absolute cells."""
    g = np.asarray(g, dtype=np.int64)
    return np.all((cmin - reach <= g) & (g <= cmax + reach), axis=1)


def build(lights, c: int, reach: int):
    """(cell_lo, dim, start, faces, items) by the loop over every cell and every light."""
    cmin, cmax = cell_ranges(lights, c)
    cell_lo = cmin.min(axis=0) - reach
    dim = cmax.max(axis=0) + reach - cell_lo + 1
    area = lights["du"].astype(np.int64) * lights["dv"].astype(np.int64)
    start, faces, light, lcum = [0], [], [], []
    for z in range(int(dim[2])):
        for y in range(int(dim[1])):
            for x in range(int(dim[0])):
                members = np.nonzero(listed(cmin, cmax, reach, cell_lo + (x, y, z)))[0]
                a = area[members]
                light.append(members)
                lcum.append(np.cumsum(a) - a)
                faces.append(int(a.sum()))
                start.append(start[-1] + len(members))
    items = np.zeros(start[-1], dtype=LIGHT_GRID_ITEM)
    items["light"] = np.concatenate(light)
    items["lcum"] = np.concatenate(lcum)
    return cell_lo, dim, np.array(start, dtype=np.uint32), np.array(faces, dtype=np.uint32), items


def density_sum(lights, c: int, reach: int, share: int, g) -> Fraction:
    """The sum over every unit face y of the table of p(y) = [A_g > 0] (s / 256) [y in list(g)] / A_g + w_glob at a shading point in
    absolute cell g, in exact rationals: 1 when the list is {L : in(L, g)} and A_g its face sum."""
    cmin, cmax = cell_ranges(lights, c)
    area = [int(d) * int(e) for d, e in zip(lights["du"], lights["dv"])]
    inlist = listed(cmin, cmax, reach, g)
    a_all = sum(area)
    a_g = sum(f for f, m in zip(area, inlist) if m)
    w_glob = (Fraction(256 - share, 256) if a_g else Fraction(1)) / a_all
    total = Fraction(0)
    for f, m in zip(area, inlist):
        total += f * ((Fraction(share, 256) / a_g if m else 0) + w_glob)
    return total
