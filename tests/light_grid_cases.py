"""TEST INFRASTRUCTURE: the light tables the light-grid tests run over (tests/test_light_grid_cpu.py, tests/test_light_grid_gpu.py).  A case
is a table of LIGHT records that passes blok_lights_check and the (cell_log2, reach) pairs it is built at; the grids come from the host
build, the numpy model (tests/light_grid_reference.py) and the device."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from blok_amd._ffi import LIGHT

ALL = tuple((c, r) for c in (2, 3, 6) for r in (0, 1, 3))


@dataclass
class Case:
    name: str
    lights: np.ndarray
    params: tuple                 # (cell_log2, reach) pairs


def table_of(records) -> np.ndarray:
    """LIGHT records from (lo, du, dv, face) tuples, cum the running sum."""
    t = np.zeros(len(records), dtype=LIGHT)
    cum = 0
    for i, (lo, du, dv, face) in enumerate(records):
        t[i] = (lo, du, dv, 3, face, cum)
        cum += du * dv
    assert cum < 2 ** 32
    return t


def _crowd(n):
    """n small lights whose emitting voxels all lie in cell (0, 0, 0) of a c = 6 grid, areas 1..6 so that lcum is uneven."""
    out = []
    for i in range(n):
        face = i % 6
        a = face >> 1
        lo = [4 + i % 7, 4 + (i // 7) % 7, 4 + (i // 49) % 7]
        lo[a] += 1 - (face & 1)                  # the emitting voxel stays where lo was
        out.append((tuple(lo), 1 + i % 3, 1 + i % 2, face))
    return out


def table() -> list[Case]:
    out = [Case("one unit light", table_of([((5, -3, 9), 1, 1, 2)]), ALL)]
    # the plane coordinate on a cell boundary (64: a boundary at c = 2, 3 and 6): a + face's emitting voxel is the last of the cell below,
    # a - face's the first of the cell above; and one voxel off it, where the two swap sides
    for a in range(3):
        recs = []
        for plane in (64, 65, 63, 0, -64):
            for sign in (0, 1):
                lo = [10, 20, 30]
                lo[a] = plane
                recs.append((tuple(lo), 2, 1, 2 * a + sign))
        out.append(Case(f"emitting voxels beside a cell boundary, axis {a}", table_of(recs), ALL))
    # rectangles over 2 and 3 cells in u and in v (c = 3: voxels 7..15 are cells 0..1, 7..16 cells 0..2), on every face
    recs = []
    for face in range(6):
        for du, dv in ((9, 1), (10, 1), (1, 9), (1, 10), (10, 9)):
            a = face >> 1
            lo = [7, 7, 7]
            lo[a] = 3
            recs.append((tuple(lo), du, dv, face))
    out.append(Case("rectangles over 2 and 3 cells", table_of(recs), ALL))
    out.append(Case("negative coordinates across 0", table_of([((-5, -1, 0), 10, 3, 4), ((0, -5, -9), 10, 12, 1), ((-1, 0, -1), 1, 1, 0), ((-64, -65, -63), 2, 2, 3)]), ALL))
    for n in (63, 64, 65, 300):
        out.append(Case(f"{n} lights in one cell", table_of(_crowd(n)), ((6, 0), (6, 1), (3, 1))))
    far = [((x + 200, y, z + 40), du, dv, f) for (x, y, z), du, dv, f in _crowd(20)]
    out.append(Case("two distant clusters", table_of(_crowd(30) + far + _crowd(5)), ((3, 0), (3, 1), (2, 1), (6, 3))))
    out.append(Case("a 65 536-long rectangle", table_of([((-32768, 7, -9), 65536, 1, 2), ((1, 2, 3), 1, 1, 5)]), ((12, 0), (12, 1), (12, 3), (11, 1))))
    return out


# ---- the limits: (name, lights, cell_log2, reach, passes) ----
def limit_cases():
    corners = lambda hi: table_of([((0, 0, 0), 1, 1, 1), ((hi[0], hi[1], hi[2]), 1, 1, 1)])      # noqa: E731
    plate = [((0, 0, 0), 4096, 4096, 4)]
    return [("2^24 cells exactly", corners((1023, 1023, 1023)), 2, 0, True),
            ("one layer of cells above 2^24", corners((1024, 1023, 1023)), 2, 0, False),
            ("the whole lattice at c = 2", table_of([((-32768, -32768, -32768), 1, 1, 1), ((32767, 32767, 32767), 1, 1, 1)]), 2, 3, False),
            ("37 plates of 1030 x 1030 x 7 cells: 2^28 items crossed", table_of(plate * 37), 2, 3, False)]
