"""TEST INFRASTRUCTURE: the volumes the light-table tests run over (tests/test_lights_cpu.py, tests/test_lights_gpu.py).  A case is a small
box of voxels with a material table; its quads come from the host extraction (blok_quads_extract), its lights from the host build, the
numpy model (tests/lights_reference.py) and the device."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from blok_amd._ffi import MATERIAL

PLAIN, STONE, GLOW_A, GLOW_B = 1, 2, 3, 4


def materials(zero_glows: bool = False, n: int = 6) -> np.ndarray:
    """Index 0: grey (or glowing with zero_glows), 1 and 2 plain, 3 and 4 glowing, 5 so faintly emissive that it is not (sum 0.009)."""
    m = np.zeros(n, dtype=MATERIAL)
    m["albedo"] = (0.5, 0.5, 0.5)
    m["flags"] = 200 << 16                       # roughness 200 / 255, metallic 0
    m["ior"] = 1.5
    m["albedo"][STONE] = (0.7, 0.6, 0.5)
    m["emission"][GLOW_A] = (4.0, 3.0, 2.0)
    m["emission"][GLOW_B] = (0.5, 1.0, 2.5)
    if n > 5:
        m["emission"][5] = (0.003, 0.003, 0.003)
    if zero_glows:
        m["emission"][0] = (1.0, 1.0, 1.0)
    return m


@dataclass
class Case:
    name: str
    origin: tuple
    shape: tuple                  # (nx, ny, nz)
    density: np.ndarray           # [z][y][x]
    ids: np.ndarray
    materials: np.ndarray
    n_lights: int | None = None   # what the case is built to give, where that is known by construction
    n_faces: int | None = None


def _empty(shape):
    nx, ny, nz = shape
    return np.zeros((nz, ny, nx), dtype=np.float32), np.zeros((nz, ny, nx), dtype=np.uint32)


def _block(d, m, lo, hi, material):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    d[z0:z1, y0:y1, x0:x1] = 1.0
    m[z0:z1, y0:y1, x0:x1] = material


def _checker(shape, block, off):
    """A solid block whose cells alternate GLOW_A / PLAIN by the parity of x + y + z + off: every surface face is a quad of its own, kept
    and dropped quads interleave."""
    d, m = _empty(shape)
    a, b, c = block
    z, y, x = np.meshgrid(np.arange(c), np.arange(b), np.arange(a), indexing="ij")
    d[1:1 + c, 1:1 + b, 1:1 + a] = 1.0
    m[1:1 + c, 1:1 + b, 1:1 + a] = np.where((x + y + z + off) % 2 == 0, GLOW_A, PLAIN)
    return d, m


def table() -> list[Case]:
    out = []
    # no emissive material in the world
    shape = (16, 16, 16)
    d, m = _empty(shape)
    _block(d, m, (2, 2, 2), (9, 6, 12), PLAIN)
    _block(d, m, (9, 2, 2), (12, 6, 12), STONE)
    out.append(Case("no emissive material", (-8, -8, -8), shape, d, m, materials(), 0, 0))
    # one glowing voxel alone
    d, m = _empty(shape)
    _block(d, m, (5, 6, 7), (6, 7, 8), GLOW_A)
    out.append(Case("one glowing voxel", (-8, -8, -8), shape, d, m, materials(), 6, 6))
    # glowing voxels fully buried
    d, m = _empty(shape)
    _block(d, m, (2, 2, 2), (10, 10, 10), PLAIN)
    _block(d, m, (4, 4, 4), (7, 8, 6), GLOW_B)
    out.append(Case("glowing voxels buried", (0, 0, 0), shape, d, m, materials(), 0, 0))
    # a glowing voxel on the box's face: the neighbour outside the box is empty
    d, m = _empty(shape)
    _block(d, m, (15, 3, 0), (16, 4, 1), GLOW_A)
    _block(d, m, (0, 15, 9), (1, 16, 10), GLOW_B)
    out.append(Case("glowing voxels on the box's faces", (-16, 4, 100), shape, d, m, materials(), 12, 12))
    # a 32 x 32 plate beside unit faces: uneven cum
    shape = (40, 16, 40)
    d, m = _empty(shape)
    _block(d, m, (4, 8, 4), (36, 9, 36), GLOW_A)
    _block(d, m, (1, 3, 1), (2, 4, 2), GLOW_B)
    _block(d, m, (38, 12, 38), (39, 13, 39), GLOW_B)
    _block(d, m, (10, 2, 10), (30, 3, 30), STONE)
    out.append(Case("a 32 x 32 plate beside unit faces", (-20, 0, -20), shape, d, m, materials(), 6 + 12, 2 * 1024 + 4 * 32 + 12))
    # 3-D checkerboards of glowing and plain cells: kept counts of 63, 64, 65 (one wave, just under and over) and one above 4096
    for kept, block, off in ((63, (3, 5, 6), 0), (64, (1, 1, 33), 1), (65, (1, 1, 32), 0)):
        shape = tuple(b + 2 for b in block)
        d, m = _checker(shape, block, off)
        out.append(Case(f"checkerboard, {kept} lights", (-3, 5, -1), shape, d, m, materials(), kept, kept))
    block = (96, 48, 2)
    shape = (98, 50, 4)
    d, m = _checker(shape, block, 0)
    out.append(Case("checkerboard, above 4096 lights", (-30, -20, 0), shape, d, m, materials(), None, None))
    # a material id beyond the table is judged as material 0: dropped while 0 is plain, kept when 0 glows
    shape = (16, 16, 16)
    d, m = _empty(shape)
    _block(d, m, (3, 3, 3), (5, 4, 4), 77)
    _block(d, m, (8, 8, 8), (9, 9, 9), 70000)
    _block(d, m, (11, 3, 3), (12, 4, 4), GLOW_A)
    _block(d, m, (3, 11, 11), (4, 12, 12), 5)           # emission below the threshold
    out.append(Case("ids beyond the table, material 0 plain", (0, 0, 0), shape, d, m, materials(False), 6, 6))
    out.append(Case("ids beyond the table, material 0 glows", (0, 0, 0), shape, d, m, materials(True), 6 + 6 + 6, 6 + 10 + 6))
    return out


def quads_of(case: Case) -> np.ndarray:
    from blok_amd import mesh as M
    return M.extract_quads_host(case.density, case.ids, case.origin)
