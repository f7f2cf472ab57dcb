"""The models the light-table tests build (tests/test_model_lights_cpu.py, tests/test_model_lights_gpu.py): the smallest at which the
table can go wrong — TESTS ONLY.  A case is a voxel list, its material ids, a material table and, where it is known by hand, the number
of faces."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from blok_amd._ffi import MATERIAL

GREY, GLOW, GLOW2 = 1, 2, 3


def materials(n=5, glowing=(GLOW, GLOW2)):
    m = np.zeros(n, dtype=MATERIAL)
    m["albedo"] = (0.6, 0.6, 0.6)
    m["flags"] = 230 << 16
    m["ior"] = 1.5
    for g in glowing:
        m["emission"][g] = (4.0, 3.0, 2.0)
    return m


@dataclass
class Case:
    name: str
    xyz: np.ndarray
    ids: np.ndarray
    materials: np.ndarray
    n_faces: int | None = None


def _case(name, xyz, ids, n_faces=None, mats=None):
    xyz = np.asarray(xyz, dtype=np.int32).reshape(-1, 3)
    ids = np.broadcast_to(np.asarray(ids, dtype=np.uint32), (len(xyz),)).copy()
    return Case(name, xyz, ids, materials() if mats is None else mats, n_faces)


def cube(n, at=(0, 0, 0)):
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    return (g + np.asarray(at)).astype(np.int32)


def table():
    out = [
        _case("one voxel", [(0, 0, 0)], GLOW, 6),
        _case("two adjacent glowing voxels", [(1, 2, 3), (2, 2, 3)], GLOW, 10),
        _case("a glowing voxel buried in a 3^3 block", cube(3), [GLOW if tuple(p) == (1, 1, 1) else GREY for p in cube(3).tolist()], 0),
        _case("a glowing voxel beside a grey one", [(5, 5, 5), (6, 5, 5)], [GLOW, GREY], 5),
        _case("two glowing materials and a duplicate", [(0, 0, 0), (0, 1, 0), (0, 0, 0)], [GREY, GLOW2, GLOW], 10),
        _case("negative local coordinates", [(-1, -1, -1), (0, -1, -1), (-17, -40, -3), (-17, -40, -4)], GLOW, 20),
        _case("65 glowing voxels in a row", [(x, 1, 2) for x in range(65)], GLOW, 65 * 4 + 2),
        _case("a 3^3 lantern", cube(3), GLOW, 54),
        _case("a glowing shell round a grey core", cube(4, (-2, 6, 1)), [GREY if all(0 < c - o < 3 for c, o in zip(p, (-2, 6, 1))) else GLOW for p in cube(4, (-2, 6, 1)).tolist()], 96),
    ]
    for axis in range(3):
        for edge in (4, 64):                           # the pair straddles a brick boundary (3|4) and a level-2 boundary (63|64)
            a, b = [1, 2, 1], [1, 2, 1]
            a[axis], b[axis] = edge - 1, edge
            out.append(_case(f"a pair across {edge - 1}|{edge} on axis {axis}", [a, b], GLOW, 10))
            out.append(_case(f"glowing and grey across {edge - 1}|{edge} on axis {axis}", [a, b], [GLOW, GREY] if axis != 1 else [GREY, GLOW], 5))
    big = materials(65536, glowing=(65535,))
    out.append(_case("ids at and above 65535 read index 65535", [(0, 0, 0), (2, 0, 0), (4, 0, 0), (6, 0, 0)], [65535, 70000, 0xFFFFFFFF, 65534], 18, big))
    zero = materials(3, glowing=(0,))
    out.append(_case("ids beyond the material table read index 0", [(0, 0, 0), (0, 0, 1), (0, 0, 3)], [7, 1, 3], 5 + 6, zero))
    rng = np.random.default_rng(33)
    pts = rng.integers(-9, 23, (700, 3))
    out.append(_case("a random cloud over several bricks", pts, rng.integers(1, 4, len(pts))))
    return out
