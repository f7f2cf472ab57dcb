"""Procedural terrain (include/blok_hip.h: blok_terrain_params; include/blok_world.h: blok_terrain_*): the parameter record and the host
evaluation of the function HipTracer.volume_generate_terrain writes on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError, TerrainParams

SHELL, CLOSE_SIDES, ADD = 1, 2, 4


def default_params(n: int, seed: int = 0xB10C0001) -> TerrainParams:
    """A landscape for an n^3 box at the origin: the values a user starts from."""
    p = TerrainParams()
    rc = _ffi.host_lib().blok_terrain_default_params(int(n), int(seed) & 0xFFFFFFFF, C.byref(p))
    if rc != 0:
        raise BlokError(rc, "blok_terrain_default_params")
    return p


def validate(params: TerrainParams) -> bool:
    return _ffi.host_lib().blok_terrain_validate(C.byref(params)) == 0


def height(params: TerrainParams, xz) -> np.ndarray:
    """H(x, z) for an (n, 2) array of world columns: the y of the column's top voxel before caves."""
    xz = np.ascontiguousarray(xz, dtype=np.int32).reshape(-1, 2)
    out = np.zeros(len(xz), dtype=np.int32)
    rc = _ffi.host_lib().blok_terrain_height(C.byref(params), _ffi.ptr(xz), len(xz), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_terrain_height")
    return out


def eval_box(params: TerrainParams, region_lo, region_hi, density=None, ids=None):
    """(density, ids, filled voxels) of the region [lo, hi) as [z][y][x] arrays; with ADD, `density` and `ids` are the prior content
    (updated copies are returned)."""
    lo = (C.c_int32 * 3)(*[int(c) for c in region_lo])
    hi = (C.c_int32 * 3)(*[int(c) for c in region_hi])
    shape = tuple(max(int(region_hi[a]) - int(region_lo[a]), 0) for a in (2, 1, 0))
    d = np.zeros(shape, np.float32) if density is None else np.array(density, dtype=np.float32, order="C").reshape(shape)
    m = np.zeros(shape, np.uint32) if ids is None else np.array(ids, dtype=np.uint32, order="C").reshape(shape)
    n = C.c_uint64(0)
    rc = _ffi.host_lib().blok_terrain_eval(C.byref(params), lo, hi, _ffi.ptr(d), _ffi.ptr(m), C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_terrain_eval")
    return d, m, int(n.value)
