"""The pyramid of coarser levels on the CPU (blok_lod_reduce): the host build of HipTracer.volume_reduce, with the flag constant and the
info dtype.  A pyramid is the pair (levels, info): info one _ffi.LOD_INFO record, levels a list with one (n, e, id) triple per level 1..K —
uint16, uint16 and uint32 arrays shaped [z][y][x] over the level's grid (info["level"][0][j - 1]["cext"])."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

VOTE_EXPOSED = _ffi.LOD_VOTE_EXPOSED
SEAMLESS = _ffi.LOD_SEAMLESS                          # terrain_reduce only
MAX_LEVELS = _ffi.LOD_MAX_LEVELS
INFO = _ffi.LOD_INFO
PLANE_DTYPES = (np.uint16, np.uint16, np.uint32)      # plane 0 n, 1 e, 2 id


def _vec(v):
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


def level_shape(info, level: int):
    """[z][y][x] shape of level `level` (1-based) of a pyramid's info."""
    cext = info["level"][0][level - 1]["cext"]
    return int(cext[2]), int(cext[1]), int(cext[0])


def split_planes(raw: np.ndarray, info):
    """The (n, e, id) triples of the levels from the one byte array blok_lod_reduce fills (blok_world.h has the layout)."""
    out, at = [], 0
    for j in range(1, int(info["levels"][0]) + 1):
        shape = level_shape(info, j)
        n = shape[0] * shape[1] * shape[2]
        out.append((raw[at:at + 2 * n].view(np.uint16).reshape(shape).copy(), raw[at + 2 * n:at + 4 * n].view(np.uint16).reshape(shape).copy(),
                    raw[at + 4 * n:at + 8 * n].view(np.uint32).reshape(shape).copy()))
        at += 8 * n
    return out


def reduce_host(density, material_ids, origin=(0, 0, 0), lo=None, hi=None, levels: int = 1, flags: int = 0):
    """blok_lod_reduce over [z][y][x] arrays of a box at world `origin`; the region in world voxels (both corners None = the whole box).
    Returns (levels, info)."""
    d = np.ascontiguousarray(density, dtype=np.float32)
    m = np.ascontiguousarray(material_ids, dtype=np.uint32)
    assert d.ndim == 3 and m.shape == d.shape, "the arrays are [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    lib = _ffi.host_lib()
    info = np.zeros(1, dtype=INFO)
    args = (_ffi.ptr(d) if d.size else None, _ffi.ptr(m) if m.size else None, _vec(origin), nx, ny, nz, _vec(lo), _vec(hi), int(levels), int(flags))
    rc = lib.blok_lod_reduce(*args, None, 0, _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_lod_reduce")
    n_bytes = 8 * sum(int(info["level"][0][j]["n_cells"]) for j in range(int(levels)))
    raw = np.zeros(n_bytes, dtype=np.uint8)
    if n_bytes:
        rc = lib.blok_lod_reduce(*args, _ffi.ptr(raw), n_bytes, _ffi.ptr(info))
        if rc != 0:
            raise BlokError(rc, "blok_lod_reduce")
    return split_planes(raw, info), info


def terrain_reduce_host(params, lo, hi, levels: int = 1, flags: int = 0):
    """blok_terrain_reduce: the terrain function (a blok_amd.terrain.TerrainParams with flags 0) over the world region [lo, hi), reduced
    without a voxel array; the host build of HipTracer.terrain_reduce.  Returns (levels, info)."""
    lib = _ffi.host_lib()
    info = np.zeros(1, dtype=INFO)
    args = (C.byref(params), _vec(lo), _vec(hi), int(levels), int(flags))
    rc = lib.blok_terrain_reduce(*args, None, 0, _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_terrain_reduce")
    n_bytes = 8 * sum(int(info["level"][0][j]["n_cells"]) for j in range(int(levels)))
    raw = np.zeros(n_bytes, dtype=np.uint8)
    if n_bytes:
        rc = lib.blok_terrain_reduce(*args, _ffi.ptr(raw), n_bytes, _ffi.ptr(info))
        if rc != 0:
            raise BlokError(rc, "blok_terrain_reduce")
    return split_planes(raw, info), info
