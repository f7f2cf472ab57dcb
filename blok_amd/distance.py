"""The distance field on the CPU (blok_distance_field, blok_distance_edit): the host build of HipTracer.volume_distance_field and
volume_edit_by_distance, with the flag and op constants.  A field is the pair (dist, info): a uint16 array shaped [z][y][x] over the region
and one _ffi.DISTANCE_INFO record."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

TO_EMPTY = _ffi.DISTANCE_TO_EMPTY
BOX_IS_SOLID = _ffi.DISTANCE_BOX_IS_SOLID
FAR = _ffi.DISTANCE_FAR
GROW, SHRINK, HOLLOW = _ffi.DISTANCE_GROW, _ffi.DISTANCE_SHRINK, _ffi.DISTANCE_HOLLOW
MAX_RADIUS = 255
# the device builder's tiles (csrc/hip/distance_kernels.hip): the x pass writes ROW_CELLS cells along x per workgroup, counted from the brick
# of the region's first cell; the y and z passes write TILE_X cells along x by TILE_ROWS rows along their axis per workgroup, counted from
# the region's corner, and stage CHUNK_ROWS input rows at a time, counted from R rows before a tile's first row
ROW_CELLS, TILE_X, TILE_ROWS, CHUNK_ROWS = 256, 64, 32, 64


def _vec(v):
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


def distance_field_host(density, origin=(0, 0, 0), lo=None, hi=None, max_radius: int = 0, flags: int = 0):
    """blok_distance_field over a [z][y][x] density array of a box at world `origin`; the region in world voxels, half open (both None =
    the whole box).  Returns (dist, info)."""
    d = np.ascontiguousarray(density, dtype=np.float32)
    assert d.ndim == 3, "the array is [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    rlo = tuple(origin) if lo is None else tuple(int(c) for c in lo)
    rhi = tuple(o + n for o, n in zip(origin, (nx, ny, nz))) if hi is None else tuple(int(c) for c in hi)
    ext = [max(h - l, 0) for l, h in zip(rlo, rhi)]
    dist = np.zeros((ext[2], ext[1], ext[0]), dtype=np.uint16)
    info = np.zeros(1, dtype=_ffi.DISTANCE_INFO)
    rc = _ffi.host_lib().blok_distance_field(_ffi.ptr(d) if d.size else None, _vec(origin), nx, ny, nz, _vec(lo), _vec(hi), int(max_radius), int(flags),
                                             _ffi.ptr(dist) if dist.size else None, _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_distance_field")
    return dist, info


def distance_edit_host(density, material_ids, origin, dist, info, op: int, d2: int, value: float = 1.0, material: int = 0) -> int:
    """blok_distance_edit on the [z][y][x] arrays (contiguous float32 / uint32, written in place) of a box at world `origin`; returns the
    number of cells written."""
    assert density.dtype == np.float32 and material_ids.dtype == np.uint32 and density.flags.c_contiguous and material_ids.flags.c_contiguous
    nz, ny, nx = density.shape
    info = np.ascontiguousarray(info, dtype=_ffi.DISTANCE_INFO).reshape(1)
    dist = np.ascontiguousarray(dist, dtype=np.uint16)
    assert dist.size == int(np.prod(info["ext"][0].astype(np.int64))), "one value per cell of the info's region"
    n = C.c_uint64(0)
    rc = _ffi.host_lib().blok_distance_edit(_ffi.ptr(density), _ffi.ptr(material_ids), _vec(origin), nx, ny, nz, _ffi.ptr(dist) if dist.size else None,
                                            _ffi.ptr(info), int(op), int(d2), float(value), int(material), C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_distance_edit")
    return int(n.value)
