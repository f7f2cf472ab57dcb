"""The flood from seeds on the CPU (blok_flood_field, blok_flood_edit): the host build of HipTracer.volume_flood_field and
volume_edit_by_flood, with the flag and op constants.  A field is the pair (steps, info): a uint16 array shaped [z][y][x] over the region
and one _ffi.FLOOD_INFO record."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

THROUGH_FILLED = _ffi.FLOOD_THROUGH_FILLED
SAME_MATERIAL = _ffi.FLOOD_SAME_MATERIAL
FAR = _ffi.FLOOD_FAR
MAX_STEPS = _ffi.FLOOD_MAX_STEPS
FILL, FILL_UNREACHED, PAINT, CLEAR = _ffi.FLOOD_FILL, _ffi.FLOOD_FILL_UNREACHED, _ffi.FLOOD_PAINT, _ffi.FLOOD_CLEAR
seed_face = _ffi.flood_seed_face
ALL_FACES = sum(seed_face(f) for f in range(6))


def _vec(v):
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


def flood_field_host(density, material_ids=None, origin=(0, 0, 0), lo=None, hi=None, seeds=None, max_steps: int = MAX_STEPS, flags: int = 0,
                     material: int = 0):
    """blok_flood_field over [z][y][x] arrays of a box at world `origin`; the region and the seeds ([n][3]) in world voxels (both region
    corners None = the whole box).  Returns (steps, info)."""
    d = np.ascontiguousarray(density, dtype=np.float32)
    assert d.ndim == 3, "the array is [z][y][x] over the whole box"
    m = None if material_ids is None else np.ascontiguousarray(material_ids, dtype=np.uint32)
    assert m is None or m.shape == d.shape
    nz, ny, nx = d.shape
    rlo = tuple(origin) if lo is None else tuple(int(c) for c in lo)
    rhi = tuple(o + n for o, n in zip(origin, (nx, ny, nz))) if hi is None else tuple(int(c) for c in hi)
    ext = [max(h - l, 0) for l, h in zip(rlo, rhi)]
    xyz = np.zeros((0, 3), np.int32) if seeds is None else np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
    steps = np.zeros((ext[2], ext[1], ext[0]), dtype=np.uint16)
    info = np.zeros(1, dtype=_ffi.FLOOD_INFO)
    rc = _ffi.host_lib().blok_flood_field(_ffi.ptr(d) if d.size else None, _ffi.ptr(m) if m is not None and m.size else None, _vec(origin), nx, ny, nz,
                                          _vec(lo), _vec(hi), _ffi.ptr(xyz) if len(xyz) else None, len(xyz), int(max_steps), int(flags), int(material),
                                          _ffi.ptr(steps) if steps.size else None, _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_flood_field")
    return steps, info


def flood_edit_host(density, material_ids, origin, steps, info, op: int, d: int = 0, value: float = 1.0, material: int = 0) -> int:
    """blok_flood_edit on the [z][y][x] arrays (contiguous float32 / uint32, written in place) of a box at world `origin`; returns the
    number of cells written."""
    assert density.dtype == np.float32 and material_ids.dtype == np.uint32 and density.flags.c_contiguous and material_ids.flags.c_contiguous
    nz, ny, nx = density.shape
    info = np.ascontiguousarray(info, dtype=_ffi.FLOOD_INFO).reshape(1)
    steps = np.ascontiguousarray(steps, dtype=np.uint16)
    assert steps.size == int(np.prod(info["ext"][0].astype(np.int64))), "one value per cell of the info's region"
    n = C.c_uint64(0)
    rc = _ffi.host_lib().blok_flood_edit(_ffi.ptr(density), _ffi.ptr(material_ids), _vec(origin), nx, ny, nz, _ffi.ptr(steps) if steps.size else None,
                                         _ffi.ptr(info), int(op), int(d), float(value), int(material), C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_flood_edit")
    return int(n.value)
