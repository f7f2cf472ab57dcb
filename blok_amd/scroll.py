"""The scroll of the resident volume on the CPU (blok_scroll_plan, blok_scroll_voxels): the host builds of HipTracer.volume_scroll.  A plan
is one _ffi.SCROLL_INFO record; boxes(info, "exposed") lists its boxes as ((lo xyz), (hi xyz)) pairs in world voxels."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

PLAN_ONLY = _ffi.SCROLL_PLAN_ONLY


def _vec(v):
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


def boxes(info, which: str = "exposed"):
    """The exposed or the leaving boxes of a SCROLL_INFO record as a list of ((x0, y0, z0), (x1, y1, z1)), world voxels, half open."""
    rec = np.asarray(info).reshape(-1)[0]
    n = int(rec["n_" + which])
    return [(tuple(int(c) for c in rec[which][i]["lo"]), tuple(int(c) for c in rec[which][i]["hi"])) for i in range(n)]


def scroll_plan_host(origin, shape_xyz, delta) -> np.ndarray:
    """blok_scroll_plan for the box [origin, origin + shape_xyz) moved by delta.  The two filled counts stay 0."""
    info = np.zeros(1, dtype=_ffi.SCROLL_INFO)
    rc = _ffi.host_lib().blok_scroll_plan(_vec(origin), int(shape_xyz[0]), int(shape_xyz[1]), int(shape_xyz[2]), _vec(delta), _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_scroll_plan")
    return info


def scroll_voxels_host(density, material_ids, origin, delta):
    """blok_scroll_voxels over [z][y][x] arrays of a box at world `origin`.  Returns (density, material ids, info) of the box at
    origin + delta."""
    d = np.ascontiguousarray(density, dtype=np.float32)
    m = np.ascontiguousarray(material_ids, dtype=np.uint32)
    assert d.ndim == 3 and m.shape == d.shape, "the arrays are [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    out_d, out_m = np.empty_like(d), np.empty_like(m)
    info = np.zeros(1, dtype=_ffi.SCROLL_INFO)
    rc = _ffi.host_lib().blok_scroll_voxels(_ffi.ptr(d), _ffi.ptr(m), _vec(origin), nx, ny, nz, _vec(delta), _ffi.ptr(out_d), _ffi.ptr(out_m), _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_scroll_voxels")
    return out_d, out_m, info
