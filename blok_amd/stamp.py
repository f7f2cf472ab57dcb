"""Models into a voxel volume and back on the CPU (include/blok_world.h: blok_stamp_voxels, blok_capture_voxels): the contracts of
HipTracer.volume_stamp_models / volume_capture_model over numpy arrays, and the placement record both take."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError, INSTANCE, STAMP_ERASE, STAMP_KEEP, STAMP_SET, CAPTURE_CUT  # noqa: F401


def placement(offset, axis=(0, 1, 2), flip: int = 0, model: int = 0) -> np.ndarray:
    """One blok_instance record: local axis k runs along world axis axis[k], against it when bit k of `flip` is set; a model voxel v'
    lands on offset[axis[k]] + v'_k, or offset[axis[k]] - 1 - v'_k under a flip."""
    p = np.zeros(1, dtype=INSTANCE)
    p["model"], p["offset"], p["axis"], p["flip"] = int(model), tuple(int(c) for c in offset), tuple(int(a) for a in axis), int(flip)
    return p


def stamp_voxels_host(density, material_ids, origin, model_xyz, model_materials, place, mode: int = STAMP_SET, value: float = 1.0) -> int:
    """blok_stamp_voxels: stamps the voxel list (local lattice; the last duplicate wins) under one placement into the [z][y][x] arrays of a
    box at world `origin`, in place (both arrays must be C-contiguous float32 / uint32).  Returns the voxels written."""
    assert density.dtype == np.float32 and material_ids.dtype == np.uint32 and density.flags.c_contiguous and material_ids.flags.c_contiguous
    assert density.ndim == 3 and density.shape == material_ids.shape, "arrays are [z][y][x] over the whole box"
    nz, ny, nx = density.shape
    xyz = np.ascontiguousarray(model_xyz, dtype=np.int32).reshape(-1, 3)
    mats = np.ascontiguousarray(model_materials, dtype=np.uint32).reshape(-1)
    assert len(xyz) == len(mats), "one material id per voxel"
    p = np.ascontiguousarray(place, dtype=INSTANCE).reshape(-1)
    assert len(p) == 1, "one placement"
    o = (C.c_int32 * 3)(*[int(c) for c in origin])
    n = C.c_uint64(0)
    rc = _ffi.host_lib().blok_stamp_voxels(_ffi.ptr(density), _ffi.ptr(material_ids), o, nx, ny, nz, _ffi.ptr(xyz) if len(xyz) else None,
                                           _ffi.ptr(mats) if len(mats) else None, len(xyz), _ffi.ptr(p), int(mode), float(value), C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_stamp_voxels")
    return int(n.value)


def capture_voxels_host(density, material_ids, origin=(0, 0, 0), lo=None, hi=None, count_only: bool = False):
    """blok_capture_voxels: the filled voxels of the region (world voxels, half open; both None = the whole box) as (xyz (n, 3) int32
    relative to the region's corner, material ids), x fastest; with count_only their number."""
    d = np.ascontiguousarray(density, dtype=np.float32)
    m = np.ascontiguousarray(material_ids, dtype=np.uint32)
    assert d.ndim == 3 and d.shape == m.shape, "arrays are [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    o = (C.c_int32 * 3)(*[int(c) for c in origin])
    rlo = None if lo is None else (C.c_int32 * 3)(*[int(c) for c in lo])
    rhi = None if hi is None else (C.c_int32 * 3)(*[int(c) for c in hi])
    n = C.c_uint64(0)
    lib = _ffi.host_lib()
    rc = lib.blok_capture_voxels(_ffi.ptr(d), _ffi.ptr(m), o, nx, ny, nz, rlo, rhi, None, None, 0, C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_capture_voxels")
    if count_only:
        return int(n.value)
    xyz = np.zeros((int(n.value), 3), dtype=np.int32)
    mats = np.zeros(int(n.value), dtype=np.uint32)
    if len(mats):
        rc = lib.blok_capture_voxels(_ffi.ptr(d), _ffi.ptr(m), o, nx, ny, nz, rlo, rhi, _ffi.ptr(xyz), _ffi.ptr(mats), len(mats), C.byref(n))
        if rc != 0:
            raise BlokError(rc, "blok_capture_voxels")
    return xyz, mats
