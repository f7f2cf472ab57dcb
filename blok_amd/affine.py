"""A model resampled into a voxel volume through an affine map (include/blok_world.h: blok_affine_from_instance, blok_affine_from_matrix,
blok_affine_stamp_voxels): the records HipTracer.volume_stamp_affine takes, and its contract over numpy arrays on the CPU."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _ffi
from ._ffi import AFFINE, BlokError, INSTANCE, STAMP_ERASE, STAMP_KEEP, STAMP_SET  # noqa: F401


def from_instance(place, scale_log2: int = 0) -> np.ndarray:
    """blok_affine_from_instance: one INSTANCE record (blok_amd.stamp.placement) and a scale exponent <= 8 as one AFFINE record, exactly:
    with exponent 0 what volume_stamp_models writes, above it the cells the tracer shows for a model of that exponent."""
    p = np.ascontiguousarray(place, dtype=INSTANCE).reshape(-1)
    assert len(p) == 1, "one placement"
    out = np.zeros(1, dtype=AFFINE)
    rc = _ffi.host_lib().blok_affine_from_instance(_ffi.ptr(p), int(scale_log2), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_affine_from_instance")
    return out


def from_matrix(forward, model: int = 0) -> np.ndarray:
    """blok_affine_from_matrix: a forward map model -> world, (3, 4) (world = F @ model + T, in voxels), as one AFFINE record of `model`."""
    f = np.ascontiguousarray(forward, dtype=np.float64).reshape(-1)
    assert len(f) == 12, "a 3 x 4 matrix, row major"
    out = np.zeros(1, dtype=AFFINE)
    rc = _ffi.host_lib().blok_affine_from_matrix(f.ctypes.data_as(C.POINTER(C.c_double)), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_affine_from_matrix")
    out["model"] = int(model)
    return out


def rotation_matrix(yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0, scale: float = 1.0, pivot=(0.0, 0.0, 0.0), position=(0.0, 0.0, 0.0)):
    """The forward map world = position + scale * R (model - pivot), R = Ry(yaw) Rx(pitch) Rz(roll), angles in radians, as (3, 4) float64.
    Every element is spelled out in Python floats (the C library's sin and cos): a driver that writes the same expressions gets the same bits."""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    ry = ((cy, 0.0, sy), (0.0, 1.0, 0.0), (-sy, 0.0, cy))
    rx = ((1.0, 0.0, 0.0), (0.0, cp, -sp), (0.0, sp, cp))
    rz = ((cr, -sr, 0.0), (sr, cr, 0.0), (0.0, 0.0, 1.0))
    if pitch == 0.0 and roll == 0.0:
        r = ry
    else:
        rxz = [[sum(rx[i][k] * rz[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        r = [[sum(ry[i][k] * rxz[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    s = float(scale)
    pv = [float(c) for c in pivot]
    out = np.zeros((3, 4), dtype=np.float64)
    for i in range(3):
        row = [s * r[i][0], s * r[i][1], s * r[i][2]]
        out[i, :3] = row
        out[i, 3] = float(position[i]) - (row[0] * pv[0] + row[1] * pv[1] + row[2] * pv[2])
    return out


def rotation(yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0, scale: float = 1.0, pivot=(0.0, 0.0, 0.0), position=(0.0, 0.0, 0.0),
             model: int = 0) -> np.ndarray:
    """One AFFINE record that turns the model by yaw about +y, pitch about +x and roll about +z (radians; applied roll first), scales it and
    puts the model-space point `pivot` at the world point `position` (both in voxels; a voxel v is the cube [v, v + 1))."""
    return from_matrix(rotation_matrix(yaw, pitch, roll, scale, pivot, position), model)


def stamp_affine_host(density, material_ids, origin, model_xyz, model_materials, record, lo=None, hi=None, mode: int = STAMP_SET,
                      value: float = 1.0) -> int:
    """blok_affine_stamp_voxels: resamples the voxel list (local lattice; the last duplicate wins) through one AFFINE record into the region
    (world voxels, half open; both None = the whole box) of the [z][y][x] arrays of a box at world `origin`, in place (both arrays must be
    C-contiguous float32 / uint32).  Returns the cells written."""
    assert density.dtype == np.float32 and material_ids.dtype == np.uint32 and density.flags.c_contiguous and material_ids.flags.c_contiguous
    assert density.ndim == 3 and density.shape == material_ids.shape, "arrays are [z][y][x] over the whole box"
    nz, ny, nx = density.shape
    xyz = np.ascontiguousarray(model_xyz, dtype=np.int32).reshape(-1, 3)
    mats = np.ascontiguousarray(model_materials, dtype=np.uint32).reshape(-1)
    assert len(xyz) == len(mats), "one material id per voxel"
    rec = np.ascontiguousarray(record, dtype=AFFINE).reshape(-1)
    assert len(rec) == 1, "one record"
    o = (C.c_int32 * 3)(*[int(c) for c in origin])
    rlo = None if lo is None else (C.c_int32 * 3)(*[int(c) for c in lo])
    rhi = None if hi is None else (C.c_int32 * 3)(*[int(c) for c in hi])
    n = C.c_uint64(0)
    rc = _ffi.host_lib().blok_affine_stamp_voxels(_ffi.ptr(density), _ffi.ptr(material_ids), o, nx, ny, nz, _ffi.ptr(xyz) if len(xyz) else None,
                                                  _ffi.ptr(mats) if len(mats) else None, len(xyz), _ffi.ptr(rec), rlo, rhi, int(mode), float(value),
                                                  C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_affine_stamp_voxels")
    return int(n.value)
