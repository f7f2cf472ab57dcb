"""A placed model swept against a voxel volume on the CPU (include/blok_world.h: blok_sweep_voxels): the contract of
HipTracer.volume_sweep_models over a numpy array and a voxel list.  Placements are blok_amd.stamp.placement records."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError, INSTANCE, SWEEP_BOX_IS_SOLID, SWEEP_RESULT  # noqa: F401

# directions, blok_hit::face numbering
PLUS_X, MINUS_X, PLUS_Y, MINUS_Y, PLUS_Z, MINUS_Z = range(6)


def sweep_voxels_host(density, origin, model_xyz, place, direction: int, max_distance: int, flags: int = 0) -> np.ndarray:
    """blok_sweep_voxels: the voxel list (local lattice, distinct voxels) under one placement against the [z][y][x] density array of a box
    at world `origin`: how many of its voxels land on filled cells, and how far it can travel along `direction` (0 +X .. 5 -Z) before
    one does, at most max_distance.  Returns one SWEEP_RESULT record."""
    d = np.ascontiguousarray(density, dtype=np.float32)
    assert d.ndim == 3, "the array is [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    xyz = np.ascontiguousarray(model_xyz, dtype=np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(place, dtype=INSTANCE).reshape(-1)
    assert len(p) == 1, "one placement"
    o = (C.c_int32 * 3)(*[int(c) for c in origin])
    out = np.zeros(1, dtype=SWEEP_RESULT)
    rc = _ffi.host_lib().blok_sweep_voxels(_ffi.ptr(d), o, nx, ny, nz, _ffi.ptr(xyz) if len(xyz) else None, len(xyz), _ffi.ptr(p),
                                           int(direction), int(max_distance), int(flags), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_sweep_voxels")
    return out[0]
