"""Posed models (include/blok_hip.h: blok_pose, "Posed models"; include/blok_world.h: blok_pose_from_instance, blok_pose_from_matrix,
blok_affine_from_pose, blok_pose_motion_record): the records HipTracer.trace_primary_posed / trace_rays_posed take, the fold into a
volume_stamp_affine record, and the motion record of a pose between two frames."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import AFFINE, BlokError, INSTANCE, POSE, POSE_ID, POSE_MOTION  # noqa: F401
from .affine import rotation_matrix


def from_instance(place, voxel_size: float = 1.0) -> np.ndarray:
    """blok_pose_from_instance: one INSTANCE record as one POSE record whose local ray is the lattice instance's, value for value."""
    p = np.ascontiguousarray(place, dtype=INSTANCE).reshape(-1)
    assert len(p) == 1, "one placement"
    out = np.zeros(1, dtype=POSE)
    rc = _ffi.host_lib().blok_pose_from_instance(_ffi.ptr(p), float(voxel_size), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_pose_from_instance")
    return out


def from_matrix(forward, model: int = 0, pivot_local=None) -> np.ndarray:
    """blok_pose_from_matrix: a forward map local -> world, (3, 4) (world = F @ local + T, world units; one model voxel is
    voxel_size * 2**scale wide in local space), inverted in double and rounded once, as one POSE record of `model`.  pivot_local: the local
    point about which the pose is most accurate (None: the local origin)."""
    f = np.ascontiguousarray(forward, dtype=np.float64).reshape(-1)
    assert len(f) == 12, "a 3 x 4 matrix, row major"
    pl = None if pivot_local is None else (C.c_double * 3)(*[float(c) for c in pivot_local])
    out = np.zeros(1, dtype=POSE)
    rc = _ffi.host_lib().blok_pose_from_matrix(f.ctypes.data_as(C.POINTER(C.c_double)), pl, int(model), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_pose_from_matrix")
    return out


def rotation(model: int = 0, yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0, scale: float = 1.0, pivot_local=(0.0, 0.0, 0.0),
             position=(0.0, 0.0, 0.0)) -> np.ndarray:
    """One POSE record that turns the model by yaw about +y, pitch about +x and roll about +z (radians; applied roll first), scales it and
    puts the local point `pivot_local` at the world point `position` (both in world units): blok_amd.affine.rotation's map, traced."""
    return from_matrix(rotation_matrix(yaw, pitch, roll, scale, pivot_local, position), model, pivot_local)


def to_affine(pose, voxel_size: float = 1.0, scale_log2: int = 0) -> np.ndarray:
    """blok_affine_from_pose: the pose of a model of scale exponent `scale_log2` as one AFFINE record for HipTracer.volume_stamp_affine."""
    p = np.ascontiguousarray(pose, dtype=POSE).reshape(-1)
    assert len(p) == 1, "one pose"
    out = np.zeros(1, dtype=AFFINE)
    rc = _ffi.host_lib().blok_affine_from_pose(_ffi.ptr(p), float(voxel_size), int(scale_log2), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_affine_from_pose")
    return out


def motion_record(cur, prev=None, model_usable: bool = True) -> np.ndarray:
    """blok_pose_motion_record: the POSE_MOTION record of pose `cur` that was `prev` one frame earlier (None: it was not in the previous
    table), bit for bit what the posed motion passes build on the device.  model_usable: the model exists and a pose may name it."""
    c = np.ascontiguousarray(cur, dtype=POSE).reshape(-1)
    assert len(c) == 1, "one pose"
    p = None
    if prev is not None:
        p = np.ascontiguousarray(prev, dtype=POSE).reshape(-1)
        assert len(p) == 1, "one previous pose"
    out = np.zeros(1, dtype=POSE_MOTION)
    rc = _ffi.host_lib().blok_pose_motion_record(_ffi.ptr(c), _ffi.ptr(p) if p is not None else None, int(bool(model_usable)), _ffi.ptr(out))
    if rc != 0:
        raise BlokError(rc, "blok_pose_motion_record")
    return out
