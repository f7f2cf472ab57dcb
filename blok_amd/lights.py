"""Emissive voxels as lights (include/blok_hip.h: blok_light, "emissive voxels as lights"; include/blok_world.h: blok_lights_from_quads,
blok_lights_check): the light table a context samples in every path-traced frame — built on the device from the quads snapshot, or on
the host from any quads and installed — and its host twin."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError, LIGHT, LIGHTS_INFO, MATERIAL, QUAD  # noqa: F401


def host_from_quads(quads, materials, voxel_size: float = 1.0):
    """blok_lights_from_quads: the LIGHT records of the emissive quads, in the quads' order, and the LIGHTS_INFO record of the table;
    bit for bit what `from_quads` builds on the device from the same quads and material table."""
    q = np.ascontiguousarray(quads, dtype=QUAD).reshape(-1)
    m = np.ascontiguousarray(materials, dtype=MATERIAL).reshape(-1)
    info = np.zeros(1, dtype=LIGHTS_INFO)
    lib = _ffi.host_lib()
    rc = lib.blok_lights_from_quads(_ffi.ptr(q) if len(q) else None, len(q), _ffi.ptr(m) if len(m) else None, len(m), None, 0, float(voxel_size), _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_lights_from_quads")
    out = np.zeros(int(info["n"][0]), dtype=LIGHT)
    rc = lib.blok_lights_from_quads(_ffi.ptr(q) if len(q) else None, len(q), _ffi.ptr(m), len(m), _ffi.ptr(out) if len(out) else None, len(out), float(voxel_size),
                                    _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_lights_from_quads")
    return out, info


def check(lights):
    """blok_lights_check: the LIGHTS_INFO record of a host table that passes blok_hip_set_lights' rules; raises BlokError (status -1, or
    -5 for the size limits) naming the first light that breaks one."""
    t = np.ascontiguousarray(lights, dtype=LIGHT).reshape(-1)
    info = np.zeros(1, dtype=LIGHTS_INFO)
    err = C.create_string_buffer(160)
    rc = _ffi.host_lib().blok_lights_check(_ffi.ptr(t) if len(t) else None, len(t), _ffi.ptr(info), err, len(err))
    if rc != 0:
        raise BlokError(rc, err.value.decode())
    return info


def from_quads(tracer) -> np.ndarray:
    """blok_hip_lights_from_quads: builds and installs the light table from the tracer's quads snapshot and material table.  Returns the
    LIGHTS_INFO record."""
    info = np.zeros(1, dtype=LIGHTS_INFO)
    tracer._check(tracer._lib.blok_hip_lights_from_quads(tracer._ctx, 0, _ffi.ptr(info)))
    return info


def set(tracer, lights) -> np.ndarray:      # noqa: A001  (the entry's name)
    """blok_hip_set_lights: installs a host-built table of LIGHT records; None or an empty table clears."""
    info = np.zeros(1, dtype=LIGHTS_INFO)
    t = np.zeros(0, dtype=LIGHT) if lights is None else np.ascontiguousarray(lights, dtype=LIGHT).reshape(-1)
    tracer._check(tracer._lib.blok_hip_set_lights(tracer._ctx, _ffi.ptr(t) if len(t) else None, len(t), _ffi.ptr(info)))
    return info


def clear(tracer) -> None:
    set(tracer, None)


def info(tracer) -> np.ndarray:
    """blok_hip_lights_info: the LIGHTS_INFO record of the installed table (zeros without one)."""
    out = np.zeros(1, dtype=LIGHTS_INFO)
    tracer._check(tracer._lib.blok_hip_lights_info(tracer._ctx, _ffi.ptr(out)))
    return out


def download(tracer, first: int | None = None, count: int | None = None, page: int = 1 << 22) -> np.ndarray:
    """blok_hip_lights_download: records [first, first + count) of the installed table (both None: all of it), `page` records a call."""
    if first is None and count is None:
        first, count = 0, int(info(tracer)["n"][0])
    return tracer._paged(tracer._lib.blok_hip_lights_download, np.zeros(int(count or 0), dtype=LIGHT), int(first or 0), page)
