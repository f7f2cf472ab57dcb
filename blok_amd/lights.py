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


# ---- the light grid (include/blok_hip.h: "the light grid") ---------------------------------------------------------------------
def host_build_grid(lights, cell_log2: int, reach: int = 1, share: int = 128):
    """blok_light_grid_build: (start, faces, items, LIGHT_GRID_INFO record) of the grid over a host table; bit for bit what `build_grid`
    builds on the device over the same table."""
    t = np.ascontiguousarray(lights, dtype=LIGHT).reshape(-1)
    info = np.zeros(1, dtype=_ffi.LIGHT_GRID_INFO)
    lib = _ffi.host_lib()
    args = (_ffi.ptr(t) if len(t) else None, len(t), int(cell_log2), int(reach), int(share))
    rc = lib.blok_light_grid_build(*args, None, None, None, 0, 0, _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_light_grid_build")
    n_cells, n_items = int(info["n_cells"][0]), int(info["n_items"][0])
    start, faces = np.zeros(n_cells + 1, dtype=np.uint32), np.zeros(n_cells, dtype=np.uint32)
    items = np.zeros(max(n_items, 1), dtype=_ffi.LIGHT_GRID_ITEM)
    rc = lib.blok_light_grid_build(*args, _ffi.ptr(start), _ffi.ptr(faces), _ffi.ptr(items), n_cells, n_items, _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_light_grid_build")
    return start, faces, items[:n_items], info


def build_grid(tracer, cell_log2: int, reach: int = 1, share: int = 128) -> np.ndarray:
    """blok_hip_build_light_grid: builds the grid over the installed world light table on the device and installs it.  Returns the
    LIGHT_GRID_INFO record."""
    out = np.zeros(1, dtype=_ffi.LIGHT_GRID_INFO)
    tracer._check(tracer._lib.blok_hip_build_light_grid(tracer._ctx, int(cell_log2), int(reach), int(share), 0, _ffi.ptr(out)))
    return out


def grid_info(tracer) -> np.ndarray:
    """blok_hip_light_grid_info: the LIGHT_GRID_INFO record of the installed grid (zeros without one)."""
    out = np.zeros(1, dtype=_ffi.LIGHT_GRID_INFO)
    tracer._check(tracer._lib.blok_hip_light_grid_info(tracer._ctx, _ffi.ptr(out)))
    return out


def grid_download(tracer, what: int, first: int | None = None, count: int | None = None, page: int = 1 << 22) -> np.ndarray:
    """blok_hip_light_grid_download: elements [first, first + count) of the grid's start (what 0), faces (1) or items (2) array (both
    None: all of it), `page` elements a call."""
    if first is None and count is None:
        g = grid_info(tracer)
        n_cells = int(g["n_cells"][0])
        first, count = 0, (n_cells + 1 if n_cells else 0, n_cells, int(g["n_items"][0]))[int(what)]
    out = np.zeros(int(count or 0), dtype=_ffi.LIGHT_GRID_ITEM if int(what) == _ffi.LIGHT_GRID_ITEMS else np.uint32)
    return tracer._paged(tracer._lib.blok_hip_light_grid_download, out, int(first or 0), page, int(what))


def clear_grid(tracer) -> None:
    tracer._check(tracer._lib.blok_hip_light_grid_clear(tracer._ctx))


# ---- emissive models as lights (include/blok_hip.h: "emissive models as lights") ----------------------------------------------
def host_model_lights(xyz, material_ids, materials) -> np.ndarray:
    """blok_model_lights: the LIGHT records of the exposed emissive unit faces of the model `model_create` makes of the voxel list, in the
    order of its material array; bit for bit what `model_lights` builds on the device."""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
    ids = np.ascontiguousarray(material_ids, dtype=np.uint32).reshape(-1)
    m = np.ascontiguousarray(materials, dtype=MATERIAL).reshape(-1)
    if len(ids) != len(xyz):
        raise ValueError("one material id per voxel")
    lib = _ffi.host_lib()
    n = C.c_uint64()
    args = (_ffi.ptr(xyz) if len(xyz) else None, _ffi.ptr(ids) if len(ids) else None, len(ids), _ffi.ptr(m) if len(m) else None, len(m))
    rc = lib.blok_model_lights(*args, None, 0, C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_model_lights")
    out = np.zeros(int(n.value), dtype=LIGHT)
    rc = lib.blok_model_lights(*args, _ffi.ptr(out) if len(out) else None, len(out), C.byref(n))
    if rc != 0:
        raise BlokError(rc, "blok_model_lights")
    return out


def instance_light_record(instance, scale_log2: int, model_face) -> np.ndarray:
    """blok_instance_light_record: the world-lattice LIGHT record (du = dv = 2**scale_log2, cum 0) of one unit face of a model's table under
    one INSTANCE record."""
    inst = np.ascontiguousarray(instance, dtype=_ffi.INSTANCE).reshape(1)
    face = np.ascontiguousarray(model_face, dtype=LIGHT).reshape(1)
    out = np.zeros(1, dtype=LIGHT)
    _ffi.host_lib().blok_instance_light_record(_ffi.ptr(inst), int(scale_log2), _ffi.ptr(face), _ffi.ptr(out))
    return out[0]


def model_lights(tracer, model: int) -> np.ndarray:
    """blok_hip_model_lights: builds and installs the model's light table from its own tree and the tracer's material table.  Returns the
    LIGHTS_INFO record (n = n_faces = the faces; zeros: no faces, no table)."""
    out = np.zeros(1, dtype=LIGHTS_INFO)
    tracer._check(tracer._lib.blok_hip_model_lights(tracer._ctx, int(model), 0, _ffi.ptr(out)))
    return out


def model_lights_info(tracer, model: int) -> np.ndarray:
    out = np.zeros(1, dtype=LIGHTS_INFO)
    tracer._check(tracer._lib.blok_hip_model_lights_info(tracer._ctx, int(model), _ffi.ptr(out)))
    return out


def model_lights_download(tracer, model: int, first: int | None = None, count: int | None = None, page: int = 1 << 22) -> np.ndarray:
    """blok_hip_model_lights_download: records [first, first + count) of the model's table (both None: all of it), `page` records a call."""
    if first is None and count is None:
        first, count = 0, int(model_lights_info(tracer, model)["n"][0])
    return tracer._paged(tracer._lib.blok_hip_model_lights_download, np.zeros(int(count or 0), dtype=LIGHT), int(first or 0), page, int(model))


def model_lights_clear(tracer, model: int) -> None:
    tracer._check(tracer._lib.blok_hip_model_lights_clear(tracer._ctx, int(model)))


def instance_lights_info(tracer, instances):
    """blok_hip_instance_lights_info: (the INSTANCE_LIGHTS_INFO record, icum as n + 1 uint32 words) of the prefix kernel over a host table."""
    inst = np.ascontiguousarray(instances if instances is not None else [], dtype=_ffi.INSTANCE).reshape(-1)
    out = np.zeros(1, dtype=_ffi.INSTANCE_LIGHTS_INFO)
    icum = np.zeros(len(inst) + 1, dtype=np.uint32)
    tracer._check(tracer._lib.blok_hip_instance_lights_info(tracer._ctx, _ffi.ptr(inst) if len(inst) else None, len(inst), _ffi.ptr(out), _ffi.ptr(icum)))
    return out, icum
