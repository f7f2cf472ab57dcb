"""The column field and scatter on the CPU (blok_column_field, blok_scatter): the host builds of HipTracer.volume_column_field and
volume_scatter_models, with the flag constants and the two record builders.  A field is the triple (top, material, info): a uint16 and a
uint32 array with one value per column (index cp + ext[p] * cq, p < q the axes other than the field's) and one _ffi.COLUMNS_INFO record."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

FROM_LOW = _ffi.COLUMNS_FROM_LOW
NONE = _ffi.COLUMNS_NONE
ANY_MATERIAL, ROTATE, MIRROR = _ffi.SCATTER_ANY_MATERIAL, _ffi.SCATTER_ROTATE, _ffi.SCATTER_MIRROR
MAX_ENTRIES = _ffi.SCATTER_MAX_ENTRIES
NO_LIMIT = _ffi.SCATTER_NO_LIMIT


def _vec(v):
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


def scatter_params(seed: int = 0, flags: int = 0, cell_log2: int = 3, probability: int = 65536, surface_material: int = 0, min_y: int = -(1 << 31),
                   max_y: int = (1 << 31) - 1, radius: int = 0, max_rise: int = NO_LIMIT, max_drop: int = NO_LIMIT) -> np.ndarray:
    """One _ffi.SCATTER_PARAMS record (blok_hip.h: blok_scatter_params)."""
    p = np.zeros(1, dtype=_ffi.SCATTER_PARAMS)
    for key, value in (("seed", seed), ("flags", flags), ("cell_log2", cell_log2), ("probability", probability), ("surface_material", surface_material),
                       ("min_y", min_y), ("max_y", max_y), ("radius", radius), ("max_rise", max_rise), ("max_drop", max_drop)):
        p[key] = value
    return p


def scatter_entries(entries) -> np.ndarray:
    """_ffi.SCATTER_ENTRY records from (model, weight, anchor xyz, sink) tuples."""
    out = np.zeros(len(entries), dtype=_ffi.SCATTER_ENTRY)
    for i, (model, weight, anchor, sink) in enumerate(entries):
        out[i] = (model, weight, tuple(anchor), sink)
    return out


def column_field_host(density, material_ids, origin=(0, 0, 0), lo=None, hi=None, axis: int = 1, flags: int = 0):
    """blok_column_field over [z][y][x] arrays of a box at world `origin`; the region in world voxels (both corners None = the whole box).
    Returns (top, material, info)."""
    d = np.ascontiguousarray(density, dtype=np.float32)
    m = np.ascontiguousarray(material_ids, dtype=np.uint32)
    assert d.ndim == 3 and m.shape == d.shape, "the arrays are [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    rlo = tuple(origin) if lo is None else tuple(int(c) for c in lo)
    rhi = tuple(o + n for o, n in zip(origin, (nx, ny, nz))) if hi is None else tuple(int(c) for c in hi)
    ext = [max(h - l, 0) for l, h in zip(rlo, rhi)]
    p, q = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    n = ext[p] * ext[q] if 0 <= axis <= 2 and all(ext) else 0
    top = np.zeros(n, dtype=np.uint16)
    material = np.zeros(n, dtype=np.uint32)
    info = np.zeros(1, dtype=_ffi.COLUMNS_INFO)
    rc = _ffi.host_lib().blok_column_field(_ffi.ptr(d) if d.size else None, _ffi.ptr(m) if m.size else None, _vec(origin), nx, ny, nz, _vec(lo), _vec(hi),
                                           int(axis), int(flags), _ffi.ptr(top) if n else None, _ffi.ptr(material) if n else None, _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_column_field")
    return top, material, info


def scatter_host(top, material, info, params, entries, count_only: bool = False):
    """blok_scatter over a column field (top, material, info) with one _ffi.SCATTER_PARAMS record and _ffi.SCATTER_ENTRY records.  Returns
    (instances, scatter info): a structured array of _ffi.INSTANCE in column order (None with count_only) and one _ffi.SCATTER_INFO record."""
    top = np.ascontiguousarray(top, dtype=np.uint16).reshape(-1)
    material = np.ascontiguousarray(material, dtype=np.uint32).reshape(-1)
    info = np.ascontiguousarray(info, dtype=_ffi.COLUMNS_INFO).reshape(1)
    params = np.ascontiguousarray(params, dtype=_ffi.SCATTER_PARAMS).reshape(1)
    entries = np.ascontiguousarray(entries, dtype=_ffi.SCATTER_ENTRY).reshape(-1)
    lib = _ffi.host_lib()
    out_info = np.zeros(1, dtype=_ffi.SCATTER_INFO)
    args = (_ffi.ptr(top) if top.size else None, _ffi.ptr(material) if material.size else None, _ffi.ptr(info), _ffi.ptr(params),
            _ffi.ptr(entries) if len(entries) else None, len(entries))
    rc = lib.blok_scatter(*args, None, 0, _ffi.ptr(out_info))
    if rc != 0:
        raise BlokError(rc, "blok_scatter")
    if count_only:
        return None, out_info
    table = np.zeros(int(out_info["n_placed"][0]), dtype=_ffi.INSTANCE)
    rc = lib.blok_scatter(*args, _ffi.ptr(table) if len(table) else None, len(table), _ffi.ptr(out_info))
    if rc != 0:
        raise BlokError(rc, "blok_scatter")
    return table, out_info
