"""Connected components of a voxel volume on the CPU (blok_components_label): the host build of HipTracer.volume_label_components."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

FLOOR = 1 << 3          # bit of blok_component::touches for the region's -Y side: `touches & FLOOR == 0` = not standing on the floor


def label_components_host(density, origin=(0, 0, 0), lo=None, hi=None, label_capacity=None, component_capacity=None):
    """blok_components_label: the contract of HipTracer.volume_label_components on the CPU, over a [z][y][x] density array of a box at
    world `origin`; the region in world voxels, half open (both None = the whole box).  Returns (labels, records): the label array of
    the region's cells in index order (uint32, _ffi.LABEL_EMPTY for empty cells) and the records (a structured array of _ffi.COMPONENT
    sorted by label); at most `label_capacity` cells and `component_capacity` records when given.  The totals of the last call
    (n_components, n_voxels) are in label_components_host.totals."""
    lib = _ffi.host_lib()
    d = np.ascontiguousarray(density, dtype=np.float32)
    assert d.ndim == 3, "the array is [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    o = (C.c_int32 * 3)(*[int(c) for c in origin])
    rlo = None if lo is None else (C.c_int32 * 3)(*[int(c) for c in lo])
    rhi = None if hi is None else (C.c_int32 * 3)(*[int(c) for c in hi])
    n_components, n_voxels = C.c_uint64(0), C.c_uint64(0)

    def call(labels, records):
        rc = lib.blok_components_label(_ffi.ptr(d), o, nx, ny, nz, rlo, rhi, 0, None if labels is None else _ffi.ptr(labels),
                                       0 if labels is None else len(labels), None if records is None else _ffi.ptr(records),
                                       0 if records is None else len(records), C.byref(n_components), C.byref(n_voxels))
        if rc != 0:
            raise BlokError(rc, "blok_components_label")
    call(None, None)
    label_components_host.totals = (int(n_components.value), int(n_voxels.value))
    cells = 1
    for a in range(3):
        cells *= (int(hi[a]) - int(lo[a])) if lo is not None else (nx, ny, nz)[a]
    labels = np.zeros(cells if label_capacity is None else min(int(label_capacity), cells), dtype=np.uint32)
    n = int(n_components.value)
    records = np.zeros(n if component_capacity is None else min(int(component_capacity), n), dtype=_ffi.COMPONENT)
    if len(labels) or len(records):
        call(labels if len(labels) else None, records if len(records) else None)
    return labels, records
