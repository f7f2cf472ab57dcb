"""Wavefront OBJ / MTL meshes (include/blok_world.h: blok_obj_load_*) as numpy arrays for HipTracer.volume_voxelize_mesh, and the host
fit of a mesh into a box of voxels."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _ffi
from ._ffi import BlokError


class ObjMesh:
    """positions (n, 3) float32, triangles (m, 3) uint32, materials (m,) uint32 (ids of the given MaterialLibrary; 0 without one)."""

    def __init__(self, positions: np.ndarray, triangles: np.ndarray, materials: np.ndarray):
        self.positions, self.triangles, self.materials = positions, triangles, materials

    @staticmethod
    def _take(lib, h: C.c_void_p) -> "ObjMesh":
        try:
            nv, nt = int(lib.blok_mesh_vertex_count(h)), int(lib.blok_mesh_triangle_count(h))

            def copy(ptr, count, dtype):
                if count == 0:
                    return np.zeros(0, dtype=dtype)
                return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype, count=count).copy()
            return ObjMesh(copy(lib.blok_mesh_positions(h), 3 * nv, np.float32).reshape(-1, 3),
                           copy(lib.blok_mesh_triangles(h), 3 * nt, np.uint32).reshape(-1, 3),
                           copy(lib.blok_mesh_materials(h), nt, np.uint32))
        finally:
            lib.blok_mesh_free(h)

    @staticmethod
    def load_file(path, materials=None) -> "ObjMesh":
        """materials: a blok_amd.vox.MaterialLibrary that the MTL's materials are added to (add_or_find), or None."""
        lib = _ffi.host_lib()
        h, err = C.c_void_p(), C.create_string_buffer(512)
        rc = lib.blok_obj_load_file(os.fsencode(path), None if materials is None else materials._h, C.byref(h), err, len(err))
        if rc != 0:
            raise BlokError(rc, err.value.decode())
        return ObjMesh._take(lib, h)

    @staticmethod
    def load_memory(obj, mtl=None, materials=None) -> "ObjMesh":
        """obj / mtl: text (str or bytes); mtl stands for the library `mtllib` names."""
        lib = _ffi.host_lib()
        o = obj.encode() if isinstance(obj, str) else bytes(obj)
        m = None if mtl is None else (mtl.encode() if isinstance(mtl, str) else bytes(mtl))
        h, err = C.c_void_p(), C.create_string_buffer(512)
        rc = lib.blok_obj_load_memory(o, len(o), m, 0 if m is None else len(m), None if materials is None else materials._h, C.byref(h), err, len(err))
        if rc != 0:
            raise BlokError(rc, err.value.decode())
        return ObjMesh._take(lib, h)


def fit_to_box(positions, lo, size) -> np.ndarray:
    """A uniform scale and offset (on the host, in float64) that puts the mesh's bounding box inside the voxels [lo, lo + size) on every
    axis, half a voxel from the box's faces, centred on the axes where it is shorter.  Returns float32 positions."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    if len(p) == 0:
        return p.astype(np.float32)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (3,))
    size = float(size)
    pmin, pmax = p.min(axis=0), p.max(axis=0)
    extent = float((pmax - pmin).max())
    scale = (size - 1.0) / extent if extent > 0 else 1.0
    centre = lo + size / 2.0
    return ((p - (pmin + pmax) / 2.0) * scale + centre).astype(np.float32)
