"""Wavefront OBJ / MTL meshes (include/blok_world.h: blok_obj_load_*) as numpy arrays for HipTracer.volume_voxelize_mesh, the host
fit of a mesh into a box of voxels, and the way back: a volume's surface as merged quads (blok_quads_extract), as triangles and as OBJ."""
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


NORMAL_AXIS = (0, 0, 1, 1, 2, 2)          # of faces 0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z
PLANE_AXES = ((1, 2), (0, 2), (0, 1))     # (u, v) of a face with normal axis a


def extract_quads_host(density, material_ids, origin=(0, 0, 0), lo=None, hi=None, ignore_material: bool = False, count_only: bool = False,
                       capacity=None):
    """blok_quads_extract: the contract of HipTracer.volume_extract_quads on the CPU, over [z][y][x] arrays of a box at world `origin`.
    Returns the records (a structured array of _ffi.QUAD; at most `capacity` of them when given), or (n_quads, n_faces) with count_only.
    The totals of the last call are in extract_quads_host.totals."""
    lib = _ffi.host_lib()
    d = np.ascontiguousarray(density, dtype=np.float32)
    m = np.ascontiguousarray(material_ids, dtype=np.uint32)
    assert d.ndim == 3 and d.shape == m.shape, "arrays are [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    o = (C.c_int32 * 3)(*[int(c) for c in origin])
    rlo = None if lo is None else (C.c_int32 * 3)(*[int(c) for c in lo])
    rhi = None if hi is None else (C.c_int32 * 3)(*[int(c) for c in hi])
    flags = (_ffi.QUADS_IGNORE_MATERIAL if ignore_material else 0)
    n_quads, n_faces = C.c_uint64(0), C.c_uint64(0)

    def call(out, cap, fl):
        rc = lib.blok_quads_extract(_ffi.ptr(d), _ffi.ptr(m), o, nx, ny, nz, rlo, rhi, fl, None if out is None else _ffi.ptr(out), cap,
                                    C.byref(n_quads), C.byref(n_faces))
        if rc != 0:
            raise BlokError(rc, "blok_quads_extract")
    call(None, 0, flags | _ffi.QUADS_COUNT_ONLY)
    extract_quads_host.totals = (int(n_quads.value), int(n_faces.value))
    if count_only:
        return extract_quads_host.totals
    n = int(n_quads.value) if capacity is None else min(int(capacity), int(n_quads.value))
    out = np.zeros(n, dtype=_ffi.QUAD)
    if n:
        call(out, n, flags)
    return out


def quad_corners(quads) -> np.ndarray:
    """(n, 4, 3) int64: each quad's corners in winding order, counter-clockwise seen from outside."""
    q = np.asarray(quads)
    n = len(q)
    lo = q["lo"].astype(np.int64)
    c = np.repeat(lo[:, None, :], 4, axis=1)
    for f in range(6):
        sel = np.nonzero(q["face"] == f)[0]
        if not len(sel):
            continue
        u, v = PLANE_AXES[NORMAL_AXIS[f]]
        du, dv = q["du"][sel].astype(np.int64), q["dv"][sel].astype(np.int64)
        k1, k3 = (1, 3) if f in (0, 3, 4) else (3, 1)
        c[sel, k1, u] += du
        c[sel, 2, u] += du
        c[sel, 2, v] += dv
        c[sel, k3, v] += dv
    return c.reshape(n, 4, 3)


def quads_to_triangles(quads):
    """positions (4 n, 3) float32, triangles (2 n, 3) uint32 and materials (2 n,) uint32 in volume_voxelize_mesh's input form: the
    triangles (c0, c1, c2) and (c0, c2, c3) of every quad, vertices not shared."""
    q = np.asarray(quads)
    n = len(q)
    positions = quad_corners(q).reshape(-1, 3).astype(np.float32)
    base = (4 * np.arange(n, dtype=np.uint32))[:, None]
    triangles = np.concatenate([base + np.array([0, 1, 2], dtype=np.uint32), base + np.array([0, 2, 3], dtype=np.uint32)], axis=1).reshape(-1, 3)
    return positions, triangles.astype(np.uint32), np.repeat(q["material"].astype(np.uint32), 2)


def write_obj(path, quads, materials=None):
    """blok_quads_write_obj: the quads as a Wavefront OBJ (shared integer vertices, one `f` line per quad, `usemtl m<id>`); with a
    blok_amd.vox.MaterialLibrary also a sibling .mtl with each material's albedo."""
    lib = _ffi.host_lib()
    q = np.ascontiguousarray(quads, dtype=_ffi.QUAD)
    err = C.create_string_buffer(512)
    rc = lib.blok_quads_write_obj(os.fsencode(path), _ffi.ptr(q) if len(q) else None, len(q), None if materials is None else materials._h, err, len(err))
    if rc != 0:
        raise BlokError(rc, err.value.decode())
