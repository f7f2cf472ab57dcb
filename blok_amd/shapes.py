"""Shape tables for HipTracer.volume_apply_shapes, and their host builds (blok_shapes_check, blok_shape_bounds, blok_shapes_voxels).

Every builder returns one or more _ffi.SHAPE records; np.concatenate joins them into a table, applied in order.  The builders take WORLD
coordinates in voxels, as numbers with a fraction of 0 or one half (a voxel's centre is w + 0.5, its low corner w), and radii in voxels
likewise; the records hold them doubled, in half-voxel units, where every test is an integer test."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

BOX, ELLIPSOID, CAPSULE, CYLINDER = _ffi.SHAPE_BOX, _ffi.SHAPE_ELLIPSOID, _ffi.SHAPE_CAPSULE, _ffi.SHAPE_CYLINDER
SET, KEEP, ERASE, PAINT, REPLACE, ADD, SUBTRACT = (_ffi.SHAPE_SET, _ffi.SHAPE_KEEP, _ffi.SHAPE_ERASE, _ffi.SHAPE_PAINT, _ffi.SHAPE_REPLACE,
                                                   _ffi.SHAPE_ADD, _ffi.SHAPE_SUBTRACT)


def half(v) -> int:
    """A world coordinate or radius in voxels, a multiple of one half, in half-voxel units."""
    h = 2 * float(v)
    assert h == int(h), f"{v} is not a multiple of one half"
    return int(h)


def _record(kind, op, a, b, r, material, value, match) -> np.ndarray:
    s = np.zeros(1, dtype=_ffi.SHAPE)
    s["kind"], s["op"], s["material"], s["match"], s["value"] = kind, op, material, match, value
    s["a"][0], s["b"][0], s["r"][0] = a, b, r
    return s


def box(lo, hi, op=SET, material=0, value=1.0, match=0) -> np.ndarray:
    """The half-open voxel box [lo, hi) of world voxels."""
    return _record(BOX, op, [half(c) for c in lo], [half(c) for c in hi], (0, 0, 0), material, value, match)


def ellipsoid(centre, radii, op=SET, material=0, value=1.0, match=0) -> np.ndarray:
    return _record(ELLIPSOID, op, [half(c) for c in centre], (0, 0, 0), [half(r) for r in radii], material, value, match)


def sphere(centre, radius, op=SET, material=0, value=1.0, match=0) -> np.ndarray:
    return ellipsoid(centre, (radius, radius, radius), op, material, value, match)


def capsule(p, q, radius, op=SET, material=0, value=1.0, match=0) -> np.ndarray:
    """Everything within `radius` of the segment p -> q; p == q is the sphere."""
    return _record(CAPSULE, op, [half(c) for c in p], [half(c) for c in q], (half(radius), 0, 0), material, value, match)


def cylinder(p, q, radius, op=SET, material=0, value=1.0, match=0) -> np.ndarray:
    """The flat-ended cylinder around the segment p -> q, p != q."""
    return _record(CYLINDER, op, [half(c) for c in p], [half(c) for c in q], (half(radius), 0, 0), material, value, match)


def stroke(points, radius, op=ADD, material=0, value=1.0, match=0) -> np.ndarray:
    """A brush dragged through `points`: the capsule from each point to the next, so that the chain has no gaps.  One point is a sphere."""
    pts = [tuple(p) for p in points]
    assert pts, "a stroke needs a point"
    pairs = list(zip(pts, pts[1:])) or [(pts[0], pts[0])]
    return np.concatenate([capsule(p, q, radius, op, material, value, match) for p, q in pairs])


def _table(shapes) -> np.ndarray:
    return np.ascontiguousarray(shapes, dtype=_ffi.SHAPE).reshape(-1)


def check_host(shapes):
    """blok_shapes_check: None, or (index, message) of the first shape that breaks a limit."""
    t = _table(shapes)
    index, err = C.c_uint32(0), C.create_string_buffer(256)
    rc = _ffi.host_lib().blok_shapes_check(_ffi.ptr(t) if len(t) else None, len(t), C.byref(index), err, len(err))
    return None if rc == 0 else (int(index.value), err.value.decode())


def bounds_host(shape):
    """blok_shape_bounds: ((x0, y0, z0), (x1, y1, z1)) of one shape, world voxels, half open."""
    t = _table(shape)
    lo, hi = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    rc = _ffi.host_lib().blok_shape_bounds(_ffi.ptr(t), lo, hi)
    if rc != 0:
        raise BlokError(rc, "blok_shape_bounds")
    return tuple(lo), tuple(hi)


def apply_host(density, material_ids, origin, shapes) -> int:
    """blok_shapes_voxels over [z][y][x] arrays of a box at world `origin`, in place.  Returns the number of writes."""
    assert density.dtype == np.float32 and material_ids.dtype == np.uint32 and density.flags.c_contiguous and material_ids.flags.c_contiguous
    assert density.ndim == 3 and material_ids.shape == density.shape, "the arrays are [z][y][x] over the whole box"
    nz, ny, nx = density.shape
    t = _table(shapes)
    n = C.c_uint64(0)
    rc = _ffi.host_lib().blok_shapes_voxels(_ffi.ptr(density), _ffi.ptr(material_ids), (C.c_int32 * 3)(*[int(c) for c in origin]), nx, ny, nz,
                                            _ffi.ptr(t) if len(t) else None, len(t), C.byref(n))
    if rc != 0:
        found = check_host(t)
        raise BlokError(rc, "blok_shapes_voxels" + (f": {found[1]}" if found else ""))
    return int(n.value)
