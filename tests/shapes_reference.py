"""The contract of blok_hip_volume_apply_shapes (include/blok_hip.h) restated in numpy — TESTS ONLY.  Independent of the host library: the
inside rules over whole coordinate grids in int64, the operations as selections, the table as a loop over its shapes in order.  Shapes are
plain dicts built here (record() turns a list of them into _ffi.SHAPE records), so that no builder of the package is on the model's side."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi

BOX, ELLIPSOID, CAPSULE, CYLINDER = range(4)
SET, KEEP, ERASE, PAINT, REPLACE, ADD, SUBTRACT = range(7)
KINDS, OPS = (BOX, ELLIPSOID, CAPSULE, CYLINDER), (SET, KEEP, ERASE, PAINT, REPLACE, ADD, SUBTRACT)
COORD_MAX, RADIUS_MAX, SPAN_MAX, SHAPES_MAX = 1 << 17, 1024, 4096, 65536
INVALID_ARG, NO_WORLD, UNSUPPORTED = -1, -4, -5


def shape(kind, op, a=(0, 0, 0), b=(0, 0, 0), r=(0, 0, 0), material=0, match=0, value=1.0, reserved=(0, 0)):
    """All of a record's fields, in half-voxel units."""
    return dict(kind=kind, op=op, a=tuple(int(c) for c in a), b=tuple(int(c) for c in b), r=tuple(int(c) for c in r), material=int(material), match=int(match),
                value=np.float32(value), reserved=tuple(reserved))


def vbox(lo, hi, op, **kw):
    """The voxel box [lo, hi) of world voxels."""
    return shape(BOX, op, [2 * c for c in lo], [2 * c for c in hi], **kw)


def record(shapes):
    out = np.zeros(len(shapes), dtype=_ffi.SHAPE)
    for i, s in enumerate(shapes):
        for k, v in s.items():
            out[k][i] = v
    return out


def centres(origin, shape_xyz):
    """Open int64 grids (cx, cy, cz) of c = 2 w + 1 that broadcast to the [z][y][x] array of a box."""
    nx, ny, nz = shape_xyz
    return (2 * (np.arange(nx, dtype=np.int64) + origin[0])[None, None, :] + 1, 2 * (np.arange(ny, dtype=np.int64) + origin[1])[None, :, None] + 1,
            2 * (np.arange(nz, dtype=np.int64) + origin[2])[:, None, None] + 1)


def inside(s, c):
    """The inside rule over grids of centres c = (cx, cy, cz): int64 arrays, or Python integers (exact at any size)."""
    a, b, r = s["a"], s["b"], s["r"]
    if s["kind"] == BOX:
        return (a[0] <= c[0]) & (c[0] <= b[0]) & (a[1] <= c[1]) & (c[1] <= b[1]) & (a[2] <= c[2]) & (c[2] <= b[2])
    if s["kind"] == ELLIPSOID:
        dx = [c[k] - a[k] for k in range(3)]
        rr = [r[k] * r[k] for k in range(3)]
        within = (abs(dx[0]) <= r[0]) & (abs(dx[1]) <= r[1]) & (abs(dx[2]) <= r[2])
        return within & (dx[0] * dx[0] * (rr[1] * rr[2]) + dx[1] * dx[1] * (rr[0] * rr[2]) + dx[2] * dx[2] * (rr[0] * rr[1]) <= rr[0] * rr[1] * rr[2])
    d = [b[k] - a[k] for k in range(3)]
    p = [c[k] - a[k] for k in range(3)]
    q = [c[k] - b[k] for k in range(3)]
    dd = sum(v * v for v in d)
    s_ = p[0] * d[0] + p[1] * d[1] + p[2] * d[2]
    pp = p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
    qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
    rr = r[0] * r[0]
    side = pp * dd - s_ * s_ <= rr * dd
    if s["kind"] == CYLINDER:
        return (s_ >= 0) & (s_ <= dd) & side
    if dd == 0:
        return pp <= rr
    if isinstance(s_, np.ndarray):
        return np.where(s_ <= 0, pp <= rr, np.where(s_ >= dd, qq <= rr, side))
    return pp <= rr if s_ <= 0 else qq <= rr if s_ >= dd else side


def filled(d):
    with np.errstate(invalid="ignore"):
        return d > 0


def inside_box(s, origin, shape_xyz):
    """The cells of the box [origin, origin + shape_xyz) inside the shape, [z][y][x]."""
    return np.broadcast_to(inside(s, centres(origin, shape_xyz)), tuple(shape_xyz)[::-1])


def apply_one(d, m, origin, s, sel=None):
    """One shape over [z][y][x] arrays of a box at world `origin`, in place.  Returns the number of writes.  sel: inside_box of the shape, if
    the caller has it."""
    if sel is None:
        sel = inside_box(s, origin, d.shape[::-1])
    op, value, material = s["op"], np.float32(s["value"]), np.uint32(s["material"])
    f = filled(d)
    with np.errstate(invalid="ignore"):
        if op == SET:
            w = sel
            d[w], m[w] = value, material
        elif op == KEEP:
            w = sel & ~f
            d[w], m[w] = value, material
        elif op == ERASE:
            w = sel
            d[w], m[w] = np.float32(0.0), 0
        elif op == PAINT:
            w = sel & f
            m[w] = material
        elif op == REPLACE:
            w = sel & f & (m == np.uint32(s["match"]))
            m[w] = material
        elif op == ADD:
            w = sel
            d[w & (d < value)] = value                             # d < value ? value : d: a NaN or an equal value stays as it is
        else:
            w = sel
            d[w & (value < d)] = value
    return int(w.sum())


def apply(d, m, origin, shapes):
    return sum(apply_one(d, m, origin, s) for s in shapes)


def extent(s, k):
    """The rule's extent along axis k in half-voxel units, both ends included."""
    if s["kind"] == BOX:
        return s["a"][k], s["b"][k]
    if s["kind"] == ELLIPSOID:
        return s["a"][k] - s["r"][k], s["a"][k] + s["r"][k]
    return min(s["a"][k], s["b"][k]) - s["r"][0], max(s["a"][k], s["b"][k]) + s["r"][0]


def noise(shape_xyz, seed=5):
    """A pre-state with everything the operations tell apart: filled cells with several ids and densities, a filled voxel with id 0, empty cells
    holding 0, -0.0, negative and NaN densities, ids under empty cells."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape_xyz
    d = rng.choice(np.array([0.0, 0.0, -0.0, -0.75, np.nan, 0.25, 0.5, 1.0, 2.0], dtype=np.float32), size=(nz, ny, nx)).astype(np.float32)
    m = rng.integers(0, 6, size=(nz, ny, nx)).astype(np.uint32)
    return np.ascontiguousarray(d), np.ascontiguousarray(m)


def same(a, b):
    return a.tobytes() == b.tobytes()
