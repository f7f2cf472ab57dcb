"""Shape tables of the shapes tests — TESTS ONLY, numpy alone.  Built from tests/shapes_reference.py's plain dicts; every case is
(tag, [shapes]) for a box given by the caller.  Coordinates below are in half-voxel units unless a name says voxels."""
from __future__ import annotations

import numpy as np

from tests import shapes_reference as R

CPU_SHAPE, CPU_ORIGIN = (40, 36, 33), (-7, 3, -20)


def c_of(w):
    """Centre of world voxel w, half-voxel units."""
    return tuple(2 * int(v) + 1 for v in w)


def kind_shape(kind, origin, dims, op, **kw):
    """One shape of `kind` well inside the box [origin, origin + dims), crossing several bricks on every axis, off the grid."""
    o = origin
    mid = tuple(o[k] + dims[k] // 2 for k in range(3))
    if kind == R.BOX:
        return R.vbox((o[0] + 4, o[1] + 5, o[2] + 5), (o[0] + dims[0] - 13, o[1] + dims[1] - 6, o[2] + dims[2] - 8), op, **kw)
    if kind == R.ELLIPSOID:
        return R.shape(kind, op, a=c_of(mid), r=(2 * (dims[0] // 2) - 9, 2 * (dims[1] // 2) - 12, 2 * (dims[2] // 2) - 15), **kw)
    a = c_of((o[0] + 8, o[1] + 9, o[2] + 10))
    b = c_of((o[0] + dims[0] - 11, o[1] + dims[1] - 14, o[2] + dims[2] - 9))
    return R.shape(kind, op, a=a, b=b, r=(13 if kind == R.CAPSULE else 15, 0, 0), **kw)


def op_fields(op):
    """material, match and value that make each op show: value above some and below other densities of noise(), match an id noise() holds."""
    return dict(material=40 + op, match=3, value={R.SET: 0.75, R.KEEP: 1.5, R.ADD: 0.5, R.SUBTRACT: 0.5}.get(op, 1.0))


def kinds_by_ops(origin, dims):
    return [(f"kind {kind} op {op}", [kind_shape(kind, origin, dims, op, **op_fields(op))]) for kind in R.KINDS for op in R.OPS]


def placements(origin, dims):
    """Centres on a voxel centre, on faces (one, two even coordinates) and on a corner (all even), for the ellipsoid and the capsule."""
    mid = c_of(tuple(origin[k] + dims[k] // 2 for k in range(3)))
    out = []
    for tag, off in (("centre", (0, 0, 0)), ("face x", (1, 0, 0)), ("edge yz", (0, 1, 1)), ("corner", (1, 1, 1))):
        a = tuple(mid[k] + off[k] for k in range(3))
        for radius in (6, 7, 9):
            out.append((f"ellipsoid on {tag} r {radius}", [R.shape(R.ELLIPSOID, R.SET, a=a, r=(radius, radius + 3, radius + 1), material=7, value=1.25)]))
            b = (a[0] + 10, a[1] - 7, a[2] + 5)
            out.append((f"capsule on {tag} r {radius}", [R.shape(R.CAPSULE, R.SET, a=a, b=b, r=(radius, 0, 0), material=8, value=1.25)]))
            out.append((f"cylinder on {tag} r {radius}", [R.shape(R.CYLINDER, R.ERASE, a=a, b=b, r=(radius, 0, 0))]))
    return out


def zero_radii(origin, dims):
    """An ellipsoid flattened to a disc, a segment and a point; a capsule and a cylinder of radius 0 along an axis through voxel centres."""
    mid = c_of(tuple(origin[k] + dims[k] // 2 for k in range(3)))
    out = [(f"ellipsoid r {r}", [R.shape(R.ELLIPSOID, R.SET, a=mid, r=r, material=9, value=2.5)])
           for r in ((0, 12, 10), (14, 0, 10), (14, 12, 0), (0, 0, 10), (14, 0, 0), (0, 12, 0), (0, 0, 0))]
    b = (mid[0] + 16, mid[1], mid[2])
    out.append(("capsule r 0", [R.shape(R.CAPSULE, R.SET, a=mid, b=b, material=9, value=2.5)]))
    out.append(("cylinder r 0", [R.shape(R.CYLINDER, R.SET, a=mid, b=b, material=9, value=2.5)]))
    out.append(("point off every centre", [R.shape(R.ELLIPSOID, R.SET, a=(mid[0] + 1, mid[1], mid[2]), material=9, value=2.5)]))      # writes nothing
    return out


FACES = ("-x", "+x", "-y", "+y", "-z", "+z")


def clipped(origin, dims, op=R.SET):
    """A sphere centred on each face of the box, a capsule through two opposite faces, a box around the whole box, and shapes wholly
    outside: [(tag, shapes)]; `outside(origin, dims)` are the ones that write nothing."""
    out = []
    hi = tuple(origin[k] + dims[k] for k in range(3))
    mid = [origin[k] + dims[k] // 2 for k in range(3)]
    for f, face in enumerate(FACES):
        w = list(mid)
        w[f // 2] = origin[f // 2] if f % 2 == 0 else hi[f // 2]
        a = tuple(2 * v for v in w)                                # on the face plane itself: an even coordinate
        out.append((f"sphere on {face}", [R.shape(R.ELLIPSOID, op, a=a, r=(11, 11, 11), **op_fields(op))]))
    out.append(("capsule through -x and +x", [R.shape(R.CAPSULE, op, a=c_of((origin[0] - 9, mid[1], mid[2])), b=c_of((hi[0] + 5, mid[1] + 3, mid[2] - 2)),
                                                      r=(9, 0, 0), **op_fields(op))]))
    out.append(("box around the box", [R.vbox([v - 3 for v in origin], [v + 2 for v in hi], op, **op_fields(op))]))
    return out


def outside(origin, dims):
    hi = tuple(origin[k] + dims[k] for k in range(3))
    return [R.vbox((hi[0], origin[1], origin[2]), (hi[0] + 9, hi[1], hi[2]), R.SET, material=5, value=1.0),      # touching +x from outside
            R.shape(R.ELLIPSOID, R.SET, a=c_of((origin[0] - 7, origin[1] + 3, origin[2] + 3)), r=(12, 12, 12), material=5, value=1.0),      # ends one centre short of -x
            R.shape(R.CAPSULE, R.ERASE, a=c_of((origin[0], origin[1] - 40, origin[2])), b=c_of((hi[0], origin[1] - 30, hi[2])), r=(20, 0, 0)),
            R.vbox((-60000, -60000, -60000), (-59000, -59990, -59990), R.ERASE)]


def order_pair(origin, dims):
    """Two overlapping shapes whose order shows: SET then PAINT differs from PAINT then SET where the SET fills an empty cell."""
    mid = c_of(tuple(origin[k] + dims[k] // 2 for k in range(3)))
    return [R.shape(R.ELLIPSOID, R.SET, a=mid, r=(15, 13, 11), material=21, value=1.0),
            R.shape(R.CAPSULE, R.PAINT, a=(mid[0] - 12, mid[1] + 2, mid[2]), b=(mid[0] + 18, mid[1] - 6, mid[2] + 4), r=(8, 0, 0), material=22)]


LONG_CYCLE = (R.SET, R.PAINT, R.REPLACE, R.SUBTRACT, R.ADD, R.ERASE, R.KEEP, R.PAINT)
LONG_PER_ROW = 26


def long_list(origin, d, m, n=130):
    """n shapes that all lie in one tile (the 64 x 4 x 4 cells at the box's corner), so that its list takes three rounds of 64, and a
    pre-state written into the [z][y][x] arrays d, m under them, made so that every shape's place in the order shows in the result.
    Shape i is the run of 3 cells [2 k, 2 k + 3) of row i // 26 of the tile, k = i % 26: its first cell is shared with shape i - 1 alone,
    its middle cell is its own, its last cell is shared with shape i + 1 alone (the first and the last shape of a row share with nobody).
    The operations go round LONG_CYCLE, in which no two neighbours commute on a cell that holds what the later comments ask:
      SET, PAINT: anything.  PAINT p, REPLACE p -> y: a filled cell whose id is not p.  REPLACE p -> y, SUBTRACT -1: a filled cell with id p.
      SUBTRACT -1, ADD v: anything.  ADD v, ERASE: anything.  ERASE, KEEP: anything.  KEEP, PAINT q: an empty cell.  PAINT q, SET: anything.
    and each shape alone changes its own cell: PAINT and REPLACE find a filled cell with another / the matched id, KEEP an empty one, ADD a
    density below its value, SUBTRACT one above, ERASE something to erase."""
    p, q, y = 60, 61, 62
    out = []
    for i in range(n):
        row, k = divmod(i, LONG_PER_ROW)
        ry, rz = row % 4, row // 4
        c = i % len(LONG_CYCLE)
        op = LONG_CYCLE[c]
        value = {R.SUBTRACT: -1.0, R.ADD: 1.75, R.KEEP: 0.5}.get(op, 0.25 + 0.01 * i)
        material = {1: p, 2: y, 7: q}.get(c, 100 + i)
        out.append(R.vbox((origin[0] + 2 * k, origin[1] + ry, origin[2] + rz), (origin[0] + 2 * k + 3, origin[1] + ry + 1, origin[2] + rz + 1), op, material=material, match=p,
                          value=value))
        shared, own = (rz, ry, 2 * k + 2), (rz, ry, 2 * k + 1)
        d[shared], m[shared] = {1: (1.0, 2), 2: (1.0, p), 3: (0.5, 4), 6: (0.0, 3)}.get(c, (d[shared], m[shared]))      # (3: not a NaN, which neither changes)
        d[own], m[own] = {1: (1.0, 2), 2: (1.0, p), 3: (0.5, 4), 4: (0.5, 4), 5: (1.0, 4), 6: (-0.0, 3), 7: (2.0, 2)}.get(c, (d[own], m[own]))
    return out


def stroke(origin, dims, op, n=40, radius=7, **kw):
    """n capsules in a chain that winds through the box across tile boundaries on all three axes."""
    t = np.linspace(0.0, 1.0, n + 1)
    pts = [c_of((origin[0] + 4 + (dims[0] - 9) * u, origin[1] + dims[1] / 2 + (dims[1] / 2 - 5) * np.sin(7 * u), origin[2] + 4 + (dims[2] - 9) * (0.5 - 0.5 * np.cos(5 * u))))
           for u in t]
    return [R.shape(R.CAPSULE, op, a=p, b=q, r=(radius, 0, 0), **kw) for p, q in zip(pts, pts[1:])]


def bad_shapes():
    """[(text in the message, shape)], each breaking one limit."""
    good = dict(a=(1, 1, 1), b=(9, 9, 9))
    top = R.COORD_MAX
    return [("unknown kind", R.shape(4, R.SET, **good)), ("unknown op", R.shape(R.BOX, 7, **good)),
            ("reserved", R.shape(R.BOX, R.SET, reserved=(0, 1), **good)), ("reserved", R.shape(R.BOX, R.SET, reserved=(5, 0), **good)),
            ("outside [-2^17, 2^17]", R.shape(R.BOX, R.SET, a=(1, 1, 1), b=(9, top + 1, 9))), ("outside [-2^17, 2^17]", R.shape(R.ELLIPSOID, R.SET, a=(1, -top - 1, 1), r=(1, 1, 1))),
            ("radius above 1024", R.shape(R.ELLIPSOID, R.SET, a=(1, 1, 1), r=(4, 1025, 4))), ("radius above 1024", R.shape(R.CAPSULE, R.SET, r=(1025, 0, 0), **good)),
            ("does not use", R.shape(R.BOX, R.SET, r=(0, 0, 1), **good)), ("does not use", R.shape(R.ELLIPSOID, R.SET, a=(1, 1, 1), b=(0, 1, 0), r=(2, 2, 2))),
            ("does not use", R.shape(R.CAPSULE, R.SET, r=(3, 1, 0), **good)), ("does not use", R.shape(R.CYLINDER, R.SET, r=(3, 0, 2), **good)),
            ("a > b", R.shape(R.BOX, R.SET, a=(1, 10, 1), b=(9, 9, 9))),
            ("above 4096", R.shape(R.CAPSULE, R.SET, a=(0, 0, 0), b=(0, 4097, 0), r=(1, 0, 0))), ("above 4096", R.shape(R.CYLINDER, R.SET, a=(0, 0, 5), b=(1, 0, -4093), r=(1, 0, 0))),
            ("a == b", R.shape(R.CYLINDER, R.SET, a=(3, 3, 3), b=(3, 3, 3), r=(2, 0, 0))),
            ("not finite", R.shape(R.BOX, R.ERASE, value=np.nan, **good)), ("not finite", R.shape(R.BOX, R.ADD, value=np.inf, **good)),
            ("not finite", R.shape(R.BOX, R.PAINT, value=-np.inf, **good)),
            ("> 0 for SET and KEEP", R.shape(R.BOX, R.SET, value=0.0, **good)), ("> 0 for SET and KEEP", R.shape(R.BOX, R.KEEP, value=-1.0, **good))]
