"""Independent reference of blok_hip_volume_voxelize_mesh (include/blok_hip.h), written from the contract in exact integer arithmetic.

Coordinates snap to q = round_half_even(x * 256) (Fraction, so the float's exact value is rounded).  A voxel is on the surface iff its
closed cube meets the closed triangle: no axis among the box normals, the triangle normal and the edge x box-axis products separates
the eight cube corners from the three vertices (projections compared corner by corner).  A column counts a triangle iff the column point,
moved by (+e, -e^2) with e -> 0, lies strictly inside the counter-clockwise projection: the first non-zero of (E, -dz, -dy) per edge is
positive.  The crossing is a Fraction."""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def snap(positions) -> np.ndarray:
    p = np.asarray(positions, dtype=np.float32)
    return np.array([round(Fraction(float(x)) * 256) for x in p.reshape(-1)], dtype=np.int64).reshape(p.shape)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def surface_voxels(q3, origin, shape):
    """S of one snapped triangle q3 (3, 3) inside the box: a list of (x, y, z) box-local, and the boolean block it came from."""
    v0 = [int(c) for c in q3[0]]
    w = [[int(q3[k][c]) - v0[c] for c in range(3)] for k in range(3)]         # w[0] = 0
    lo, hi = [], []
    for c in range(3):
        a, b = min(w[k][c] for k in range(3)) + v0[c], max(w[k][c] for k in range(3)) + v0[c]
        lo.append(max(-((-(a)) // 256) - 1 - origin[c], 0))          # voxels whose [i, i+1] meets [a, b]
        hi.append(min(b // 256 - origin[c], shape[c] - 1))
    if any(lo[c] > hi[c] for c in range(3)):
        return []
    axes = [[1, 0, 0], [0, 1, 0], [0, 0, 1], _cross(w[1], w[2])]
    edges = [w[1], [w[2][c] - w[1][c] for c in range(3)], [-w[2][c] for c in range(3)]]
    for e in edges:
        for u in ([1, 0, 0], [0, 1, 0], [0, 0, 1]):
            axes.append(_cross(e, u))
    xs = np.arange(lo[0], hi[0] + 1, dtype=np.int64)
    ys = np.arange(lo[1], hi[1] + 1, dtype=np.int64)
    zs = np.arange(lo[2], hi[2] + 1, dtype=np.int64)
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    base = [256 * (X + origin[0]) - v0[0], 256 * (Y + origin[1]) - v0[1], 256 * (Z + origin[2]) - v0[2]]
    keep = np.ones(X.shape, dtype=bool)
    for a in axes:
        if a == [0, 0, 0]:
            continue
        tp = [sum(a[c] * w[k][c] for c in range(3)) for k in range(3)]
        tmin, tmax = min(tp), max(tp)
        cmin = cmax = None
        for corner in range(8):
            d = [(corner >> c) & 1 for c in range(3)]
            proj = sum(np.int64(a[c]) * (base[c] + 256 * d[c]) for c in range(3))
            cmin = proj if cmin is None else np.minimum(cmin, proj)
            cmax = proj if cmax is None else np.maximum(cmax, proj)
        keep &= ~((cmax < tmin) | (cmin > tmax))
    idx = np.nonzero(keep)
    return list(zip(X[idx].tolist(), Y[idx].tolist(), Z[idx].tolist()))


def _column_counts(q3, Yq, Zq):
    """Does the column point (Yq, Zq) (snapped) count this triangle?  The perturbed-point rule."""
    p = [(int(q3[k][1]), int(q3[k][2])) for k in range(3)]
    area = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0])
    if area == 0:
        return False
    if area < 0:
        p = [p[0], p[2], p[1]]
    for k in range(3):
        a, b = p[k], p[(k + 1) % 3]
        dy, dz = b[0] - a[0], b[1] - a[1]
        E = dy * (Zq - a[1]) - dz * (Yq - a[0])
        first = next((s for s in (E, -dz, -dy) if s != 0), 0)
        if first <= 0:
            return False
    return True


def voxelize(positions, triangles, origin, shape, materials=None, material=1, solid=False):
    """(filled bool [z][y][x], ids uint32 [z][y][x] of the written voxels, 0 elsewhere)."""
    q = snap(positions)
    tris = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nx, ny, nz = shape
    owner = np.full((nz, ny, nx), -1, dtype=np.int64)
    for i, t in enumerate(tris):
        for (x, y, z) in surface_voxels(q[t], origin, shape):
            if owner[z, y, x] < 0:
                owner[z, y, x] = i
    filled = owner >= 0
    ids = np.zeros((nz, ny, nx), dtype=np.uint32)
    mats = None if materials is None else np.asarray(materials, dtype=np.uint32)
    ids[filled] = material if mats is None else mats[owner[filled]]
    if solid:
        toggles = np.zeros((nz, ny, nx + 1), dtype=np.uint8)
        for t in tris:
            q3 = q[t]
            ylo, yhi = int(q3[:, 1].min()), int(q3[:, 1].max())
            zlo, zhi = int(q3[:, 2].min()), int(q3[:, 2].max())
            for k in range(nz):
                Zq = 256 * (k + origin[2]) + 128
                if not zlo <= Zq <= zhi:
                    continue
                for j in range(ny):
                    Yq = 256 * (j + origin[1]) + 128
                    if not ylo <= Yq <= yhi or not _column_counts(q3, Yq, Zq):
                        continue
                    v0 = [int(c) for c in q3[0]]
                    n = _cross([int(q3[1][c]) - v0[c] for c in range(3)], [int(q3[2][c]) - v0[c] for c in range(3)])
                    X = Fraction(v0[0]) - Fraction(n[1] * (Yq - v0[1]) + n[2] * (Zq - v0[2]), n[0])
                    # first voxel whose centre 256 (i + ox) + 128 >= X
                    i = -((-(X - 128 - 256 * origin[0])) // 256)
                    i = max(int(i), 0)
                    if i < nx:
                        toggles[k, j, i] ^= 1
        interior = (np.cumsum(toggles[:, :, :nx], axis=2) & 1).astype(bool)
        only = interior & ~filled
        ids[only] = material
        filled = filled | interior
    return filled, ids
