"""Procedural closed meshes for the voxelizer tests: (positions (n, 3) float32, triangles (m, 3) uint32), outward winding."""
from __future__ import annotations

import numpy as np


def box(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    p = np.array([[hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]] for i in range(8)], dtype=np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = []
    for a, b, c, d in quads:
        t += [(a, b, c), (a, c, d)]
    return p, np.array(t, dtype=np.uint32)


def icosphere(center, radius, subdivisions=2, displace=None):
    g = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    faces = np.array(f, dtype=np.int64)
    for _ in range(subdivisions):
        cache, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                cache[key] = len(verts) - 1
            return cache[key]
        for a, b, c in faces.tolist():
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = np.array(out, dtype=np.int64)
    V = np.array(verts)
    r = radius if displace is None else radius * (1.0 + displace(V))[:, None]
    return (np.asarray(center, dtype=np.float64) + V * r).astype(np.float32), faces.astype(np.uint32)


def torus(center, R, r, n=24, m=12):
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    u, v = 2 * np.pi * i / n, 2 * np.pi * j / m
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    t = []
    for a in range(n):
        for b in range(m):
            p00, p10, p01, p11 = a * m + b, ((a + 1) % n) * m + b, a * m + (b + 1) % m, ((a + 1) % n) * m + (b + 1) % m
            t += [(p00, p10, p11), (p00, p11, p01)]
    return (p + np.asarray(center)).astype(np.float32), np.array(t, dtype=np.uint32)


def octahedron(center, radius):
    c = np.asarray(center, dtype=np.float64)
    p = np.array([c + d for d in ([radius, 0, 0], [-radius, 0, 0], [0, radius, 0], [0, -radius, 0], [0, 0, radius], [0, 0, -radius])], dtype=np.float32)
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return p, np.array(t, dtype=np.uint32)


def merge(*meshes):
    ps, ts, base = [], [], 0
    for p, t in meshes:
        ps.append(p)
        ts.append(t + base)
        base += len(p)
    return np.concatenate(ps).astype(np.float32), np.concatenate(ts).astype(np.uint32)
