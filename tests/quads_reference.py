"""Independent reference of blok_hip_volume_extract_quads / blok_quads_extract (include/blok_hip.h), written from the contract with numpy.

Per face number: the key array K over the region (0 = not exposed, key + 1 otherwise) in [plane][v][u] order; run starts and ends are
where K differs from its u - 1 / u + 1 neighbour (nothing outside the region); a row's runs are the set of (first, last, key) triples;
a quad starts at a run that the row below does not hold and is as tall as the number of consecutive rows that hold it."""
from __future__ import annotations

import hashlib

import numpy as np

NORMAL_AXIS = (0, 0, 1, 1, 2, 2)          # faces 0:+X 1:-X 2:+Y 3:-Y 4:+Z 5:-Z
PLANE_AXES = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
DTYPE = np.dtype([("lo", "<i4", 3), ("du", "<u4"), ("dv", "<u4"), ("material", "<u4"), ("face", "<u4"), ("reserved", "<u4")])


def filled(density) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.asarray(density) > 0          # NaN > 0 is False


def exposure(density, face: int) -> np.ndarray:
    """[z][y][x] bool over the whole box: face `face` of the voxel is exposed (neighbours outside the box are empty)."""
    f = filled(density)
    axis = 2 - NORMAL_AXIS[face]                # array axis of the normal
    nb = np.zeros_like(f)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if face % 2 == 0:
        dst[axis], src[axis] = slice(0, -1), slice(1, None)
    else:
        dst[axis], src[axis] = slice(1, None), slice(0, -1)
    nb[tuple(dst)] = f[tuple(src)]
    return f & ~nb


def _region(shape_zyx, origin, lo, hi):
    nz, ny, nx = shape_zyx
    lo = list(origin) if lo is None else list(lo)
    hi = [origin[0] + nx, origin[1] + ny, origin[2] + nz] if hi is None else list(hi)
    return lo, hi, [lo[a] - origin[a] for a in range(3)], [hi[a] - origin[a] for a in range(3)]


def extract(density, ids, origin=(0, 0, 0), lo=None, hi=None, ignore_material=False):
    """Returns (records in canonical order as a DTYPE array, n_faces)."""
    density, ids = np.asarray(density), np.asarray(ids)
    lo, hi, r0, r1 = _region(density.shape, origin, lo, hi)
    records = []
    n_faces = 0
    for face in range(6):
        a = NORMAL_AXIS[face]
        u, v = PLANE_AXES[a]
        key = np.where(exposure(density, face), (0 if ignore_material else ids.astype(np.int64)) + 1, 0)
        K = np.transpose(key, (2 - a, 2 - v, 2 - u))[r0[a]:r1[a], r0[v]:r1[v], r0[u]:r1[u]]
        n_faces += int(np.count_nonzero(K))
        if K.size == 0:
            continue
        left = np.zeros_like(K); left[:, :, 1:] = K[:, :, :-1]
        right = np.zeros_like(K); right[:, :, :-1] = K[:, :, 1:]
        starts, ends = (K != 0) & (K != left), (K != 0) & (K != right)
        for s in np.nonzero(K.any(axis=(1, 2)))[0]:
            rows = []
            for vv in range(K.shape[1]):
                u0, u1 = np.nonzero(starts[s, vv])[0], np.nonzero(ends[s, vv])[0]
                rows.append({(int(b), int(e), int(K[s, vv, b])) for b, e in zip(u0, u1)})
            for vv, row in enumerate(rows):
                for (b, e, k) in sorted(row):
                    if vv > 0 and (b, e, k) in rows[vv - 1]:
                        continue
                    dv = 1
                    while vv + dv < len(rows) and (b, e, k) in rows[vv + dv]:
                        dv += 1
                    c = [0, 0, 0]
                    c[a] = lo[a] + int(s) + (1 if face % 2 == 0 else 0)
                    c[u] = lo[u] + b
                    c[v] = lo[v] + vv
                    records.append((c, e - b + 1, dv, k - 1, face, 0))
    out = np.zeros(len(records), dtype=DTYPE)
    for i, r in enumerate(records):
        out[i] = (r[0], r[1], r[2], r[3], r[4], r[5])
    order = sorted(range(len(out)), key=lambda i: canonical_key(out[i]))
    assert order == list(range(len(out))), "the construction order is the canonical order"
    return out, n_faces


def canonical_key(q):
    a = NORMAL_AXIS[int(q["face"])]
    u, v = PLANE_AXES[a]
    return (int(q["face"]), int(q["lo"][a]), int(q["lo"][v]), int(q["lo"][u]))


def digest(quads) -> str:
    """SHA-256 over the records packed little-endian as <3i5I in the given order."""
    q = np.ascontiguousarray(quads, dtype=DTYPE)
    return hashlib.sha256(q.tobytes()).hexdigest()


def corners(q):
    """The four corners of one record in winding order (counter-clockwise seen from outside), int64 (4, 3)."""
    face = int(q["face"])
    a = NORMAL_AXIS[face]
    u, v = PLANE_AXES[a]
    eu = np.zeros(3, np.int64); eu[u] = int(q["du"])
    ev = np.zeros(3, np.int64); ev[v] = int(q["dv"])
    n = np.zeros(3, np.int64); n[a] = 1 if face % 2 == 0 else -1
    c = np.asarray(q["lo"], dtype=np.int64)
    cs = [c, c + eu, c + eu + ev, c + ev]
    if int(np.dot(np.cross(eu, ev), n)) < 0:
        cs = [cs[0], cs[3], cs[2], cs[1]]
    return np.array(cs)


def signed_volume6(quads) -> int:
    """Sum over the triangles (c0, c1, c2), (c0, c2, c3) of p0 . (p1 x p2): six times the enclosed volume of a closed mesh."""
    total = 0
    for q in quads:
        c = corners(q)
        for p0, p1, p2 in ((c[0], c[1], c[2]), (c[0], c[2], c[3])):
            total += int(np.dot(p0, np.cross(p1, p2)))
    return total


def rasterise(quads, shape_zyx, origin):
    """The unit faces the quads cover: per face number a [z][y][x] int array of how often the voxel's face is covered, and its key."""
    nz, ny, nx = shape_zyx
    cover = np.zeros((6, nz, ny, nx), dtype=np.int32)
    key = np.zeros((6, nz, ny, nx), dtype=np.int64)
    for q in quads:
        face = int(q["face"])
        a = NORMAL_AXIS[face]
        u, v = PLANE_AXES[a]
        p0 = [int(q["lo"][c]) - origin[c] for c in range(3)]
        p0[a] -= 1 if face % 2 == 0 else 0
        p1 = list(p0)
        p1[a] += 1; p1[u] += int(q["du"]); p1[v] += int(q["dv"])
        cover[face, p0[2]:p1[2], p0[1]:p1[1], p0[0]:p1[0]] += 1
        key[face, p0[2]:p1[2], p0[1]:p1[1], p0[0]:p1[0]] = int(q["material"])
    return cover, key
