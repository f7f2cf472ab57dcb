"""The expected records of world + instances + posed models (include/blok_hip.h, "Posed models"), from the existing oracle alone — TESTS ONLY.

Per pose: the model alone in an oracle ChunkManager at its own voxel size (tests/instance_oracle.OracleModel through
tests/scaled_instance_oracle.scaled_model), the rays moved into its local space in numpy float32 in exactly the specified order of operations
(every numpy float32 operation rounds once; nothing is fused), the oracle's trace, the records kept as they are (local voxel, local face),
then composed on top of scaled_instance_oracle.compose's output by the tie rule."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from blok_amd._ffi import POSE, POSE_ID
from tests import instance_oracle as IO


def pose(model, m, pivot, local):
    rec = np.zeros(1, dtype=POSE)
    rec["model"] = model
    rec["m"] = np.asarray(m, dtype=np.float32)
    rec["pivot"] = np.asarray(pivot, dtype=np.float32)
    rec["local"] = np.asarray(local, dtype=np.float32)
    return rec[0]


def local_rays(rays, p):
    """(local rays, usable mask).  r_j = fl(o_j - pivot_j); o'_k = fl(fl(fl(fl(m_k0 r_0) + fl(m_k1 r_1)) + fl(m_k2 r_2)) + local_k);
    d'_k = fl(fl(fl(m_k0 d_0) + fl(m_k1 d_1)) + fl(m_k2 d_2)); tmin, tmax unchanged.  A ray with a non-finite component is masked out (and
    replaced by one that can hit nothing, so that the oracle never sees a NaN)."""
    out = rays.copy()
    m = np.asarray(p["m"], dtype=np.float32)
    o = rays["org"].astype(np.float32)
    d = rays["dir"].astype(np.float32)
    with np.errstate(all="ignore"):
        r = [o[:, j] - np.float32(p["pivot"][j]) for j in range(3)]
        for k in range(3):
            acc = (m[k, 0] * r[0]) + (m[k, 1] * r[1])
            acc = acc + (m[k, 2] * r[2])
            out["org"][:, k] = acc + np.float32(p["local"][k])
            acc = (m[k, 0] * d[:, 0]) + (m[k, 1] * d[:, 1])
            out["dir"][:, k] = acc + (m[k, 2] * d[:, 2])
    assert out["org"].dtype == np.float32 and out["dir"].dtype == np.float32
    ok = np.isfinite(out["org"]).all(axis=1) & np.isfinite(out["dir"]).all(axis=1)
    out["org"][~ok] = 0.0
    out["dir"][~ok] = (1.0, 0.0, 0.0)
    out["tmax"][~ok] = out["tmin"][~ok]
    return out, ok


def candidates(rays, p, models):
    """The pose's own records for the rays (local voxel, local face), misses where the ray does not enter the pose."""
    lr, ok = local_rays(rays, p)
    cand = models[int(p["model"])].trace(lr)
    cand["hit"][~ok] = 0
    return cand


def compose(best, ids, rays, poses, models, per_pose=None):
    """(records, ids) of `best` / `ids` (scaled_instance_oracle.compose's output, or the world's records and INSTANCE_NONE) composed with
    the poses in index order.  models[m]: the oracle's copy of model m at ITS voxel size vs * 2^e.  per_pose: a list that receives each
    pose's own hit mask."""
    best = best.copy()
    ids = ids.copy()
    for j, p in enumerate(poses):
        cand = candidates(rays, p, models)
        if per_pose is not None:
            per_pose.append(cand["hit"] == 1)
        take = (cand["hit"] == 1) & ((best["hit"] == 0) | (cand["t"] < best["t"]))
        best[take] = cand[take]
        ids[take] = POSE_ID | j
    return best, ids


def shade_face(p, face):
    """The world face the frame shades local face 2k + n by: of s * row k of m the component of largest magnitude (ties: the lowest axis),
    2a for a component >= 0, 2a + 1 for one < 0."""
    k, n = int(face) >> 1, int(face) & 1
    v = (np.float32(-1.0) if n else np.float32(1.0)) * np.asarray(p["m"], dtype=np.float32)[k]
    a = np.abs(v)
    if a[0] >= a[1] and a[0] >= a[2]:
        axis = 0
    elif a[1] >= a[2]:
        axis = 1
    else:
        axis = 2
    return 2 * axis + (1 if v[axis] < 0 else 0)


def shade(hits, ids, poses, materials):
    """RGBA8 of composed records: instance_oracle.shade, with the shade face for the pixels a pose won."""
    h = hits.copy()
    won = np.flatnonzero((ids != 0xFFFFFFFF) & ((ids & POSE_ID) != 0) & (hits["hit"] == 1))
    for i in won:
        h["face"][i] = shade_face(poses[int(ids[i]) & 0x7FFFFFFF], hits["face"][i])
    return IO.shade(h, materials)


def preimage_box(p, lo, hi, voxel_size):
    """The exact bounding box (lo[3], hi[3] as Fractions, world units) of the preimage of the model's box [lo, hi) * vs (lo, hi in WORLD voxels
    from the local origin, as the store's descriptor holds them), w = pivot + m^-1 (c - local); None when m is singular."""
    m = [[Fraction(float(x)) for x in row] for row in np.asarray(p["m"], dtype=np.float32)]
    det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
           + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    if det == 0:
        return None
    inv = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            inv[j][i] = (m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]) / det
    vs = Fraction(float(voxel_size))
    pivot = [Fraction(float(x)) for x in p["pivot"]]
    local = [Fraction(float(x)) for x in p["local"]]
    blo, bhi = [None] * 3, [None] * 3
    for c in range(8):
        corner = [(Fraction(int(hi[k])) if (c >> k) & 1 else Fraction(int(lo[k]))) * vs - local[k] for k in range(3)]
        for j in range(3):
            w = pivot[j] + sum(inv[j][k] * corner[k] for k in range(3))
            blo[j] = w if blo[j] is None else min(blo[j], w)
            bhi[j] = w if bhi[j] is None else max(bhi[j], w)
    return blo, bhi
