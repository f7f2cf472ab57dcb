"""Emissive models as lights (include/blok_hip.h, "emissive models as lights") in plain numpy — TESTS ONLY.

The model's table as a SET of (voxel, face, material) from a dense boolean array and six shifts, its order from the tree's key restated
here, the rectangle of an instance's face from the world voxels tests/instance_oracle.py maps a cell to, and the prefix rule of an
instance table with its overflow rule.  Nothing here calls the library."""
from __future__ import annotations

import numpy as np

from blok_amd._ffi import LIGHT

NORMALS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))      # faces 0..5: +X -X +Y -Y +Z -Z


def material_index(ids, n_materials):
    c = np.minimum(np.asarray(ids, dtype=np.int64), 65535)
    return np.where(c < n_materials, c, 0)


def glows(materials):
    """The emissive indices of a material table: dot(e, 1) > 0.01 in float32, summed left to right."""
    e = materials["emission"].astype(np.float32)
    return ((e[:, 0] + e[:, 1]) + e[:, 2]) > np.float32(0.01)


def last_wins(xyz, ids):
    """The voxel list as model_create reads it: of duplicates the last one."""
    seen = {}
    for p, m in zip(np.asarray(xyz).reshape(-1, 3).tolist(), np.asarray(ids).tolist()):
        seen[tuple(p)] = m
    pts = np.array(list(seen.keys()), dtype=np.int64).reshape(-1, 3)
    return pts, np.array(list(seen.values()), dtype=np.int64)


def model_faces(xyz, ids, materials):
    """The set of (x, y, z, face, material id) of the model's exposed emissive unit faces."""
    pts, mats = last_wins(xyz, ids)
    lo = pts.min(axis=0)
    ext = pts.max(axis=0) - lo + 3                       # a one-cell margin of empty cells all round
    filled = np.zeros(tuple(ext), dtype=bool)
    mat = np.zeros(tuple(ext), dtype=np.int64)
    q = pts - lo + 1
    filled[q[:, 0], q[:, 1], q[:, 2]] = True
    mat[q[:, 0], q[:, 1], q[:, 2]] = mats
    g = glows(materials)
    glowing = filled & g[material_index(mat, min(len(materials), 65536))]
    out = set()
    for f, n in enumerate(NORMALS):
        neighbour = np.roll(filled, tuple(-c for c in n), axis=(0, 1, 2))        # neighbour[p] = filled[p + n] (the margin keeps the wrap empty)
        for p in np.argwhere(glowing & ~neighbour):
            w = p + lo - 1
            out.add((int(w[0]), int(w[1]), int(w[2]), f, int(mat[tuple(p)])))
    return out


def tree_order_key(xyz):
    """The position of a voxel in the model's material array: the tree's key, 2-bit digits of the voxel from the tree's origin (each axis
    of the lowest voxel floored to a multiple of 16), the most significant digit first, x the lowest bits of a digit."""
    pts = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    origin = (pts.min(axis=0) // 16) * 16
    r = pts - origin
    key = np.zeros(len(pts), dtype=np.int64)
    for level in range(8):
        digit = ((r[:, 0] >> (2 * level)) & 3) | (((r[:, 1] >> (2 * level)) & 3) << 2) | (((r[:, 2] >> (2 * level)) & 3) << 4)
        key |= digit << (6 * level)
    return key


def table_of(xyz, ids, materials):
    """The LIGHT records of the model's table in their order: the set above sorted by (tree key of the voxel, face)."""
    faces = sorted(model_faces(xyz, ids, materials))
    if not faces:
        return np.zeros(0, dtype=LIGHT)
    pts, _ = last_wins(xyz, ids)
    origin = (pts.min(axis=0) // 16) * 16
    v = np.array([f[:3] for f in faces], dtype=np.int64)
    r = v - origin
    key = np.zeros(len(v), dtype=np.int64)
    for level in range(8):
        digit = ((r[:, 0] >> (2 * level)) & 3) | (((r[:, 1] >> (2 * level)) & 3) << 2) | (((r[:, 2] >> (2 * level)) & 3) << 4)
        key |= digit << (6 * level)
    order = np.lexsort((np.array([f[3] for f in faces]), key))
    t = np.zeros(len(faces), dtype=LIGHT)
    for at, i in enumerate(order):
        x, y, z, f, m = faces[i]
        t["lo"][at] = (x + (f == 0), y + (f == 2), z + (f == 4))
        t["face"][at], t["material"][at] = f, m
    t["du"] = t["dv"] = 1
    t["cum"] = np.arange(len(t))
    return t


def rectangle_voxels(light):
    """(the set of world voxels that carry the rectangle as one of their faces, the face number)."""
    f = int(light["face"])
    a = f >> 1
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    lo = [int(c) for c in light["lo"]]
    plane = lo[a] - 1 if f % 2 == 0 else lo[a]
    out = set()
    for iu in range(int(light["du"])):
        for iv in range(int(light["dv"])):
            p = [0, 0, 0]
            p[a], p[u], p[v] = plane, lo[u] + iu, lo[v] + iv
            out.add(tuple(p))
    return out, f


# ---- the prefix of an instance table -------------------------------------------------------------------------------------------------------
def usable(inst, model, vs=1.0):
    """The kernels' instance_usable with the store's voxel-size limit: model = dict(lo, hi: the box in its own voxels; e; live)."""
    axis = [int(a) for a in inst["axis"]]
    if sorted(axis) != [0, 1, 2] or int(inst["flip"]) >= 8 or any(int(r) for r in inst["reserved"]):
        return False
    if model is None or not model["live"] or vs * 2.0 ** model["e"] > 256.0:
        return False
    for a in range(3):
        k = axis.index(a)
        o = int(inst["offset"][a])
        mlo, mhi = int(model["lo"][k]) << model["e"], int(model["hi"][k]) << model["e"]
        lo, hi = (o - mhi, o - mlo) if (int(inst["flip"]) >> k) & 1 else (o + mlo, o + mhi)
        if lo < -32768 or hi > 32768:
            return False
    return True


def prefix(instances, models, a_world=0, vs=1.0):
    """(icum as n + 1 uint32 words, dict of the header) — models: id -> dict(lo, hi, e, live, n_faces) (n_faces 0: no table)."""
    faces = []
    for inst in instances:
        m = models.get(int(inst["model"]))
        faces.append((m["n_faces"] << (2 * m["e"])) if usable(inst, m, vs) and m["n_faces"] else 0)
    disabled = a_world + sum(faces) >= 2 ** 32
    if disabled:
        faces = [0] * len(faces)
    icum = np.concatenate([[0], np.cumsum(np.array(faces, dtype=np.uint64))]).astype(np.uint64)
    a_inst = int(sum(faces))
    header = {"a_inst": a_inst, "a_total": a_world + a_inst, "area_world": (np.float32(a_world + a_inst) * np.float32(vs)) * np.float32(vs),
              "n_lit": sum(1 for f in faces if f), "disabled": int(disabled)}
    return (icum & 0xFFFFFFFF).astype(np.uint32), header
