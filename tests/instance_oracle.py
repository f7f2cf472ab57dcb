"""The expected records of world + instances (include/blok_hip.h, instanced voxel models), from the existing oracle alone — TESTS ONLY.

Per instance: the model alone in an oracle ChunkManager (tests/oracle_ffi.OracleWorld), the rays moved into its local space in numpy
float32 exactly as specified, the oracle's trace, the records mapped back, then composed with the world's records by the tie rule
(a candidate replaces the record only with a strictly smaller t; world first, then instance 0, 1, ...)."""
from __future__ import annotations

import itertools

import numpy as np

from blok_amd._ffi import INSTANCE, INSTANCE_NONE
from tests import oracle_ffi as O

SIGNED_PERMUTATIONS = [(p, f) for p in itertools.permutations(range(3)) for f in range(8)]     # all 48


def instance(model, offset, axis=(0, 1, 2), flip=0):
    rec = np.zeros(1, dtype=INSTANCE)
    rec["model"] = model
    rec["offset"] = offset
    rec["axis"] = axis
    rec["flip"] = flip
    return rec[0]


class OracleModel:
    """A model's voxels in the oracle's own ChunkManager, and its local box."""

    def __init__(self, xyz, mats, voxel_size=1.0):
        self.xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        self.mats = np.ascontiguousarray(mats, dtype=np.uint32)
        world = O.OracleWorld(128, voxel_size)
        world.set_voxels(self.xyz, self.mats)
        world.rebuild()
        self.nodes, self.subs = world.pack()
        self.lattice = O.Lattice(self.nodes, self.subs)
        self.lo = self.xyz.min(axis=0)
        self.hi = self.xyz.max(axis=0) + 1

    def trace(self, rays):
        return self.lattice.trace(rays, threads=8)[0]


def local_rays(rays, inst, voxel_size=1.0):
    """o'_k = s_k * fl(o[axis[k]] - offset[axis[k]] * vs), d'_k = s_k * d[axis[k]], tmin / tmax unchanged."""
    out = rays.copy()
    axis = [int(a) for a in inst["axis"]]
    for k in range(3):
        a = axis[k]
        s = np.float32(-1.0) if (int(inst["flip"]) >> k) & 1 else np.float32(1.0)
        rel = rays["org"][:, a].astype(np.float32) - np.float32(int(inst["offset"][a]) * voxel_size)
        out["org"][:, k] = s * rel
        out["dir"][:, k] = s * rays["dir"][:, a]
    return out


def world_records(local, inst):
    """Local records back to world space: t and material unchanged, voxel and face through the instance's orientation."""
    out = local.copy()
    hit = local["hit"] == 1
    axis = [int(a) for a in inst["axis"]]
    flip = int(inst["flip"])
    v = local["voxel"].astype(np.int64)
    for k in range(3):
        a = axis[k]
        o = int(inst["offset"][a])
        out["voxel"][:, a] = np.where(hit, (o - 1 - v[:, k]) if (flip >> k) & 1 else (o + v[:, k]), 0).astype(np.int16)
    face = local["face"].astype(np.int64)
    k = face // 2
    n = face % 2
    ax = np.array(axis)[np.minimum(k, 2)]
    fl = (flip >> np.minimum(k, 2)) & 1
    out["face"] = np.where(hit, 2 * ax + (n ^ fl), local["face"]).astype(np.uint8)
    return out


def compose(world, rays, instances, models, voxel_size=1.0):
    """(records, instance ids) of world + instances, bit for bit as specified."""
    best = world.copy()
    ids = np.full(len(rays), INSTANCE_NONE, dtype=np.uint32)
    for i, inst in enumerate(instances):
        m = models[int(inst["model"])]
        cand = world_records(m.trace(local_rays(rays, inst, voxel_size)), inst)
        take = (cand["hit"] == 1) & ((best["hit"] == 0) | (cand["t"] < best["t"]))
        best[take] = cand[take]
        ids[take] = i
    return best, ids


def shade(hits, materials):
    """RGBA8 of first-hit records as the trace kernels shade them (trace_core.h: shade_rgba)."""
    mats = np.ascontiguousarray(materials)
    face_k = np.array([0.8, 0.8, 1.0, 0.4, 0.6, 0.6], dtype=np.float32)
    mid = np.minimum(hits["material_id"], 65535)
    inside = mid < len(mats)
    alb = np.where(inside[:, None], mats["albedo"][np.minimum(mid, len(mats) - 1)], np.array([1.0, 0.0, 1.0], dtype=np.float32))
    q = (np.minimum(alb * face_k[np.minimum(hits["face"], 5)][:, None], np.float32(1.0)) * np.float32(255.0) + np.float32(0.5)).astype(np.uint32)
    return np.where(hits["hit"] == 1, 0xFF000000 | (q[:, 2] << 16) | (q[:, 1] << 8) | q[:, 0],
                    0xFF000000 | (230 << 16) | (200 << 8) | 160).astype(np.uint32)


def procedural_models(seed=7):
    """Voxel lists of a few asymmetric shapes (so that every orientation is visible): a notched slab, a ball, a sparse cloud, a rod."""
    rng = np.random.default_rng(seed)
    out = []
    g = np.stack(np.meshgrid(np.arange(12), np.arange(9), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
    keep = ~((g[:, 0] > 7) & (g[:, 1] > 4)) & ~((g[:, 2] < 2) & (g[:, 0] < 3))
    xyz = g[keep]
    out.append((xyz, (1 + (xyz[:, 0] * 7 + xyz[:, 1] * 3 + xyz[:, 2]) % 40).astype(np.uint32)))
    g = np.stack(np.meshgrid(*[np.arange(-6, 7)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r2 = (g ** 2).sum(1)
    xyz = g[(r2 <= 36) & ~((g[:, 0] > 2) & (g[:, 1] > 2))]
    out.append((xyz, (1 + np.abs(xyz[:, 1]) * 5 % 50).astype(np.uint32)))
    xyz = np.unique(rng.integers(0, 20, size=(300, 3)), axis=0)
    out.append((xyz, rng.integers(1, 60, size=len(xyz)).astype(np.uint32)))
    xyz = np.array([(x, 0, 0) for x in range(10)] + [(0, 1, 0), (0, 0, 1)], dtype=np.int32)
    out.append((xyz, np.arange(1, len(xyz) + 1, dtype=np.uint32)))
    return [(np.ascontiguousarray(x, dtype=np.int32), m) for x, m in out]


def random_instances(n, n_models, lo, hi, seed):
    """n instances with seeded models, offsets in [lo, hi) and orientations."""
    rng = np.random.default_rng(seed)
    table = np.zeros(n, dtype=INSTANCE)
    for i in range(n):
        p, f = SIGNED_PERMUTATIONS[rng.integers(48)]
        table[i] = instance(int(rng.integers(n_models)), rng.integers(lo, hi, size=3), p, f)
    return table
