"""The expected records of world + instances of scaled models (include/blok_hip.h, "Scaled models"), from the existing oracle alone —
TESTS ONLY.

A model with exponent e is the same voxel list in an oracle ChunkManager of voxel size vs * 2^e (tests/instance_oracle.OracleModel with
that voxel size).  The ray rule is instance_oracle.local_rays, unchanged: the offset is in world voxels.  The record comes back with t,
material and the face rule unchanged, and the voxel of the cell's lowest world voxel:
    w[axis[k]] = offset + v'_k * 2^e,   or   offset - (v'_k + 1) * 2^e   when flipped."""
from __future__ import annotations

import numpy as np

from blok_amd._ffi import INSTANCE_NONE
from tests import instance_oracle as IO


def scaled_model(xyz, mats, exponent, voxel_size=1.0):
    """The oracle's copy of a model walked at vm = vs * 2^e."""
    return IO.OracleModel(xyz, mats, voxel_size=voxel_size * float(1 << exponent))


def world_span(inst, lo, hi, exponent):
    """The instance's world box [lo, hi) in world voxels (int64) for a model box [lo, hi) in model voxels."""
    out_lo = np.zeros(3, dtype=np.int64)
    out_hi = np.zeros(3, dtype=np.int64)
    cell = 1 << exponent
    for k in range(3):
        a = int(inst["axis"][k])
        o = int(inst["offset"][a])
        if (int(inst["flip"]) >> k) & 1:
            out_lo[a], out_hi[a] = o - int(hi[k]) * cell, o - int(lo[k]) * cell
        else:
            out_lo[a], out_hi[a] = o + int(lo[k]) * cell, o + int(hi[k]) * cell
    return out_lo, out_hi


def world_records(local, inst, exponent):
    """Local records back to world space: instance_oracle.world_records' face rule, the scaled voxel rule."""
    out = IO.world_records(local, inst)            # t, material, face (and the scale-0 voxel, replaced below)
    hit = local["hit"] == 1
    flip = int(inst["flip"])
    v = local["voxel"].astype(np.int64)
    cell = 1 << exponent
    for k in range(3):
        a = int(inst["axis"][k])
        o = int(inst["offset"][a])
        w = (o - (v[:, k] + 1) * cell) if (flip >> k) & 1 else (o + v[:, k] * cell)
        out["voxel"][:, a] = np.where(hit, w, 0).astype(np.int16)
    return out


def compose(world, rays, instances, models, exponents, voxel_size=1.0):
    """(records, instance ids) of world + instances.  models[m]: scaled_model(..., exponents[m], voxel_size)."""
    best = world.copy()
    ids = np.full(len(rays), INSTANCE_NONE, dtype=np.uint32)
    for i, inst in enumerate(instances):
        m = int(inst["model"])
        cand = world_records(models[m].trace(IO.local_rays(rays, inst, voxel_size)), inst, exponents[m])
        take = (cand["hit"] == 1) & ((best["hit"] == 0) | (cand["t"] < best["t"]))
        best[take] = cand[take]
        ids[take] = i
    return best, ids
