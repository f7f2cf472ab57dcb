"""The case table of the posed-model tests (tests/test_posed_instances_cpu.py, tests/test_posed_instances_gpu.py) — TESTS ONLY.

Five models: the four of instance_oracle.procedural_models at scale exponent 0 and the notched slab again at exponent 2.  Every case is a
set-up over one small world (a ground plate and a sparse cloud above it): a table of lattice instances, a table of poses, a camera."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

from blok_amd import pose as P
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, POSE
from blok_amd.affine import rotation_matrix
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests import pose_oracle as PO
from tests import scaled_instance_oracle as SO

SEED = 0xB10C0001
EXPONENTS = (0, 0, 0, 0, 2)
SLAB, BALL, CLOUD, ROD, BIG_SLAB = range(5)
WD, HT = 96, 64                                     # 3 x 2 bins
BIG = (116, 86)                                     # the larger frame ...
RECT = (8, 8, 100, 70)                              # ... and the rectangle of it: ragged tiles and bins


def models():
    m = IO.procedural_models()
    return m + [m[SLAB]]


def oracle_models(vs):
    return [SO.scaled_model(xyz, mats, e, vs) for (xyz, mats), e in zip(models(), EXPONENTS)]


def boxes():
    """[lo, hi) of every model in its own voxels."""
    return [(xyz.min(axis=0), xyz.max(axis=0) + 1) for xyz, _ in models()]


@functools.lru_cache(maxsize=None)
def world_voxels():
    """(xyz, material ids) of the world: a ground plate and a sparse cloud of voxels above it (distinct voxels)."""
    rng = np.random.default_rng(5)
    plate = np.array([(x, 0, z) for x in range(-40, 60) for z in range(-40, 60)], dtype=np.int32)
    pts = np.stack([rng.integers(-40, 60, 300), rng.integers(1, 50, 300), rng.integers(-40, 60, 300)], axis=1).astype(np.int32)
    xyz = np.unique(np.concatenate([plate, pts]), axis=0).astype(np.int32)
    return xyz, rng.integers(1, 60, size=len(xyz)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def world(vs):
    """world_voxels in a lattice of voxel size vs, packed (computed once per size, never changed)."""
    cm = W.ChunkManager(128, vs)
    cm.set_voxels(*world_voxels())
    cm.rebuild_dirty_chunks()
    return cm.pack_chunks_to_gpu_svo(W.scene_materials(SEED))


@dataclass
class Case:
    name: str
    instances: np.ndarray
    poses: np.ndarray
    eye: tuple
    target: tuple
    fov: float = 60.0
    min_pose_share: float = 0.05                    # of the 96 x 64 frame's pixels, from the oracle alone
    notes: dict = field(default_factory=dict)

    def camera(self, w, h):
        return W.camera_look_at(self.eye, self.target, self.fov, w, h)


def centre(model, vs):
    lo, hi = boxes()[model]
    return tuple(float(c) for c in (lo + hi) * 0.5 * vs * (1 << EXPONENTS[model]))


def turned(model, vs, pos, yaw=0.0, pitch=0.0, roll=0.0, scale=1.0):
    """The model turned about its box's centre, the centre at world voxel position `pos` (times vs)."""
    return P.rotation(model, math.radians(yaw), math.radians(pitch), math.radians(roll), scale, centre(model, vs), tuple(c * vs for c in pos))[0]


def through(model, vs, pos, linear):
    """The model under the forward linear map `linear` (3 x 3) about its box's centre, the centre at `pos` (times vs)."""
    c = np.array(centre(model, vs))
    f = np.zeros((3, 4))
    f[:, :3] = linear
    f[:, 3] = np.array(pos, dtype=np.float64) * vs - f[:, :3] @ c
    return P.from_matrix(f, model, c)[0]


def view(vs, pos, dist, up=8.0, shift=(0.0, 0.0, 0.0)):
    target = tuple((p + s) * vs for p, s in zip(pos, shift))
    return (target[0], target[1] + up * vs, target[2] - dist * vs), target


def table(vs):
    """The cases at voxel size vs, in the order of the issue's table."""
    none_i, none_p = np.zeros(0, dtype=INSTANCE), np.zeros(0, dtype=POSE)
    pos = (10.0, 20.0, 10.0)
    out = []
    mk = lambda name, inst, poses, eye_target, **kw: out.append(Case(name, np.array(inst, dtype=INSTANCE).reshape(-1), np.array(poses, dtype=POSE).reshape(-1), *eye_target, **kw))
    yaw30 = turned(SLAB, vs, pos, yaw=30.0)
    mk("1 yaw 30", none_i, [yaw30], view(vs, pos, 22.0))
    mk("2 compound at scale 1.5", none_i, [turned(BALL, vs, pos, 40.0, 25.0, -15.0, 1.5)], view(vs, pos, 40.0))
    mk("3 scale 0.5", none_i, [turned(CLOUD, vs, pos, 20.0, 10.0, 0.0, 0.5)], view(vs, pos, 18.0))
    mk("4 scale 4 rod", none_i, [turned(ROD, vs, pos, 25.0, 0.0, 10.0, 4.0)], view(vs, pos, 35.0))
    ry = rotation_matrix(math.radians(20.0))[:, :3]
    mk("5 mirror", none_i, [through(SLAB, vs, pos, ry @ np.diag([-1.0, 1.0, 1.0]))], view(vs, pos, 22.0))
    mk("6 shear", none_i, [through(SLAB, vs, pos, np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.3, 0.0, 1.0]]))], view(vs, pos, 24.0))
    c30, s30 = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    flat = PO.pose(SLAB, [[c30, 0.0, -s30], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], tuple(c * vs for c in pos), centre(SLAB, vs))
    mk("7 rank 2", none_i, [flat], view(vs, pos, 22.0))
    high = (10.0, 40.0, 10.0)
    mk("8 exponent 2", none_i, [turned(BIG_SLAB, vs, high, yaw=30.0)], view(vs, high, 90.0))
    inside = (10.0, 30.0, 10.0)
    eye = tuple((p + d) * vs for p, d in zip(inside, (0.7, 0.3, 0.2)))
    mk("9 camera inside", none_i, [turned(CLOUD, vs, inside, 15.0, 5.0, 0.0, 2.0)], (eye, tuple((p + d) * vs for p, d in zip(inside, (3.0, 1.0, 9.0)))))
    below = (10.0, -12.0, 10.0)
    mk("10 behind the world", none_i, [turned(SLAB, vs, below, yaw=30.0)], ((10.0 * vs, 20.0 * vs, -12.0 * vs), (10.0 * vs, 0.0, 10.0 * vs)),
       min_pose_share=0.0)
    mk("11 the same pose twice", none_i, [yaw30, yaw30], view(vs, pos, 22.0))
    a = IO.instance(BALL, (-5, 12, 20), (2, 0, 1), 5)
    b = IO.instance(ROD, (18, 9, 4), (1, 0, 2), 2)
    mk("12 mixed", [a, b], [P.from_instance(a, vs)[0], turned(SLAB, vs, (25.0, 15.0, 12.0), yaw=30.0)],
       ((10.0 * vs, 22.0 * vs, -25.0 * vs), (10.0 * vs, 12.0 * vs, 15.0 * vs)), min_pose_share=0.0)
    # 70 small rods in a patch that the 96 x 64 frame shows around pixel (48, 16), the middle of bin (1, 0): the camera looks 11.5 voxels below it
    patch = [turned(ROD, vs, (pos[0] - 1.6 + 0.4 * (i % 10), pos[1] - 1.1 + 0.4 * (i // 10), pos[2] + 0.05 * i), yaw=5.0 * i, scale=0.8) for i in range(70)]
    mk("13 overflow", none_i, patch, view(vs, (pos[0], pos[1] - 11.5, pos[2]), 60.0, up=0.0), min_pose_share=0.0, notes={"overflow": True})
    mk("14 no poses", [a, b], none_p, ((10.0 * vs, 22.0 * vs, -25.0 * vs), (10.0 * vs, 12.0 * vs, 15.0 * vs)), min_pose_share=0.0)
    return out


def corner_case(vs):
    """The yaw-30 slab with its silhouette's upper right corner at pixel (64, 32) of the 96 x 64 frame, a corner of four bins (a pixel is
    0.265 voxels wide at distance 22: 16 pixels right of the centre are 4.2 voxels)."""
    pos = (10.0, 20.0, 10.0)
    eye, target = view(vs, pos, 22.0, up=0.0, shift=(2.7, 4.5, 0.0))
    return Case("corner", np.zeros(0, dtype=INSTANCE), np.array([turned(SLAB, vs, pos, yaw=30.0)], dtype=POSE), eye, target)


def world_point(p, local_pt):
    """A world point that the pose sends to (or, under a singular m, nearest to) the local point, in float64."""
    m = np.asarray(p["m"], dtype=np.float64)
    return np.asarray(p["pivot"], dtype=np.float64) + np.linalg.pinv(m) @ (np.asarray(local_pt, dtype=np.float64) - np.asarray(p["local"], dtype=np.float64))


def aimed_rays(case, vs, per_entry, n_miss, seed, reach=120.0, length=1.0):
    """Rays from seeded origins towards a seeded point of each pose's and each instance's model, and n_miss rays that point away from all
    of them.  length: the length of every direction (the walk does not care)."""
    rng = np.random.default_rng(seed)
    bx = boxes()
    org, tgt = [], []
    for p in case.poses:
        m = int(p["model"])
        vm = vs * (1 << EXPONENTS[m])
        for _ in range(per_entry):
            tgt.append(world_point(p, rng.uniform(bx[m][0], bx[m][1]) * vm))
            org.append(tgt[-1] + rng.uniform(-reach, reach, size=3) * vs)
    for inst in case.instances:
        m = int(inst["model"])
        lo, hi = SO.world_span(inst, bx[m][0], bx[m][1], EXPONENTS[m])
        for _ in range(per_entry):
            tgt.append(rng.uniform(lo, hi) * vs)
            org.append(tgt[-1] + rng.uniform(-reach, reach, size=3) * vs)
    for _ in range(n_miss):
        org.append(rng.uniform(4 * reach, 5 * reach, size=3) * vs)
        tgt.append(org[-1] + rng.uniform(0.1, 1.0, size=3))
    org, tgt = np.array(org), np.array(tgt)
    d = tgt - org
    d *= length / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(len(org), dtype=O.RAY)
    rays["org"] = org.astype(np.float32)
    rays["dir"] = d.astype(np.float32)
    rays["tmin"] = 0.001
    rays["tmax"] = 10000.0 / length
    return rays


@functools.lru_cache(maxsize=None)
def world_lattice(vs):
    pw = world(vs)
    return O.Lattice(pw.nodes, pw.sub_chunks)


def expected(case, vs, rays, omodels, per_pose=None):
    """(records, ids) of the rays over the world, the case's instances and its poses, from the oracle alone."""
    base, _ = world_lattice(vs).trace(rays, threads=8)
    best, ids = SO.compose(base, rays, case.instances, omodels, EXPONENTS, vs)
    return PO.compose(best, ids, rays, case.poses, omodels, per_pose)
