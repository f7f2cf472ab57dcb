"""CPU: posed models in the path-traced frame (include/blok_hip.h, "Path-traced frames with poses") — what the posed path kernel adds to the
instanced one (blok_amd/csrc/hip/posed_paths_core.h, path_core.h), compiled for the host through tests/host_harness/posed_paths_shim.cpp and, for the pose BVH (pose_tlas_core.h), tests/host_harness/pose_tlas_shim.cpp on top of it:
the path loop's pose queries against the oracle composition of tests/pose_oracle.py, the normal of a posed hit against a numpy float32
restatement of the rule, the sampling frame of any unit normal against the face frame, bit for bit."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import pose as P
from blok_amd._ffi import INSTANCE, POSE
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests import pose_cases as PC
from tests import pose_oracle as PO
from tests.conftest import records_equal
from tests.test_posed_instances_cpu import FLAGS, ROOT, SRC, VOXEL_SIZES, Shim, _p, case_file

f32 = np.float32


def build_shim(out) -> C.CDLL:
    subprocess.run(["g++", *FLAGS, "-shared", "-o", os.fspath(out), os.fspath(SRC / "pose_tlas_shim.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    L.pt_node_count.argtypes = [C.c_uint32]
    L.pt_node_count.restype = C.c_uint32
    L.pt_max.restype = C.c_uint32
    L.pt_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    L.pt_boxes.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_int,
                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.is_model.restype = C.c_void_p
    L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_free.argtypes = [C.c_void_p]
    L.ss_set_scale.argtypes = [C.c_void_p, C.c_uint32]
    L.ps_shade_face.argtypes = [C.c_void_p, C.c_uint32]
    L.ps_shade_face.restype = C.c_uint32
    L.pp_normals.argtypes = [C.c_void_p, C.c_void_p]
    L.pp_tangent_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.pp_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_size_t,
                             C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return Shim(build_shim(tmp_path_factory.mktemp("posed_paths") / "libposed_paths_shim.so"))


@pytest.fixture(scope="module")
def omodels():
    return {vs: PC.oracle_models(vs) for vs in VOXEL_SIZES}


AXIS_NORMALS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=f32) + f32(0.0)      # every zero +0


def normal_rule(p, face):
    """The rule of blok_hip.h in numpy float32 (every operation rounds once): v = s * row k; q = (v0 v0 + v1 v1) + v2 v2; !(q > 0): the axis
    normal of the shade face; else v / sqrt(q) + 0."""
    k, n = face >> 1, face & 1
    v = (f32(-1.0) if n else f32(1.0)) * np.asarray(p["m"], dtype=f32)[k]
    with np.errstate(all="ignore"):
        q = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        assert q.dtype == f32
        if not q > 0:
            return AXIS_NORMALS[PO.shade_face(p, face)]
        return v / np.sqrt(q) + f32(0.0)


def shim_normals(shim, p):
    rec = np.array([p], dtype=POSE)
    out = np.zeros((6, 3), dtype=f32)
    shim.lib.pp_normals(_p(rec), _p(out))
    return out


def path_compose(shim, case, vs, rays):
    got = np.zeros(len(rays), dtype=O.HIT)
    ids = np.zeros(len(rays), dtype=np.uint32)
    any_hit = np.zeros(len(rays), dtype=np.uint8)
    shim.lib.pp_compose(shim.world(vs), shim.array, len(shim.handles), _p(case.instances), len(case.instances), _p(case.poses), len(case.poses),
                        vs, _p(rays), len(rays), _p(got), _p(ids), _p(any_hit))
    return got, ids, any_hit


def surface_rays(case, vs, want, rays, seed):
    """Bounce-like and shadow-like rays: origins ON the surfaces the aimed rays found (hit point + 0.002 along a seeded direction, as the path
    loop leaves a surface), seeded directions and the sun's."""
    rng = np.random.default_rng(seed)
    hit = np.flatnonzero(want["hit"] == 1)
    org = rays["org"][hit] + rays["dir"][hit] * want["t"][hit, None]
    d = rng.normal(size=org.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sun = np.array([0.5, 0.8, 0.3]) / np.linalg.norm([0.5, 0.8, 0.3])
    d[::2] = sun
    out = np.zeros(len(hit), dtype=O.RAY)
    out["org"] = (org + 0.002 * d).astype(f32)
    out["dir"] = d.astype(f32)
    out["tmin"] = 0.001
    out["tmax"] = 1000.0
    return out


# ---- 1. the path loop's pose queries equal the oracle composition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_closest_and_any_hit_equal_the_oracle(shim, omodels, vs):
    """Closest: record and winner equal the oracle's composition (world, instances, poses in order, strictly smaller t).  Any-hit: 1 exactly
    where that composition reports a voxel on the same interval.  Aimed rays, then rays that start on the surfaces they found."""
    for n, case in enumerate(PC.table(vs)):
        aimed = PC.aimed_rays(case, vs, per_entry=max(10, 600 // max(1, len(case.poses) + len(case.instances))), n_miss=40, seed=300 + n)
        want, want_ids = PC.expected(case, vs, aimed, omodels[vs])
        for rays, w, wi in ((aimed, want, want_ids), (None, None, None)):
            if rays is None:
                rays = surface_rays(case, vs, want, aimed, 400 + n)
                w, wi = PC.expected(case, vs, rays, omodels[vs])
            got, ids, any_hit = path_compose(shim, case, vs, rays)
            bad = np.flatnonzero(~records_equal(got, w) | (ids != wi))
            assert bad.size == 0, f"{case.name} at vs {vs}: {bad.size} of {len(rays)} differ, first {bad[:3]}"
            assert (any_hit == w["hit"]).all(), case.name


def test_unusable_poses_and_destroyed_models_are_skipped(shim, omodels):
    vs = 1.0
    case = PC.table(vs)[0]
    bad_floats = case.poses[0].copy(); bad_floats["m"][1][1] = np.inf
    no_model = case.poses[0].copy(); no_model["model"] = 99
    table = np.array([bad_floats, no_model, case.poses[0], bad_floats], dtype=POSE)
    rays = PC.aimed_rays(case, vs, 400, 40, 7)
    want, want_ids = PC.expected(case, vs, rays, omodels[vs])
    mixed = PC.Case("skipped", case.instances, table, case.eye, case.target)
    got, ids, any_hit = path_compose(shim, mixed, vs, rays)
    assert records_equal(got, want).all() and (any_hit == want["hit"]).all()
    won = (want_ids != 0xFFFFFFFF)
    assert won.sum() > 100 and (ids[won] == (_ffi.POSE_ID | 2)).all() and (ids[~won] == 0xFFFFFFFF).all()


# ---- 2. the normal of a posed hit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_normal_rule_equals_its_float32_restatement(shim, vs):
    seen_general = 0
    for case in PC.table(vs):
        for p in case.poses:
            got = shim_normals(shim, p)
            for face in range(6):
                want = normal_rule(p, face)
                assert got[face].tobytes() == np.asarray(want, dtype=f32).tobytes(), (case.name, face, got[face], want)
                seen_general += int(np.count_nonzero(got[face]) > 1)
    assert seen_general > 30


def test_normals_of_poses_from_instances_are_the_axis_normals(shim):
    """The 48 orientations through blok_pose_from_instance, models of scale exponents 0 and 2 (the exponent is the model's: it does not
    enter the pose), at three voxel sizes: the instance's world face (instance_core.h: face 2k + n -> 2 axis[k] + (n ^ flip_k)), zeros +0."""
    for vs in (1.0, 0.5, 2.0):
        for i, (perm, flip) in enumerate(IO.SIGNED_PERMUTATIONS):
            inst = np.array([IO.instance((PC.SLAB, PC.BIG_SLAB, PC.ROD)[i % 3], (3 - i, 7, i), perm, flip)], dtype=INSTANCE)
            p = P.from_instance(inst, vs)[0]
            got = shim_normals(shim, p)
            for face in range(6):
                k, n = face >> 1, face & 1
                world_face = 2 * int(inst[0]["axis"][k]) + (n ^ ((int(inst[0]["flip"]) >> k) & 1))
                assert got[face].tobytes() == AXIS_NORMALS[world_face].tobytes(), (perm, flip, face)


def test_a_zero_row_falls_back_to_the_shade_face(shim):
    flat = PC.table(1.0)[6].poses[0]                       # the rank-2 pose: row 2 is zero
    assert not np.asarray(flat["m"])[2].any()
    got = shim_normals(shim, flat)
    for face in (4, 5):
        rec = np.array([flat], dtype=POSE)
        assert got[face].tobytes() == AXIS_NORMALS[shim.lib.ps_shade_face(_p(rec), face)].tobytes()
    tiny = flat.copy(); tiny["m"][2] = (1.0e-30, 0.0, -1.0e-30)          # q underflows to 0
    got = shim_normals(shim, tiny)
    assert got[4].tobytes() == AXIS_NORMALS[0].tobytes() and got[5].tobytes() == AXIS_NORMALS[1].tobytes()


# ---- 3. the sampling frame -------------------------------------------------------------------------------------------------------------------
def test_general_tangent_frame_equals_the_face_frame_on_axis_normals(shim):
    for n in AXIS_NORMALS:
        a, b = np.zeros(6, dtype=f32), np.zeros(6, dtype=f32)
        n = np.ascontiguousarray(n)
        shim.lib.pp_tangent_frame(_p(n), 1, _p(a))
        shim.lib.pp_tangent_frame(_p(n), 0, _p(b))
        assert a.tobytes() == b.tobytes(), (n, a, b)
    # and a unit, orthogonal frame for a turned normal
    n = np.array([0.48, 0.6, 0.64], dtype=f32)
    a = np.zeros(6, dtype=f32)
    shim.lib.pp_tangent_frame(_p(n), 1, _p(a))
    t, b = a[:3].astype(np.float64), a[3:].astype(np.float64)
    assert abs(np.linalg.norm(t) - 1) < 1e-6 and abs(t @ n) < 1e-6 and abs(b @ n) < 1e-6 and abs(b @ t) < 1e-6


# ---- 3b. the pose BVH: an optimisation of the loop ------------------------------------------------------------------------------------------------
from fractions import Fraction  # noqa: E402

KIND_SKIPPED, KIND_BOXED, KIND_UNBOUNDED = 0, 1, 2


def tree_compose(shim, case, vs, rays, tree, models=None, cam=None):
    got = np.zeros(len(rays), dtype=O.HIT)
    ids = np.zeros(len(rays), dtype=np.uint32)
    any_hit = np.zeros(len(rays), dtype=np.uint8)
    eye = np.asarray(case.eye if cam is None else cam, dtype=f32)
    array, count = (shim.array, len(shim.handles)) if models is None else models
    shim.lib.pt_compose(shim.world(vs), array, count, _p(case.instances), len(case.instances), _p(case.poses), len(case.poses), vs, _p(eye), int(tree),
                        _p(rays), len(rays), _p(got), _p(ids), _p(any_hit))
    return got, ids, any_hit


def build_tree(shim, poses, vs, eye, models=None):
    array, count = (shim.array, len(shim.handles)) if models is None else models
    nodes = np.zeros((shim.lib.pt_node_count(len(poses)), 8), dtype=np.int32)
    eye = np.asarray(eye, dtype=f32)
    shim.lib.pt_build(array, count, _p(poses), len(poses), vs, _p(eye), _p(nodes))
    return nodes


def leaf_boxes(shim, poses, vs, eye):
    origin = np.zeros(6)
    kind = np.zeros(len(poses), dtype=np.uint32)
    box = np.zeros((len(poses), 6))
    eye = np.asarray(eye, dtype=f32)
    shim.lib.pt_boxes(shim.array, len(shim.handles), _p(poses), len(poses), vs, _p(eye), _p(origin), _p(kind), _p(box))
    return origin, kind, box


def assert_tree_equals_loop(shim, case, vs, rays, what, models=None):
    a = tree_compose(shim, case, vs, rays, 1, models)
    b = tree_compose(shim, case, vs, rays, 0, models)
    bad = np.flatnonzero(~records_equal(a[0], b[0]) | (a[1] != b[1]) | (a[2] != b[2]))
    assert bad.size == 0, f"{what}: tree and loop differ on {bad.size} of {len(rays)} rays, first {bad[:3]}"
    return b


@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_tree_equals_loop_on_every_case(shim, omodels, vs):
    """Closest: record and winner; any-hit: the answer.  Aimed rays, and rays that start ON model surfaces and inside preimage boxes."""
    for n, case in enumerate(PC.table(vs)):
        aimed = PC.aimed_rays(case, vs, per_entry=max(10, 600 // max(1, len(case.poses) + len(case.instances))), n_miss=40, seed=500 + n)
        want, _ = PC.expected(case, vs, aimed, omodels[vs])
        loop = assert_tree_equals_loop(shim, case, vs, aimed, case.name)
        assert records_equal(loop[0], want).all()
        assert_tree_equals_loop(shim, case, vs, surface_rays(case, vs, want, aimed, 600 + n), case.name + ", surface rays")
        if len(case.poses):                                  # origins inside the preimage boxes
            rng = np.random.default_rng(700 + n)
            inside = np.zeros(200, dtype=O.RAY)
            bx = PC.boxes()
            for i in range(len(inside)):
                p = case.poses[i % len(case.poses)]
                m = int(p["model"])
                inside["org"][i] = PC.world_point(p, rng.uniform(bx[m][0], bx[m][1]) * vs * (1 << PC.EXPONENTS[m]))
            d = rng.normal(size=(len(inside), 3))
            inside["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
            inside["tmin"], inside["tmax"] = 0.001, 1000.0
            assert_tree_equals_loop(shim, case, vs, inside, case.name + ", rays from inside")


@pytest.mark.parametrize("count", [1, 3, 70, 4097])
def test_tree_equals_loop_with_many_poses(shim, count):
    """Seeded small rods, with the same pose twice, unusable poses and a destroyed model between them; 4097 poses take the loop either way."""
    vs = 1.0
    rng = np.random.default_rng(count)
    poses = np.concatenate([PC.turned(PC.ROD if i % 5 else PC.BALL, vs, tuple(rng.uniform((-30, 5, -30), (50, 45, 50))), *rng.uniform(-180, 180, size=3),
                                      scale=float(rng.uniform(0.5, 2.0))).reshape(1) for i in range(count)])
    clean = poses.copy()
    if count >= 3:
        poses[1] = poses[0]                                  # the same pose twice: the lower index keeps the tie
    if count >= 70:
        poses[5]["m"][0][0] = np.nan
        poses[6]["model"] = 99
        poses[7]["model"] = PC.BALL                          # destroyed below
        poses[7 + 5]["model"] = PC.ROD
    handles = list(shim.handles)
    destroyed = (C.c_void_p * len(handles))(*[None if (count >= 70 and i == PC.BALL) else h.value for i, h in enumerate(handles)])
    case = PC.Case("many", np.zeros(0, dtype=INSTANCE), poses, (10.0, 60.0, -70.0), (10.0, 15.0, 10.0))
    sample = PC.Case("sample", case.instances, clean[:: max(1, count // 64)][:64], case.eye, case.target)
    rays = PC.aimed_rays(sample, vs, per_entry=20, n_miss=50, seed=count)
    loop = assert_tree_equals_loop(shim, case, vs, rays, f"{count} poses", (destroyed, len(handles)))
    won = loop[1][loop[1] != 0xFFFFFFFF] & 0x7FFFFFFF
    assert len(won) > 10 and (count < 3 or 1 not in won)
    if count >= 70:
        assert not {5, 6}.intersection(won.tolist()) and 7 not in won
    if count <= shim.lib.pt_max():
        nodes = build_tree(shim, poses, vs, case.eye, (destroyed, len(handles)))
        assert nodes[0][6] == 1 << max(0, count - 1).bit_length() and nodes[0][0] == 0


def exact_in_leaf(exact, lo, hi, vs):
    return all(Fraction(int(lo[j])) * Fraction(vs) <= exact[0][j] and exact[1][j] <= Fraction(int(hi[j])) * Fraction(vs) for j in range(3))


def test_leaf_boxes_hold_the_exact_preimage_and_are_no_blanket(shim):
    bx = PC.boxes()
    checked = 0
    for vs in VOXEL_SIZES:
        for case in PC.table(vs):
            if not len(case.poses):
                continue
            origin, kind, box = leaf_boxes(shim, case.poses, vs, case.eye)
            nodes = build_tree(shim, case.poses, vs, case.eye)
            slots = int(nodes[0][6])
            leaves = {int(nd[6]) & 0x7FFFFFFF: nd for nd in nodes[slots:] if nd[6] != -1}
            for i, p in enumerate(case.poses):
                m = int(p["model"])
                cell = 1 << PC.EXPONENTS[m]
                exact = PO.preimage_box(p, bx[m][0] * cell, bx[m][1] * cell, vs)
                if exact is None:
                    assert kind[i] == KIND_UNBOUNDED and i not in leaves
                    continue
                assert kind[i] == KIND_BOXED and all(Fraction(box[i][j]) <= exact[0][j] and exact[1][j] <= Fraction(box[i][3 + j]) for j in range(3))
                assert exact_in_leaf(exact, leaves[i][0:3], leaves[i][3:6], vs), (case.name, leaves[i], exact)
                # the origin box holds the camera, the lattice and the preimage
                assert all(origin[j] <= min(case.eye[j], -32768 * vs, float(exact[0][j])) and origin[3 + j] >= max(case.eye[j], 32768 * vs, float(exact[1][j])) for j in range(3))
                checked += 1
    assert checked >= 20
    rng = np.random.default_rng(78)
    covered = 0
    for i in range(200):
        m = int(rng.integers(5))
        mat = np.clip(rng.uniform(-1, 1, size=(3, 3)) * 10.0 ** rng.uniform(-2, 3), -1024, 1024)
        p = PO.pose(m, mat, rng.uniform(-2.0 ** 20, 2.0 ** 20, size=3) * 10.0 ** rng.uniform(-4, 0), rng.uniform(-2.0 ** 20, 2.0 ** 20, size=3) * 10.0 ** rng.uniform(-5, 0))
        vs = VOXEL_SIZES[i % 2]
        rec = np.array([p], dtype=POSE)
        eye = rng.uniform(-500, 500, size=3)
        _, kind, box = leaf_boxes(shim, rec, vs, eye)
        cell = 1 << PC.EXPONENTS[m]
        exact = PO.preimage_box(p, bx[m][0] * cell, bx[m][1] * cell, vs)
        if kind[0] == KIND_BOXED:
            assert exact is not None and all(Fraction(box[0][j]) <= exact[0][j] and exact[1][j] <= Fraction(box[0][3 + j]) for j in range(3)), (i, p)
            nodes = build_tree(shim, rec, vs, eye)
            assert exact_in_leaf(exact, nodes[1][0:3], nodes[1][3:6], vs) or np.abs(nodes[1][0:6]).max() >= 2 ** 31 - 2      # (a box clamped at the ends of int32)
            covered += 1
        else:
            assert kind[0] == KIND_UNBOUNDED
    assert covered > 150
    # No blanket: a rotation at scale 1 near the origin, vs 1.  From the margin formula at these inputs: the ray origins reach |o - pivot| <=
    # 32768 + 1 + 32769 / 4096 + |pivot| < 32800, the preimage B < 2 * 20, so q < 2 * 32800 + 40 = 65640 per axis; a rotation's row has
    # |m_k0| + |m_k1| + |m_k2| <= sqrt(3), so delta_k <= 16 * 2^-24 * (sqrt(3) * 65640 + |local| + |box|) < 16 * 2^-24 * 113800 < 0.109; mapped
    # back by the inverse rotation (rows again <= sqrt(3) in sum) the box grows by < 0.189 per side, plus 2^-20 (|pivot| + R) < 0.0001; rounding
    # outwards to whole voxels adds < 1, the pad adds 1: at most 2 voxels a side beyond the exact preimage's own outward rounding, 2.19 beyond the preimage.
    for yaw, pitch, roll in ((30.0, 0.0, 0.0), (40.0, 25.0, -15.0), (10.0, 80.0, 45.0)):
        p = PC.turned(PC.SLAB, 1.0, (10.0, 20.0, 10.0), yaw, pitch, roll)
        exact = PO.preimage_box(p, bx[PC.SLAB][0], bx[PC.SLAB][1], 1.0)
        nd = build_tree(shim, np.array([p], dtype=POSE), 1.0, (10.0, 28.0, -12.0))[1]
        for j in range(3):
            assert 0 <= float(exact[0][j]) - nd[j] <= 2.19 and 0 <= nd[3 + j] - float(exact[1][j]) <= 2.19, (yaw, nd, exact)
            assert math.floor(exact[0][j]) - nd[j] <= 2 and nd[3 + j] - math.ceil(exact[1][j]) <= 2


def test_a_rank_2_pose_sets_the_linear_flag_and_queries_equal_the_loop(shim, omodels):
    vs = 1.0
    table = PC.table(vs)
    flat, yaw30 = table[6].poses[0], table[0].poses[0]
    poses = np.array([yaw30, flat, table[1].poses[0]], dtype=POSE)
    case = PC.Case("rank 2 among others", np.zeros(0, dtype=INSTANCE), poses, table[0].eye, table[0].target)
    nodes = build_tree(shim, poses, vs, case.eye)
    assert nodes[0][0] == 1 and nodes[0][7] == 2                    # the linear flag; two poses have a box
    assert build_tree(shim, poses[[0, 2]], vs, case.eye)[0][0] == 0
    rays = PC.aimed_rays(case, vs, 300, 40, 11)
    loop = assert_tree_equals_loop(shim, case, vs, rays, case.name)
    want, want_ids = PC.expected(case, vs, rays, omodels[vs])
    assert records_equal(loop[0], want).all() and (loop[1] == want_ids).all()
    assert ((loop[1] & 0x7FFFFFFF) == 1).sum() > 20                # the flat pose wins rays: it is in the loop


def test_tree_invariants(shim):
    """Heap order, escape links, empty nodes, the header — the instance tree's format."""
    vs = 1.0
    for case in (PC.table(vs)[12], PC.table(vs)[11], PC.table(vs)[0]):             # 70 rods; two poses; one
        n = len(case.poses)
        nodes = build_tree(shim, case.poses, vs, case.eye)
        slots = 1 << max(0, n - 1).bit_length()
        assert len(nodes) == 2 * slots and nodes[0][6] == slots and nodes[0][7] == n and nodes[0][0] == 0
        child, escape = nodes[:, 6].view(np.uint32), nodes[:, 7].view(np.uint32)
        seen = []
        for k in range(1, 2 * slots):
            e = k
            while e & 1:
                e >>= 1
            e += 1
            assert escape[k] == (0 if e == 1 else e)
            if k >= slots:
                if k - slots < n:
                    assert child[k] & 0x80000000 and child[k] != 0xFFFFFFFF
                    seen.append(int(child[k] & 0x7FFFFFFF))
                else:
                    assert child[k] == 0xFFFFFFFF and (nodes[k][0:3] == 0x7FFFFFFF).all() and (nodes[k][3:6] == -2 ** 31).all()
            else:
                l, r = nodes[2 * k], nodes[2 * k + 1]
                both_empty = child[2 * k] == 0xFFFFFFFF and child[2 * k + 1] == 0xFFFFFFFF
                assert child[k] == (0xFFFFFFFF if both_empty else 2 * k)
                assert (nodes[k][0:3] == np.minimum(l[0:3], r[0:3])).all() and (nodes[k][3:6] == np.maximum(l[3:6], r[3:6])).all()
        assert sorted(seen) == list(range(n))


def test_tree_shim_under_address_and_ub_sanitizers(tmp_path, omodels):
    """pose_tlas_shim.cpp as a stand-alone program (its own main): every case replayed through the tree and the loop.  Nothing loaded into
    Python is sanitized."""
    exe = tmp_path / "pose_tlas_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", "-DPOSE_TLAS_SHIM_MAIN", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-o",
                    os.fspath(exe), os.fspath(SRC / "pose_tlas_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    files = []
    for vs in VOXEL_SIZES:
        for n, case in enumerate(PC.table(vs)):
            rays = PC.aimed_rays(case, vs, per_entry=max(4, 300 // max(1, len(case.poses) + len(case.instances))), n_miss=20, seed=290 + n)
            want, want_ids = PC.expected(case, vs, rays, omodels[vs])
            files.append(tmp_path / f"case_{n}_{vs}.bin")
            case_file(files[-1], case, vs, rays, want, want_ids)
    run = subprocess.run([os.fspath(exe), *map(os.fspath, files)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "pose_tlas_shim: ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count(" rays\n") == len(files)


# ---- 4. the shim alone under the sanitizers ---------------------------------------------------------------------------------------------------
def test_shim_under_address_and_ub_sanitizers(tmp_path, omodels):
    """The shim as a stand-alone program (its own main) replays the case table's aimed rays against the oracle's records.  Nothing loaded into
    Python is sanitized."""
    exe = tmp_path / "posed_paths_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", "-DPOSED_PATHS_SHIM_MAIN", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-o",
                    os.fspath(exe), os.fspath(SRC / "posed_paths_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    files = []
    for vs in VOXEL_SIZES:
        for n, case in enumerate(PC.table(vs)):
            rays = PC.aimed_rays(case, vs, per_entry=max(4, 300 // max(1, len(case.poses) + len(case.instances))), n_miss=20, seed=190 + n)
            want, want_ids = PC.expected(case, vs, rays, omodels[vs])
            files.append(tmp_path / f"case_{n}_{vs}.bin")
            case_file(files[-1], case, vs, rays, want, want_ids)
    run = subprocess.run([os.fspath(exe), *map(os.fspath, files)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "posed_paths_shim: ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count(" rays\n") == len(files)


# ---- 5. ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_abi_and_symbols():
    lib = _ffi.hip_lib()
    assert lib.blok_hip_abi_version() >= (1 << 16) | 23
    for name in ("blok_hip_trace_paths_posed", "blok_hip_trace_paths_posed_device", "blok_hip_trace_paths_posed_ref_device", "blok_hip_draw_frame_rt_posed",
                 "blok_hip_debug_build_pose_tlas", "blok_hip_set_pose_tlas"):
        assert getattr(lib, name) is not None
    from blok_amd.tracer import HipTracer
    for name in ("trace_paths_posed", "trace_paths_posed_device", "trace_paths_posed_ref_device", "draw_frame_rt_posed", "debug_build_pose_tlas", "set_pose_tlas"):
        assert callable(getattr(HipTracer, name))
