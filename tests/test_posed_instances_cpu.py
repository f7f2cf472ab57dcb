"""CPU: posed models (include/blok_hip.h, "Posed models") — the kernels' pose math (blok_amd/csrc/hip/posed_core.h) compiled for the host
through tests/host_harness/posed_instance_shim.cpp, against the oracle helper tests/pose_oracle.py, bit for bit, over the case table of
tests/pose_cases.py; the bins' world box against exact preimages; the limits; the host helpers of blok_world.h."""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import affine as AF
from blok_amd import pose as P
from blok_amd._ffi import INSTANCE, INSTANCE_NONE, POSE, POSE_ID, BlokError
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests import pose_cases as PC
from tests import pose_oracle as PO
from tests import scaled_instance_oracle as SO
from tests.conftest import records_equal

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
FLAGS = ["-O1", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}"]
VOXEL_SIZES = [1.0, 0.5]


def build_shim(out: Path) -> C.CDLL:
    subprocess.run(["g++", *FLAGS, "-shared", "-o", os.fspath(out), os.fspath(SRC / "posed_instance_shim.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    L.is_model.restype = C.c_void_p
    L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_free.argtypes = [C.c_void_p]
    L.ss_set_scale.argtypes = [C.c_void_p, C.c_uint32]
    L.ss_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ps_usable.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
    L.ps_floats_rule.argtypes = [C.c_void_p]
    L.ps_box_usable.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ps_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ps_shade_face.argtypes = [C.c_void_p, C.c_uint32]
    L.ps_shade_face.restype = C.c_uint32
    L.ps_world_box.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ps_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_size_t,
                             C.c_void_p, C.c_void_p]
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data) if len(a) else None


class Shim:
    """The library, the five models of the case table at their exponents, and the small world per voxel size."""

    def __init__(self, lib):
        self.lib = lib
        self.handles = []
        for (xyz, mats), e in zip(PC.models(), PC.EXPONENTS):
            self.handles.append(self.model(xyz, mats, e))
        self.array = (C.c_void_p * len(self.handles))(*[h.value for h in self.handles])
        self.worlds = {}

    def model(self, xyz, mats, exponent=0):
        why = C.c_char_p()
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        mats = np.ascontiguousarray(mats, dtype=np.uint32)
        h = self.lib.is_model(_p(xyz), _p(mats), len(mats), C.byref(why))
        assert h, why.value
        h = C.c_void_p(h)
        assert self.lib.ss_set_scale(h, exponent) == 0
        return h

    def world(self, vs):
        if vs not in self.worlds:
            self.worlds[vs] = self.model(*PC.world_voxels())                  # the world's tree from its voxel list, walked at vs
        return self.worlds[vs]

    def compose(self, case, vs, rays):
        got = np.zeros(len(rays), dtype=O.HIT)
        ids = np.zeros(len(rays), dtype=np.uint32)
        self.lib.ps_compose(self.world(vs), self.array, len(self.handles), _p(case.instances), len(case.instances), _p(case.poses), len(case.poses),
                            vs, _p(rays), len(rays), _p(got), _p(ids))
        return got, ids

    def world_box(self, pose, handle, vs, cam):
        rec = np.array([pose], dtype=POSE)
        cam = np.ascontiguousarray(cam, dtype=np.float32)
        lo, hi = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        ok = self.lib.ps_world_box(_p(rec), handle, vs, _p(cam), _p(lo), _p(hi))
        return (lo, hi) if ok else None


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return Shim(build_shim(tmp_path_factory.mktemp("posed_instance_shim") / "libposed_instance_shim.so"))


@pytest.fixture(scope="module")
def omodels():
    return {vs: PC.oracle_models(vs) for vs in VOXEL_SIZES}


def assert_same(got, ids, want, want_ids, rays, what):
    bad = np.flatnonzero(~records_equal(got, want) | (ids != want_ids))
    assert bad.size == 0, f"{what}: {bad.size} of {len(rays)} differ; first: {rays[bad[:2]]} got {got[bad[:2]]} {ids[bad[:2]]} want {want[bad[:2]]} {want_ids[bad[:2]]}"


def pose_won(ids):
    return (ids != INSTANCE_NONE) & ((ids & POSE_ID) != 0)


# ---- 1. the shim against the oracle composition, over the case table ----------------------------------------------------------------------
@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_composed_records_and_ids_equal_the_oracle(shim, omodels, vs):
    for n, case in enumerate(PC.table(vs)):
        lengths = (1.0, 0.25, 4.0) if n == 0 else (1.0,)              # the first case: the walk does not care about |d|
        for length in lengths:
            rays = PC.aimed_rays(case, vs, per_entry=max(30, 2000 // max(1, len(case.poses) + len(case.instances))), n_miss=100, seed=40 + n, length=length)
            want, want_ids = PC.expected(case, vs, rays, omodels[vs])
            got, ids = shim.compose(case, vs, rays)
            assert_same(got, ids, want, want_ids, rays, f"{case.name} at vs {vs}, |d| = {length}")
            if len(case.poses) and "behind" not in case.name:
                assert pose_won(want_ids).sum() > 100, case.name
            assert not pose_won(want_ids[-100:]).any()


# ---- 2. no case is vacuous: the frames the GPU test will trace, from the oracle alone ------------------------------------------------------
@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_the_cases_show_what_they_are_for(shim, omodels, vs):
    for case in PC.table(vs) + [PC.corner_case(vs)]:
        rays = O.primary_rays(case.camera(PC.WD, PC.HT), PC.WD, PC.HT)
        per_pose = []
        want, want_ids = PC.expected(case, vs, rays, omodels[vs], per_pose)
        got, ids = shim.compose(case, vs, rays)
        assert_same(got, ids, want, want_ids, rays, f"frame of {case.name} at vs {vs}")
        won = pose_won(want_ids)
        share = won.sum() / len(rays)
        print(f"{case.name} at vs {vs}: poses win {won.sum()} of {len(rays)} pixels")
        assert share >= case.min_pose_share, (case.name, share)
        if case.name.startswith("10"):
            assert per_pose[0].sum() > 200 and not won.any()                     # the pose is there, and the world wins everywhere
        if case.name.startswith("11"):
            assert won.any() and (want_ids[won] == POSE_ID | 0).all()             # the lower index wins every tie
        if case.name.startswith("12"):
            world_px = (want_ids == INSTANCE_NONE) & (want["hit"] == 1)
            assert world_px.any() and (want_ids == 0).any() and won.any()         # the world, a lattice instance and a pose each win a pixel
            assert per_pose[0].sum() > 100 and not (want_ids == POSE_ID | 0).any()   # the instance wins every tie with its own pose
        if case.notes.get("overflow"):
            x, y = np.meshgrid(np.arange(PC.WD), np.arange(PC.HT))
            in_bin = ((x // 32 == 1) & (y // 32 == 0)).reshape(-1)
            assert sum(1 for hit in per_pose if (hit & in_bin).any()) > 63, "more poses in one bin than its list holds"
            assert won.any()
        if case.name == "corner":
            # the slab's silhouette passes within two pixels of the bins' corner at (64, 32): there are winners and losers around it
            block = won.reshape(PC.HT, PC.WD)[29:35, 61:67]
            assert block.any() and not block.all()


# ---- 3. the 48 orientations: a pose made from an instance is the instance -----------------------------------------------------------------
@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_poses_from_instances_equal_the_lattice_instances(shim, omodels, vs):
    rng = np.random.default_rng(9)
    table = np.array([IO.instance(i % 5, rng.integers(-60, 60, size=3), p, f) for i, (p, f) in enumerate(IO.SIGNED_PERMUTATIONS)], dtype=INSTANCE)
    poses = np.concatenate([P.from_instance(inst, vs) for inst in table])
    as_inst = PC.Case("instances", table, np.zeros(0, dtype=POSE), (0, 0, 0), (0, 0, 1))
    as_pose = PC.Case("poses", np.zeros(0, dtype=INSTANCE), poses, (0, 0, 0), (0, 0, 1))
    rays = PC.aimed_rays(as_inst, vs, per_entry=50, n_miss=50, seed=3)
    a, a_ids = shim.compose(as_inst, vs, rays)
    b, b_ids = shim.compose(as_pose, vs, rays)
    for k in ("t", "material_id", "hit"):
        assert a[k].tobytes() == b[k].tobytes(), k
    hit = a_ids != INSTANCE_NONE
    assert hit.sum() > 1000 and len(np.unique(a_ids[hit])) >= 40
    assert ((b_ids == INSTANCE_NONE) == ~hit).all() and (b_ids[hit] == (POSE_ID | a_ids[hit])).all()
    # voxel and face: the pose's local record mapped back by the instance rule is the instance's record
    for j in np.unique(a_ids[hit]):
        sel = np.flatnonzero(a_ids == j)
        m = int(table[j]["model"])
        back = SO.world_records(b[sel], table[j], PC.EXPONENTS[m])
        assert records_equal(back, a[sel]).all(), j
    # and against the oracle, like every other table
    want, want_ids = PC.expected(as_pose, vs, rays, omodels[vs])
    assert_same(b, b_ids, want, want_ids, rays, "48 orientations as poses")


def test_the_three_shims_share_one_candidate(shim, omodels):
    """instance_core.h: placed_candidate is the one statement of a candidate that the three shims walk — instance_shim.cpp (is_compose, voxel size
    1), scaled_instance_shim.cpp (ss_compose) and posed_instance_shim.cpp (ps_compose).  Over the mixed case's lattice instances alone the
    three give the oracle's records, and over its poses the third does."""
    vs = 1.0
    mixed = PC.table(vs)[11]
    lattice = PC.Case("lattice", mixed.instances, np.zeros(0, dtype=POSE), mixed.eye, mixed.target)
    rays = PC.aimed_rays(mixed, vs, per_entry=400, n_miss=100, seed=17)
    want, want_ids = PC.expected(lattice, vs, rays, omodels[vs])
    assert ((want_ids != INSTANCE_NONE).sum() > 300)
    L = shim.lib
    L.is_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    for name in ("is_compose", "ss_compose", "ps_compose"):
        got, ids = np.zeros(len(rays), dtype=O.HIT), np.zeros(len(rays), dtype=np.uint32)
        head = (shim.world(vs), shim.array, len(shim.handles), _p(lattice.instances), len(lattice.instances))
        tail = (_p(rays), len(rays), _p(got), _p(ids))
        if name == "is_compose":
            L.is_compose(*head, *tail)
        elif name == "ss_compose":
            L.ss_compose(*head, vs, *tail)
        else:
            L.ps_compose(*head, None, 0, vs, *tail)
        assert_same(got, ids, want, want_ids, rays, name)
    want, want_ids = PC.expected(mixed, vs, rays, omodels[vs])
    got, ids = shim.compose(mixed, vs, rays)
    assert_same(got, ids, want, want_ids, rays, "ps_compose with poses")
    assert pose_won(want_ids).sum() > 100


# ---- 4. the bins' world box holds the exact preimage ---------------------------------------------------------------------------------------
def contains(box, exact):
    (lo, hi), (elo, ehi) = box, exact
    return all(Fraction(float(lo[j])) <= elo[j] and ehi[j] <= Fraction(float(hi[j])) for j in range(3))


def test_world_box_contains_the_exact_preimage(shim):
    bx = PC.boxes()
    checked = degenerate = 0
    for vs in VOXEL_SIZES:
        for case in PC.table(vs) + [PC.corner_case(vs)]:
            for p in case.poses:
                m = int(p["model"])
                cell = 1 << PC.EXPONENTS[m]
                exact = PO.preimage_box(p, bx[m][0] * cell, bx[m][1] * cell, vs)
                box = shim.world_box(p, shim.handles[m], vs, case.eye)
                if exact is None:
                    assert box is None, case.name                                # rank 2: covers everything
                    degenerate += 1
                else:
                    assert box is not None and contains(box, exact), (case.name, box, exact)
                    size = max(float(exact[1][j] - exact[0][j]) for j in range(3))
                    assert all(float(box[1][j]) - float(box[0][j]) <= float(exact[1][j] - exact[0][j]) + 0.01 * size for j in range(3)), "the margin is a margin, not a blanket"
                    checked += 1
    assert checked > 150 and degenerate == 2
    rng = np.random.default_rng(77)
    covered = 0
    for i in range(200):
        m = int(rng.integers(5))
        scale = 10.0 ** rng.uniform(-2, 3)
        mat = rng.uniform(-1, 1, size=(3, 3)) * scale
        mat = np.clip(mat, -1024, 1024)
        p = PO.pose(m, mat, rng.uniform(-2.0 ** 20, 2.0 ** 20, size=3) * 10.0 ** rng.uniform(-4, 0), rng.uniform(-2.0 ** 20, 2.0 ** 20, size=3) * 10.0 ** rng.uniform(-5, 0))
        vs = VOXEL_SIZES[i % 2]
        rec = np.array([p], dtype=POSE)
        assert shim.lib.ps_usable(_p(rec), shim.handles[m], vs) == 1
        cell = 1 << PC.EXPONENTS[m]
        exact = PO.preimage_box(p, bx[m][0] * cell, bx[m][1] * cell, vs)
        box = shim.world_box(p, shim.handles[m], vs, rng.uniform(-500, 500, size=3))
        if box is not None:
            assert exact is not None and contains(box, exact), (i, p, box, exact)
            covered += 1
    assert covered > 150
    # degenerate matrices: zero, rank 1, rank 2, and one whose determinant is far below its rows' product
    for mat in (np.zeros((3, 3)), [[1, 2, 3], [2, 4, 6], [3, 6, 9]], [[1, 0, 0], [0, 1, 0], [1, 1, 0]], [[1, 0, 0], [0, 1, 0], [1, 1, 1e-7]]):
        assert shim.world_box(PO.pose(0, mat, (1, 2, 3), (0, 0, 0)), shim.handles[0], 1.0, (0, 0, -50)) is None


# ---- 5. the limits -------------------------------------------------------------------------------------------------------------------------
def test_limits(shim):
    good = PO.pose(0, np.eye(3), (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))

    def usable(p, handle=None, vs=1.0):
        rec = np.array([p], dtype=POSE)
        return shim.lib.ps_usable(_p(rec), handle or shim.handles[int(p["model"])], vs), shim.lib.ps_floats_rule(_p(rec))

    assert usable(good) == (1, 0)
    for field, shape, bound, rule in (("m", (3, 3), 1024.0, 2), ("pivot", (3,), 2.0 ** 20, 3), ("local", (3,), 2.0 ** 20, 4)):
        for at in np.ndindex(*shape):
            for bad in (np.nan, np.inf, -np.inf):
                p = good.copy()
                p[field][at] = bad
                assert usable(p) == (0, 1), (field, at, bad)
            p = good.copy()
            p[field][at] = -bound
            assert usable(p) == (1, 0), (field, at)
            p[field][at] = np.nextafter(np.float32(bound), np.float32(np.inf))
            assert usable(p) == (0, rule), (field, at)
    # the model's own voxel box against the int16 lattice, whatever the exponent: [-32768, 32768) is the last usable one
    rec = np.array([good], dtype=POSE)

    def box_usable(lo, hi, e):
        lo, hi = np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32)
        return shim.lib.ps_box_usable(_p(rec), _p(lo), _p(hi), e)

    for e in (0, 2, 6):
        assert box_usable((-32768, -5, 0), (32768, 5, 1), e) == 1
        for axis in range(3):
            lo, hi = [-4, -4, -4], [4, 4, 4]
            hi[axis] = 32769
            assert box_usable(lo, hi, e) == 0, (e, axis)
            hi[axis], lo[axis] = 4, -32769
            assert box_usable(lo, hi, e) == 0, (e, axis)
    # the model's voxel size in this world: vs * 2^e = 256 passes, 512 does not (the store's device copy)
    big = shim.model([(0, 0, 0), (3, 1, 0)], [1, 2], 8)
    assert usable(good, big, 1.0)[0] == 1 and usable(good, big, 2.0)[0] == 0
    shim.lib.is_free(big)
    # an unknown model is skipped by the composition
    case = PC.Case("unknown", np.zeros(0, dtype=INSTANCE), np.array([PO.pose(5, np.eye(3), (0, 0, 0), (0, 0, 0)), PO.pose(0xFFFFFFFF, np.eye(3), (0, 0, 0), (0, 0, 0))], dtype=POSE), (0, 0, 0), (0, 0, 1))
    rays = PC.aimed_rays(PC.Case("aim", np.zeros(0, dtype=INSTANCE), np.array([PO.pose(0, np.eye(3), (0, 0, 0), (0, 0, 0))], dtype=POSE), (0, 0, 0), (0, 0, 1)), 1.0, 200, 0, 1)
    rays["org"][:, 1] += 100.0                                                    # above the world's plate and cloud
    _, ids = shim.compose(case, 1.0, rays)
    assert not pose_won(ids).any()
    # a singular matrix is legal
    assert usable(PO.pose(0, np.zeros((3, 3)), (0, 0, 0), (0, 0, 0))) == (1, 0)


def test_a_ray_that_overflows_does_not_enter_the_pose(shim, omodels):
    """|m| = 1024 and |d| near the top of float32: d' is infinite, the ray is left out, in the shim as in the oracle's mask."""
    p = PO.pose(0, np.eye(3) * 1024.0, (0.0, 100.0, 0.0), (0.0, 0.0, 0.0))
    case = PC.Case("overflow", np.zeros(0, dtype=INSTANCE), np.array([p], dtype=POSE), (0, 0, 0), (0, 0, 1))
    rays = PC.aimed_rays(case, 1.0, 300, 0, 2, reach=1.0)
    rays["dir"][::2] *= np.float32(1e37)
    rays["tmax"][::2] = 1e-30
    out = np.zeros_like(rays)
    ok = np.zeros(len(rays), dtype=np.uint8)
    rec = np.array([p], dtype=POSE)
    shim.lib.ps_transform(_p(rec), _p(rays), len(rays), _p(out), _p(ok))
    want, want_ok = PO.local_rays(rays, p)
    assert (ok.astype(bool) == want_ok).all() and not want_ok[::2].any() and want_ok[1::2].all()
    assert out["org"][want_ok].tobytes() == want["org"][want_ok].tobytes() and out["dir"][want_ok].tobytes() == want["dir"][want_ok].tobytes()
    want, want_ids = PC.expected(case, 1.0, rays, omodels[1.0])
    got, ids = shim.compose(case, 1.0, rays)
    assert_same(got, ids, want, want_ids, rays, "overflowing directions")
    assert not pose_won(ids[::2]).any() and pose_won(ids[1::2]).sum() > 50


def test_shade_face_follows_the_rule(shim):
    rng = np.random.default_rng(4)
    mats = [rng.uniform(-2, 2, size=(3, 3)) for _ in range(40)] + [np.eye(3), -np.eye(3), np.zeros((3, 3)), [[1, 1, 1], [1, -1, 1], [-1, -1, -1]], [[0, 2, -2], [0, 0, 0], [3, 0, -3]]]
    for mat in mats:
        p = PO.pose(0, mat, (0, 0, 0), (0, 0, 0))
        rec = np.array([p], dtype=POSE)
        for face in range(6):
            assert shim.lib.ps_shade_face(_p(rec), face) == PO.shade_face(p, face), (mat, face)
    ident = PO.pose(0, np.eye(3), (0, 0, 0), (0, 0, 0))
    assert [PO.shade_face(ident, f) for f in range(6)] == list(range(6))           # the identity keeps the face


# ---- 6. the host helpers -------------------------------------------------------------------------------------------------------------------
def test_affine_from_pose_equals_affine_from_instance():
    rng = np.random.default_rng(6)
    for vs in (1.0, 0.5, 4.0):
        for p, f in IO.SIGNED_PERMUTATIONS:
            inst = IO.instance(int(rng.integers(9)), rng.integers(-3000, 3000, size=3), p, f)
            pose = P.from_instance(inst, vs)
            for e in range(4):
                assert P.to_affine(pose, vs, e).tobytes() == AF.from_instance(inst, e).tobytes(), (vs, p, f, e)
    with pytest.raises(BlokError):
        P.to_affine(P.from_instance(IO.instance(0, (0, 0, 0)), 1.0), 1.0, 9)
    bad = P.from_instance(IO.instance(0, (0, 0, 0)), 1.0)
    bad["m"][0, 0, 0] = np.nan
    with pytest.raises(BlokError):
        P.to_affine(bad, 1.0, 0)


def test_pose_from_matrix_inverts_the_forward_map():
    import math
    fwd = AF.rotation_matrix(math.radians(30.0), math.radians(10.0), math.radians(-20.0), 1.5, (6.0, 4.5, 3.5), (100.0, 20.0, -50.0))
    p = P.from_matrix(fwd, 3, (6.0, 4.5, 3.5))[0]
    assert int(p["model"]) == 3
    inv = np.linalg.inv(fwd[:, :3])
    assert np.abs(p["m"] - inv).max() <= 2.0 ** -24 * np.abs(inv).max()
    assert np.allclose(p["pivot"], (100.0, 20.0, -50.0)) and np.allclose(p["local"], (6.0, 4.5, 3.5), atol=1e-5)
    same = P.rotation(3, math.radians(30.0), math.radians(10.0), math.radians(-20.0), 1.5, (6.0, 4.5, 3.5), (100.0, 20.0, -50.0))[0]
    assert same.tobytes() == p.tobytes()
    for bad in (np.zeros((3, 4)), np.full((3, 4), np.nan)):
        with pytest.raises(BlokError):
            P.from_matrix(bad)
    with pytest.raises(BlokError):
        P.from_matrix(np.hstack([np.eye(3) * 1e-4, np.zeros((3, 1))]))            # the inverse's elements are above 1024


# ---- 7. the shim alone under the sanitizers ------------------------------------------------------------------------------------------------
def case_file(path, case, vs, rays, want, want_ids):
    wxyz, wm = PC.world_voxels()
    with open(path, "wb") as f:
        mods = PC.models()
        f.write(struct.pack("<I", len(mods)))
        for (xyz, mats), e in zip(mods, PC.EXPONENTS):
            f.write(struct.pack("<II", len(mats), e))
            f.write(np.ascontiguousarray(xyz, dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(mats, dtype="<u4").tobytes())
        f.write(struct.pack("<fI", vs, len(wm)))
        f.write(np.ascontiguousarray(wxyz, dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(wm, dtype="<u4").tobytes())
        for table in (case.instances, case.poses, rays):
            f.write(struct.pack("<I", len(table)))
            f.write(table.tobytes())
        f.write(want.tobytes())
        f.write(want_ids.astype("<u4").tobytes())


def test_shim_under_address_and_ub_sanitizers(tmp_path, omodels):
    """The shim as a stand-alone program (its own main) replays the case table — the rays and the oracle's records, written to files here — and
    its own table of limits.  Nothing loaded into Python is sanitized."""
    exe = tmp_path / "posed_instance_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-DPOSED_INSTANCE_SHIM_MAIN", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}",
                    f"-I{SRC}", "-o", os.fspath(exe), os.fspath(SRC / "posed_instance_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    files = []
    for vs in VOXEL_SIZES:
        for n, case in enumerate(PC.table(vs)):
            rays = PC.aimed_rays(case, vs, per_entry=max(4, 300 // max(1, len(case.poses) + len(case.instances))), n_miss=20, seed=90 + n)
            want, want_ids = PC.expected(case, vs, rays, omodels[vs])
            files.append(tmp_path / f"case_{n}_{vs}.bin")
            case_file(files[-1], case, vs, rays, want, want_ids)
    run = subprocess.run([os.fspath(exe), *map(os.fspath, files)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "posed_instance_shim: ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("won by poses") == len(files)
