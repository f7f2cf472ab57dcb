"""CPU: the instance math of the kernels (blok_amd/csrc/hip/instance_core.h) against the oracle, bit for bit.

The header is compiled for the host together with trace_core.h through this test's own shim (tests/host_harness/instance_shim.cpp).
The expected records come from the existing oracle alone (tests/instance_oracle.py): each instance's model traced by itself on rays
moved into its local space in numpy, mapped back and composed with the world's records by the tie rule."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd._ffi import INSTANCE, INSTANCE_NONE
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests.conftest import edge_case_rays, random_rays, records_equal

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
HDRS = ["instance_core.h", "trace_core.h", "trace_kernels.h", "tree.h", "reference_world.h"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("instance_shim") / "libinstance_shim.so"
    subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-shared", "-o", os.fspath(out),
                    os.fspath(SRC / "instance_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    for name in ("is_world", "is_model"):
        getattr(L, name).restype = C.c_void_p
    L.is_world.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_free.argtypes = [C.c_void_p]
    L.is_transform.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    L.is_map_back.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.is_usable.argtypes = [C.c_void_p, C.c_void_p]
    L.is_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _inst(rec):
    return np.ascontiguousarray(np.array([rec], dtype=INSTANCE))


def _model(shim, xyz, mats):
    why = C.c_char_p()
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    mats = np.ascontiguousarray(mats, dtype=np.uint32)
    h = shim.is_model(_p(xyz), _p(mats), len(mats), C.byref(why))
    assert h, why.value
    return C.c_void_p(h)


def test_record_layout():
    assert INSTANCE.itemsize == 32
    assert INSTANCE.fields["flip"][1] == 19 and INSTANCE.fields["reserved"][1] == 20


@pytest.mark.parametrize("voxel_size", [1.0, 0.5])
def test_transform_and_map_back_all_48_orientations(shim, voxel_size):
    rng = np.random.default_rng(11)
    rays = np.concatenate([edge_case_rays(), random_rays(64, 2000, 5)])
    rays["org"] += rng.normal(scale=3.0, size=(len(rays), 3)).astype(np.float32)        # origins with low bits to lose
    local = np.zeros(500, dtype=O.HIT)
    local["t"] = rng.uniform(0, 100, 500).astype(np.float32)
    local["material_id"] = rng.integers(1, 1000, 500)
    local["voxel"] = rng.integers(-300, 300, size=(500, 3))
    local["face"] = rng.integers(0, 6, 500)
    local["hit"] = 1
    assert len(IO.SIGNED_PERMUTATIONS) == 48
    for axis, flip in IO.SIGNED_PERMUTATIONS:
        inst = _inst(IO.instance(0, rng.integers(-2000, 2000, size=3), axis, flip))
        got = np.zeros(len(rays), dtype=O.RAY)
        shim.is_transform(_p(inst), voxel_size, _p(rays), len(rays), _p(got))
        want = IO.local_rays(rays, inst[0], voxel_size)
        assert (got.view(np.uint8) == want.view(np.uint8)).all(), (axis, flip)
        back = np.zeros(len(local), dtype=O.HIT)
        shim.is_map_back(_p(inst), _p(local), len(local), _p(back))
        assert records_equal(back, IO.world_records(local, inst[0])).all(), (axis, flip)
        # a local voxel and its world image cover the same box: the local ray of the world box's centre lies in the local voxel
        w = back["voxel"][:1].astype(np.float64)
        centre = np.zeros(1, dtype=O.RAY)
        centre["org"] = ((w + 0.5) * voxel_size).astype(np.float32)
        loc = IO.local_rays(centre, inst[0], voxel_size)
        assert (np.floor(loc["org"][0] / voxel_size).astype(np.int64) == local["voxel"][0]).all(), (axis, flip)


def test_limits(shim):
    m = _model(shim, np.array([[0, 0, 0], [9, 3, 1]]), np.array([1, 2]))
    ok = IO.instance(0, (32758, -32768, 0), (0, 1, 2), 0)                        # box [32758, 32768) x [-32768, -32764) x [0, 2)
    assert shim.is_usable(_p(_inst(ok)), m) == 1
    for bad in (IO.instance(0, (32759, 0, 0)), IO.instance(0, (0, -32768, 0), (0, 1, 2), 2),
                IO.instance(0, (0, 0, 0), (0, 0, 2)), IO.instance(0, (0, 0, 0), (0, 1, 3))):
        assert shim.is_usable(_p(_inst(bad)), m) == 0
    rec = IO.instance(0, (0, 0, 0))
    rec["reserved"][1] = 1
    assert shim.is_usable(_p(_inst(rec)), m) == 0
    rec = IO.instance(0, (0, 0, 0))
    rec["flip"] = 8
    assert shim.is_usable(_p(_inst(rec)), m) == 0
    shim.is_free(m)


def scene_instances(n_models):
    """40 instances over scene64: seeded ones, some sunk into the terrain, overlapping pairs, exact duplicates (ties between instances)
    and one coincident with a world voxel block (ties with the world)."""
    table = IO.random_instances(30, n_models, -4, 60, seed=3)
    rng = np.random.default_rng(4)
    extra = []
    for i in range(4):                                   # exact duplicates of earlier instances: a tie, the lower index wins
        extra.append(table[int(rng.integers(30))].copy())
    for i in range(3):                                   # overlapping neighbours
        base = table[i].copy()
        base["offset"] = base["offset"] + rng.integers(-3, 4, size=3)
        extra.append(base)
    for p, f in [((2, 0, 1), 5), ((1, 2, 0), 0), ((0, 1, 2), 7)]:
        extra.append(IO.instance(0, (20, 0, 20), p, f))   # sunk into the ground
    return np.concatenate([table, np.array(extra, dtype=INSTANCE)])


def test_composition_equals_oracle(shim, scene64):
    cm, pw = scene64
    models = IO.procedural_models()
    omodels = [IO.OracleModel(xyz, mats) for xyz, mats in models]
    handles = [_model(shim, xyz, mats) for xyz, mats in models]
    table = scene_instances(len(models))
    assert len(table) == 40
    rays = np.concatenate([edge_case_rays(), random_rays(64, 9000, 17)])
    world, ctr = O.Lattice(pw.nodes, pw.sub_chunks).trace(rays, threads=8)
    want, want_ids = IO.compose(world, rays, table, omodels)
    why = C.c_char_p()
    wh = C.c_void_p(shim.is_world(_p(pw.nodes), len(pw.nodes), _p(pw.sub_chunks), len(pw.sub_chunks), C.byref(why)))
    got = np.zeros(len(rays), dtype=O.HIT)
    ids = np.zeros(len(rays), dtype=np.uint32)
    arr = (C.c_void_p * len(handles))(*[h.value for h in handles])
    shim.is_compose(wh, arr, len(handles), _p(table), len(table), _p(rays), len(rays), _p(got), _p(ids))
    bad = np.flatnonzero(~records_equal(got, want) | (ids != want_ids))
    assert bad.size == 0, f"{bad.size} of {len(rays)} differ; first: {rays[bad[:3]]} got {got[bad[:3]]} ids {ids[bad[:3]]} want {want[bad[:3]]} {want_ids[bad[:3]]}"
    # the cases the test is for are all there
    won = ids != INSTANCE_NONE
    assert won.sum() > 500 and (world["hit"][won] == 1).sum() > 50        # instances in front of terrain
    assert len(np.unique(ids[won])) > 20
    dup_ties = 0
    for i in range(30, 34):                              # the duplicates never win: their twin has the lower index
        assert not (ids == i).any()
    for i in range(30, 34):
        twin = next(j for j in range(30) if table[j].tobytes() == table[i].tobytes())
        dup_ties += int((ids == twin).sum())
    assert dup_ties > 0
    shim.is_free(wh)
    for h in handles:
        shim.is_free(h)


def test_world_tie_goes_to_the_world(shim):
    """A model voxel exactly where a world voxel is (integer offset, identity orientation, ray origins whose subtraction is exact): the
    same t on both sides, and the world keeps the pixel."""
    world_xyz = np.array([(x, 0, z) for x in range(8) for z in range(8)], dtype=np.int32)
    wm = np.full(len(world_xyz), 3, dtype=np.uint32)
    m = _model(shim, np.array([(0, 0, 0), (1, 0, 0)]), np.array([9, 9]))
    w = _model(shim, world_xyz, wm)
    table = np.array([IO.instance(0, (4, 0, 4))], dtype=INSTANCE)
    rays = np.zeros(3, dtype=O.RAY)
    rays["org"] = [(4.5, 5.0, 4.5), (5.25, 3.0, 4.5), (4.5, 2.0, 4.75)]
    rays["dir"] = [(0, -1, 0), (0, -1, 0), (0, -1, 0)]
    rays["tmin"] = 0.001
    rays["tmax"] = 10000.0
    got = np.zeros(3, dtype=O.HIT)
    ids = np.zeros(3, dtype=np.uint32)
    arr = (C.c_void_p * 1)(m.value)
    shim.is_compose(w, arr, 1, _p(table), 1, _p(rays), 3, _p(got), _p(ids))
    assert (got["hit"] == 1).all() and (got["material_id"] == 3).all() and (ids == INSTANCE_NONE).all()
    table[0]["offset"] = (4, 1, 4)                        # one voxel up: the instance is in front
    shim.is_compose(w, arr, 1, _p(table), 1, _p(rays), 3, _p(got), _p(ids))
    assert (got["material_id"] == 9).all() and (ids == 0).all() and (got["voxel"][:, 1] == 1).all()
    shim.is_free(m)
    shim.is_free(w)
