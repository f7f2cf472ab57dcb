"""CPU: instanced models at power-of-two scales (include/blok_hip.h, "Scaled models") — the kernels' instance math and instance BVH
(blok_amd/csrc/hip/instance_core.h, tlas_core.h) compiled for the host through tests/host_harness/scaled_instance_shim.cpp, against the
oracle helper tests/scaled_instance_oracle.py, bit for bit."""
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
from tests import scaled_instance_oracle as SO
from tests.conftest import records_equal

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
FLAGS = ["-O1", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}"]
TLAS_NODE = np.dtype([("lo", "<i4", 3), ("hi", "<i4", 3), ("child", "<u4"), ("escape", "<u4")])
TLAS_LEAF, TLAS_PAD = 0x80000000, 1


def build_shim(out: Path) -> C.CDLL:
    """The shim as a shared library with its entries typed (test_scaled_instances_gpu.py uses it for the host BVH too)."""
    subprocess.run(["g++", *FLAGS, "-shared", "-o", os.fspath(out), os.fspath(SRC / "scaled_instance_shim.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    L.is_model.restype = C.c_void_p
    L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_free.argtypes = [C.c_void_p]
    L.ss_set_scale.argtypes = [C.c_void_p, C.c_uint32]
    L.ss_scale.argtypes = [C.c_void_p]
    L.ss_scale.restype = C.c_uint32
    L.ss_usable.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
    L.ss_span.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ss_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ss_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]
    L.ss_closest.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ts_node_count.argtypes = [C.c_uint32]
    L.ts_node_count.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("scaled_instance_shim") / "libscaled_instance_shim.so")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def shim_model(shim, xyz, mats, exponent=0):
    why = C.c_char_p()
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    mats = np.ascontiguousarray(mats, dtype=np.uint32)
    h = shim.is_model(_p(xyz), _p(mats), len(mats), C.byref(why))
    assert h, why.value
    h = C.c_void_p(h)
    assert shim.ss_set_scale(h, exponent) == 0
    return h


def handle_array(handles):
    return (C.c_void_p * len(handles))(*[h.value for h in handles])


def box_of(xyz):
    return xyz.min(axis=0), xyz.max(axis=0) + 1


def aimed_rays(table, boxes, exponents, voxel_size, per_instance, n_miss, seed, reach=300.0):
    """Rays from seeded origins towards a seeded point of each instance's world box, and n_miss rays that point away from all of them."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(len(table) * per_instance + n_miss, dtype=O.RAY)
    org = rng.uniform(-reach, reach, size=(len(rays), 3))
    tgt = rng.uniform(-reach, reach, size=(len(rays), 3))
    for i, inst in enumerate(table):
        m = int(inst["model"])
        lo, hi = SO.world_span(inst, boxes[m][0], boxes[m][1], exponents[m])
        tgt[i * per_instance:(i + 1) * per_instance] = rng.uniform(lo, hi, size=(per_instance, 3))
    if n_miss:
        org[-n_miss:] = rng.uniform(4 * reach, 5 * reach, size=(n_miss, 3))
        tgt[-n_miss:] = org[-n_miss:] + rng.uniform(0.1, 1.0, size=(n_miss, 3))        # onwards, away from everything
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["org"] = (org * voxel_size).astype(np.float32)
    rays["dir"] = d.astype(np.float32)
    rays["tmin"] = 0.001
    rays["tmax"] = 10000.0
    return rays


def all_orientations_table(n_models, lo, hi, seed):
    """48 instances, one per signed permutation, models in turn, seeded offsets (not multiples of any cell size)."""
    rng = np.random.default_rng(seed)
    return np.array([IO.instance(i % n_models, rng.integers(lo, hi, size=3), p, f) for i, (p, f) in enumerate(IO.SIGNED_PERMUTATIONS)], dtype=INSTANCE)


@pytest.mark.parametrize("voxel_size, exponents", [(1.0, (0, 1, 2, 3)), (0.5, (2, 2, 2, 2))])
def test_composed_records_and_ids_equal_the_oracle(shim, voxel_size, exponents):
    models = IO.procedural_models()
    omodels = [SO.scaled_model(xyz, mats, e, voxel_size) for (xyz, mats), e in zip(models, exponents)]
    handles = [shim_model(shim, xyz, mats, e) for (xyz, mats), e in zip(models, exponents)]
    boxes = [box_of(xyz) for xyz, _ in models]
    table = all_orientations_table(len(models), -90, 90, seed=5)
    assert len(table) == 48 and (table["offset"] % 8 != 0).any()
    rays = aimed_rays(table, boxes, exponents, voxel_size, per_instance=40, n_miss=80, seed=6)
    assert len(rays) == 2000
    world = np.zeros(len(rays), dtype=O.HIT)                     # no world: every ray starts as a miss
    want, want_ids = SO.compose(world, rays, table, omodels, exponents, voxel_size)
    got = np.zeros(len(rays), dtype=O.HIT)
    ids = np.zeros(len(rays), dtype=np.uint32)
    shim.ss_compose(None, handle_array(handles), len(handles), _p(table), len(table), voxel_size, _p(rays), len(rays), _p(got), _p(ids))
    bad = np.flatnonzero(~records_equal(got, want) | (ids != want_ids))
    assert bad.size == 0, f"{bad.size} of {len(rays)} differ; first: {rays[bad[:3]]} got {got[bad[:3]]} ids {ids[bad[:3]]} want {want[bad[:3]]} {want_ids[bad[:3]]}"
    # what the test is for is there: most aimed rays hit, every orientation and every model wins somewhere, the misses miss
    won = ids != INSTANCE_NONE
    assert won[:-80].sum() > 1200 and not won[-80:].any()
    assert len(np.unique(ids[won])) >= 44                  # (a thin model may sit behind its neighbours)
    # the voxel is the lowest world voxel of a cell of the winner's size, inside its span
    for i in np.flatnonzero(won)[::7]:
        inst = table[ids[i]]
        m = int(inst["model"])
        lo, hi = SO.world_span(inst, boxes[m][0], boxes[m][1], exponents[m])
        v = got["voxel"][i].astype(np.int64)
        assert (v >= lo).all() and (v + (1 << exponents[m]) <= hi).all()
        assert ((v - inst["offset"]) % (1 << exponents[m]) == 0).all()
    for h in handles:
        shim.is_free(h)


def test_limits(shim):
    m = shim_model(shim, np.array([[0, 0, 0], [3, 1, 0]]), np.array([1, 2]), 3)        # box [0, 4) x [0, 2) x [0, 1) cells of 8 voxels

    def usable(vs, *placement):
        rec = np.ascontiguousarray(np.array([IO.instance(0, *placement)], dtype=INSTANCE))
        return shim.ss_usable(_p(rec), m, vs)

    # a span ending exactly at 32768 is usable, one cell (here: one voxel of offset) further is not
    assert usable(1.0, (32768 - 32, 0, 0)) == 1
    assert usable(1.0, (32768 - 31, 0, 0)) == 0
    assert usable(1.0, (32768 - 24, 0, 0)) == 0                        # one whole cell further
    assert usable(1.0, (0, 32768 - 16, 0)) == 1 and usable(1.0, (0, 32768 - 15, 0)) == 0
    # the same at -32768 with a flip: the span is [o - 32, o)
    assert usable(1.0, (-32768 + 32, 0, 0), (0, 1, 2), 1) == 1
    assert usable(1.0, (-32768 + 31, 0, 0), (0, 1, 2), 1) == 0
    assert usable(1.0, (-32768 + 24, 0, 0), (0, 1, 2), 1) == 0
    # at scale 0 the same offsets are far inside
    assert shim.ss_set_scale(m, 0) == 0 and usable(1.0, (32768 - 24, 0, 0)) == 1
    # vs * 2^e = 256 is usable, 512 is not
    assert shim.ss_set_scale(m, 3) == 0
    assert usable(32.0, (0, 0, 0)) == 1 and usable(64.0, (0, 0, 0)) == 0
    assert shim.ss_set_scale(m, 8) == 0
    assert usable(1.0, (0, 0, 0)) == 1 and usable(2.0, (0, 0, 0)) == 0
    # an exponent of 9 is refused and changes nothing
    assert shim.ss_set_scale(m, 9) == -1 and shim.ss_scale(m) == 8
    shim.is_free(m)


@pytest.mark.parametrize("n", [7, 64, 1000])
def test_host_bvh_with_mixed_scales(shim, n):
    models = IO.procedural_models()
    exponents = (0, 1, 2, 3)
    handles = [shim_model(shim, xyz, mats, e) for (xyz, mats), e in zip(models, exponents)]
    boxes = [box_of(xyz) for xyz, _ in models]
    reach = 60 if n < 100 else 400
    table = IO.random_instances(n, len(models), -reach, reach, seed=20 + n)
    arr = handle_array(handles)
    nodes = np.zeros(shim.ts_node_count(n), dtype=TLAS_NODE)
    shim.ss_build(arr, len(handles), _p(table), n, 1.0, _p(nodes))
    slots = int(nodes[0]["child"])
    assert slots == 1 << (n - 1).bit_length() and int(nodes[0]["escape"]) == n
    leaves = nodes[slots:]
    used = leaves[leaves["child"] != 0xFFFFFFFF]
    assert sorted(used["child"] & ~np.uint32(TLAS_LEAF)) == list(range(n))
    for leaf in used:                                            # leaf box = the scaled span, padded by one world voxel
        inst = table[int(leaf["child"]) & 0x7FFFFFFF]
        m = int(inst["model"])
        lo, hi = SO.world_span(inst, boxes[m][0], boxes[m][1], exponents[m])
        assert (leaf["lo"] == lo - TLAS_PAD).all() and (leaf["hi"] == hi + TLAS_PAD).all()
    # the tree's winners are the linear loop's, record for record
    rays = aimed_rays(table[:: max(1, n // 50)], boxes, exponents, 1.0, per_instance=12, n_miss=40, seed=n, reach=1.5 * reach)
    lin = np.zeros(len(rays), dtype=O.HIT)
    lin_ids = np.zeros(len(rays), dtype=np.uint32)
    shim.ss_compose(None, arr, len(handles), _p(table), n, 1.0, _p(rays), len(rays), _p(lin), _p(lin_ids))
    tree = np.zeros(len(rays), dtype=O.HIT)
    tree_ids = np.zeros(len(rays), dtype=np.uint32)
    any_hit = np.zeros(len(rays), dtype=np.uint8)
    shim.ss_closest(arr, len(handles), _p(table), n, 1.0, _p(rays), len(rays), _p(tree), _p(tree_ids), _p(any_hit))
    assert (tree_ids == lin_ids).all() and records_equal(tree, lin).all()
    assert ((any_hit == 1) == (lin_ids != INSTANCE_NONE)).all()
    assert (lin_ids != INSTANCE_NONE).sum() > len(rays) // 3
    for h in handles:
        shim.is_free(h)


def test_shim_under_address_and_ub_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main): mixed exponents, all 48 orientations, both voxel sizes, the tree against the
    loop, the limits.  Nothing loaded into Python is sanitized."""
    exe = tmp_path / "scaled_instance_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-DSCALED_INSTANCE_SHIM_MAIN", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}",
                    f"-I{SRC}", "-o", os.fspath(exe), os.fspath(SRC / "scaled_instance_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    run = subprocess.run([os.fspath(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "scaled_instance_shim: ok" in run.stdout, run.stdout + run.stderr
