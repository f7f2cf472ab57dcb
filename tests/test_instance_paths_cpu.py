"""CPU: the instance BVH of the instanced path frame (blok_amd/csrc/hip/tlas_core.h) against the linear composition, bit for bit.

The header is compiled for the host with instance_core.h and trace_core.h through this test's own shim
(tests/host_harness/tlas_shim.cpp, which includes instance_shim.cpp for the linear loop the instanced primary frame runs)."""
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
NODE = np.dtype([("lo", "<i4", 3), ("hi", "<i4", 3), ("child", "<u4"), ("escape", "<u4")])
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("tlas_shim") / "libtlas_shim.so"
    subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-shared", "-o", os.fspath(out),
                    os.fspath(SRC / "tlas_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    for name in ("is_world", "is_model"):
        getattr(L, name).restype = C.c_void_p
    L.is_world.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_free.argtypes = [C.c_void_p]
    L.is_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ts_max.restype = C.c_uint32
    L.ts_node_count.restype = C.c_uint32
    L.ts_node_count.argtypes = [C.c_uint32]
    L.ts_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p]
    L.ts_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def scene(shim, scene64):
    cm, pw = scene64
    models = IO.procedural_models()
    handles = []
    for xyz, mats in models:
        why = C.c_char_p()
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        h = shim.is_model(_p(xyz), _p(mats), len(mats), C.byref(why))
        assert h, why.value
        handles.append(h)
    why = C.c_char_p()
    wh = shim.is_world(_p(pw.nodes), len(pw.nodes), _p(pw.sub_chunks), len(pw.sub_chunks), C.byref(why))
    assert wh, why.value
    yield wh, handles
    shim.is_free(wh)
    for h in handles:
        shim.is_free(h)


def table_of(n, n_models, seed):
    """n instances over the 64^3 scene with exact duplicates (ties between instances), some unusable records and one outside the lattice."""
    table = IO.random_instances(n, n_models, -8, 64, seed=seed)
    rng = np.random.default_rng(seed + 1)
    if n >= 7:
        for i in rng.choice(n, size=max(1, n // 8), replace=False):
            j = int(rng.integers(n))
            table[i] = table[j]                              # a duplicate: coincident instances
        table[int(rng.integers(n))]["flip"] = 9              # malformed: skipped
        table[int(rng.integers(n))]["offset"] = (32767, 0, 0)     # box leaves the int16 lattice: skipped
        table[int(rng.integers(n))]["model"] = n_models + 3       # unknown model: skipped
    return table


def compose(shim, wh, handles, table, rays, linear=False):
    n = len(rays)
    got = np.zeros(n, dtype=O.HIT)
    ids = np.zeros(n, dtype=np.uint32)
    any_hit = np.zeros(n, dtype=np.uint8)
    alone = np.zeros(n, dtype=np.uint8)
    arr = (C.c_void_p * len(handles))(*handles)
    shim.ts_compose(C.c_void_p(wh), arr, len(handles), _p(table), len(table), _p(rays), n, 1 if linear else 0, _p(got), _p(ids), _p(any_hit), _p(alone))
    return got, ids, any_hit, alone


def linear_reference(shim, wh, handles, table, rays):
    """instance_shim's loop (the instanced primary frame's composition); it cannot take destroyed models or unknown ids."""
    n_models = len(handles)
    ok = np.array([int(t["model"]) < n_models for t in table])
    table = table.copy()
    table["model"][~ok] = 0
    table["flip"][~ok] = 9                                   # still skipped (malformed), and every index keeps its place
    got = np.zeros(len(rays), dtype=O.HIT)
    ids = np.zeros(len(rays), dtype=np.uint32)
    arr = (C.c_void_p * n_models)(*handles)
    shim.is_compose(C.c_void_p(wh), arr, n_models, _p(table), len(table), _p(rays), len(rays), _p(got), _p(ids))
    return got, ids


def rays_for_scene(n=10000, seed=17):
    rays = np.concatenate([edge_case_rays(), random_rays(64, n, seed)])
    return rays[:n]


@pytest.mark.parametrize("n", [1, 7, 64, 1000])
def test_closest_query_equals_the_linear_composition(shim, scene, n):
    wh, handles = scene
    table = table_of(n, len(handles), seed=n)
    rays = rays_for_scene()
    got, ids, any_hit, alone = compose(shim, wh, handles, table, rays)
    want, want_ids = linear_reference(shim, wh, handles, table, rays)
    bad = np.flatnonzero(~records_equal(got, want) | (ids != want_ids))
    assert bad.size == 0, f"{bad.size} of {len(rays)} differ; first ids {ids[bad[:4]]} want {want_ids[bad[:4]]}"
    assert (any_hit == alone).all()
    if n >= 64:
        won = ids != INSTANCE_NONE
        assert won.sum() > 200 and len(np.unique(ids[won])) > 10


def test_duplicates_tie_to_the_lowest_index(shim, scene):
    wh, handles = scene
    base = IO.random_instances(16, len(handles), 0, 56, seed=5)
    # the same instances again in reverse, then the originals: every pixel an instance wins goes to one of the first 16
    table = np.concatenate([base, base[::-1], base])
    rays = rays_for_scene(6000, 23)
    got, ids, _, _ = compose(shim, wh, handles, table, rays)
    want, want_ids = linear_reference(shim, wh, handles, table, rays)
    assert records_equal(got, want).all() and (ids == want_ids).all()
    won = ids != INSTANCE_NONE
    assert won.sum() > 100 and (ids[won] < 16).all()


def test_destroyed_model_and_overflow_fallback(shim, scene):
    wh, handles = scene
    rays = rays_for_scene(4000, 29)
    table = table_of(64, len(handles), seed=64)
    gone = list(handles)
    gone[1] = None                                           # model 1 destroyed: its instances are skipped
    got, ids, any_hit, alone = compose(shim, wh, gone, table, rays)
    lin, lin_ids, _, _ = compose(shim, wh, gone, table, rays, linear=True)
    assert records_equal(got, lin).all() and (ids == lin_ids).all() and (any_hit == alone).all()
    assert not np.isin(ids[ids != INSTANCE_NONE], np.flatnonzero(table["model"] == 1)).any()
    # above kTlasMax the queries take the loop over the table, whose answer is the linear composition
    big = table_of(int(shim.ts_max()) + 1, len(handles), seed=3)
    got, ids, any_hit, alone = compose(shim, wh, handles, big, rays[:1500])
    want, want_ids = linear_reference(shim, wh, handles, big, rays[:1500])
    assert records_equal(got, want).all() and (ids == want_ids).all() and (any_hit == alone).all()


def build(shim, handles, table):
    count = shim.ts_node_count(len(table))
    nodes = np.zeros(count, dtype=NODE)
    arr = (C.c_void_p * len(handles))(*handles)
    shim.ts_build(arr, len(handles), _p(table), len(table), _p(nodes))
    return nodes


def world_box(inst, model_xyz):
    lo, hi = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    for k in range(3):
        a = int(inst["axis"][k])
        o = int(inst["offset"][a])
        mlo, mhi = int(model_xyz[:, k].min()), int(model_xyz[:, k].max()) + 1
        lo[a], hi[a] = (o - mhi, o - mlo) if (int(inst["flip"]) >> k) & 1 else (o + mlo, o + mhi)
    return lo, hi


@pytest.mark.parametrize("n", [1, 7, 64, 1000, 1025])
def test_tree_invariants(shim, scene, n):
    wh, handles = scene
    models = IO.procedural_models()
    table = table_of(n, len(handles), seed=n)
    nodes = build(shim, handles, table)
    P = int(nodes[0]["child"])
    assert P >= n and P & (P - 1) == 0 and len(nodes) == 2 * P
    def is_usable(t):
        if int(t["model"]) >= len(handles) or int(t["flip"]) >= 8:
            return False
        lo, hi = world_box(t, models[int(t["model"])][0])
        return bool((lo >= -32768).all() and (hi <= 32768).all())
    usable = [i for i, t in enumerate(table) if is_usable(t)]
    assert int(nodes[0]["escape"]) == len(usable)
    # every usable instance in exactly one leaf, with its padded box
    leaves = nodes[P:]
    listed = [int(c) & ~LEAF for c in leaves["child"] if int(c) != EMPTY]
    assert sorted(listed) == usable
    for leaf in leaves:
        if int(leaf["child"]) == EMPTY:
            continue
        i = int(leaf["child"]) & ~LEAF
        lo, hi = world_box(table[i], models[int(table[i]["model"])][0])
        assert (leaf["lo"] == lo - 1).all() and (leaf["hi"] == hi + 1).all()
    # a parent's box contains its children's (which carry the padding); a node over no usable leaf is marked empty, so no node the
    # traversal may enter has an inverted box (whose slab test would pass every ray)
    for k in range(1, P):
        for c in (2 * k, 2 * k + 1):
            if int(nodes[c]["child"]) == EMPTY:
                continue
            assert (nodes[k]["lo"] <= nodes[c]["lo"]).all() and (nodes[k]["hi"] >= nodes[c]["hi"]).all()
        empty = int(nodes[2 * k]["child"]) == EMPTY and int(nodes[2 * k + 1]["child"]) == EMPTY
        assert int(nodes[k]["child"]) == (EMPTY if empty else 2 * k)
    live = nodes[1:][nodes[1:]["child"] != EMPTY]
    assert (live["lo"] < live["hi"]).all()
    # the escape links: a walk that always descends visits every node once, in depth-first order
    order, k = [], 1
    while k:
        order.append(k)
        k = 2 * k if k < P else int(nodes[k]["escape"])
    def dfs(k):
        return [k] + (dfs(2 * k) + dfs(2 * k + 1) if k < P else [])
    assert order == dfs(1)
    # skipping a subtree lands on the node after it in that order
    pos = {k: i for i, k in enumerate(order)}
    for k in range(1, 2 * P):
        size = 2 * (P // (1 << (k.bit_length() - 1))) - 1
        nxt = pos[k] + size
        assert int(nodes[k]["escape"]) == (order[nxt] if nxt < len(order) else 0)
    # deterministic
    assert build(shim, handles, table).tobytes() == nodes.tobytes()
