"""CPU: the lit path loop (blok_amd/csrc/hip/path_core.h: shade_pixel<…, kLit>, light_sample) compiled for the host through
tests/host_harness/lit_paths_shim.cpp: without a table the posed superset body gives the world-only body's frame byte for byte; the light
sample against the numpy float32 restatement of tests/lights_reference.py bit for bit; the bookkeeping of what a diffuse bounce ray may
count, scripted through the materials' lobes; the stand-alone program under ASan + UBSan."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, LIGHT, MATERIAL, POSE
from tests import harness_ffi as H
from tests import lights_cases as LC
from tests import lights_reference as LR
from tests.test_posed_instances_cpu import FLAGS, ROOT, SRC

f32 = np.float32
PLANES = ("color", "world_pos", "normal_roughness", "albedo_metallic")
GREY, GLOW, GLOW2, DARK, MIRROR, TWIN = 1, 2, 3, 4, 5, 6


def materials():
    """1 grey and rough, 2 and 3 glowing, 4 black, 5 a metal (its lobe choice is always the specular one: spec_w = 1), 6 material 3's twin."""
    m = np.zeros(7, dtype=MATERIAL)
    m["albedo"] = (0.6, 0.6, 0.6)
    m["flags"] = 230 << 16
    m["ior"] = 1.5
    m["emission"][GLOW] = (4.0, 3.0, 2.0)
    m["emission"][GLOW2] = (1.0, 2.0, 6.0)
    m["emission"][TWIN] = (1.0, 2.0, 6.0)
    m["albedo"][DARK] = (0.0, 0.0, 0.0)
    m["flags"][MIRROR] = (255 << 24) | (60 << 16)
    return m


def voxels_of(d, m, origin=(0, 0, 0)):
    z, y, x = np.nonzero(d > 0)
    xyz = np.stack([x + origin[0], y + origin[1], z + origin[2]], -1).astype(np.int32)
    return xyz, m[z, y, x].astype(np.uint32)


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and len(a) else None


class LitShim:
    def __init__(self, out):
        subprocess.run(["g++", *FLAGS, "-shared", "-o", os.fspath(out), os.fspath(SRC / "lit_paths_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
        L = C.CDLL(os.fspath(out))
        L.is_model.restype = C.c_void_p
        L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
        L.is_free.argtypes = [C.c_void_p]
        L.lp_render.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 +
                                [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 5)
        L.lp_light_sample.restype = C.c_int
        L.lp_light_sample.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib = L

    def tree(self, xyz, ids):
        why = C.c_char_p()
        xyz, ids = np.ascontiguousarray(xyz, dtype=np.int32), np.ascontiguousarray(ids, dtype=np.uint32)
        h = self.lib.is_model(_ptr(xyz), _ptr(ids), len(ids), C.byref(why))
        assert h, why.value
        return C.c_void_p(h)

    def render(self, world, models, inst, poses, cam, mats, w, h, spp, bounces, frame, table=None, vs=1.0):
        """The planes dict plus "ids"; table: LIGHT records (None or empty: no table)."""
        planes = {k: np.zeros((h, w, 4), dtype=f32) for k in PLANES}
        ids = np.zeros((h, w), dtype=np.uint32)
        handles = (C.c_void_p * max(1, len(models)))(*[m.value for m in models])
        inst = np.ascontiguousarray(inst if inst is not None else [], dtype=INSTANCE).reshape(-1)
        poses = np.ascontiguousarray(poses if poses is not None else [], dtype=POSE).reshape(-1)
        mats = np.ascontiguousarray(mats, dtype=MATERIAL)
        cam = np.ascontiguousarray(cam)
        n, faces, area, owned = 0, 0, 0.0, None
        if table is not None and len(table):
            table = np.ascontiguousarray(table, dtype=LIGHT)
            n = len(table)
            faces = int((table["du"].astype(np.int64) * table["dv"]).sum())
            area = float(f32(faces) * f32(vs) * f32(vs))
            owned = np.zeros(2048, dtype=np.uint32)
            for i in LR.material_index(table["material"], len(mats)):
                owned[i >> 5] |= np.uint32(1 << (i & 31))
        self.lib.lp_render(world, handles, len(models), _ptr(inst), len(inst), _ptr(poses), len(poses), vs, _ptr(cam), _ptr(mats), len(mats), w, h, spp, bounces, frame,
                           _ptr(table) if n else None, n, _ptr(owned) if n else None, faces, area, *[_ptr(planes[k]) for k in PLANES], _ptr(ids))
        planes["ids"] = ids
        return planes


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return LitShim(tmp_path_factory.mktemp("lit") / "liblit_paths_shim.so")


# ---- the scenes (tests/test_lit_paths_gpu.py renders the same ones on the device) ----
def mixed_scene():
    """A floor, a wall, a glowing plate over the floor and a glowing block of the other material on it, in a 32^3 box."""
    d = np.zeros((32, 32, 32), dtype=f32)
    m = np.zeros((32, 32, 32), dtype=np.uint32)
    d[:, 0:2, :] = 1.0
    m[:, 0:2, :] = GREY
    d[24:26, 2:20, 4:28] = 1.0
    m[24:26, 2:20, 4:28] = GREY
    d[12:16, 12, 12:16] = 1.0
    m[12:16, 12, 12:16] = GLOW
    d[8:10, 2:4, 20:22] = 1.0
    m[8:10, 2:4, 20:22] = GLOW2
    return d, m


MIXED_CAM = ((6.5, 13.3, -7.2), (16.0, 3.0, 15.0))


def mixed_models():
    cube = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    return cube, np.full(len(cube), GREY, dtype=np.uint32)


def room(wall=GREY, patch=GLOW2):
    """A closed 14^3 room with walls of `wall`, a ceiling two voxels thick and a 4 x 4 glowing patch in it."""
    d = np.ones((14, 14, 14), dtype=f32)
    m = np.full((14, 14, 14), wall, dtype=np.uint32)
    d[1:13, 1:12, 1:13] = 0.0
    m[5:9, 12, 5:9] = patch
    return d, m


def room_table(material):
    t = np.zeros(1, dtype=LIGHT)
    t["lo"], t["du"], t["dv"], t["material"], t["face"] = (5, 12, 5), 4, 4, material, 3
    return t


ROOM_CAM = ((7.0, 8.0, 2.5), (7.0, 1.0, 8.0))


# ---- 1. no table: the posed superset body is the world-only body ----
def test_without_a_table_the_frame_is_the_world_only_bodys(shim):
    d, m = mixed_scene()
    xyz, ids = voxels_of(d, m)
    cm = W.ChunkManager(128, 1.0)
    cm.set_voxels(xyz, ids)
    cm.rebuild_dirty_chunks()
    mats = materials()
    pw = cm.pack_chunks_to_gpu_svo(mats)
    w, h = 32, 24
    cam = W.camera_look_at(*MIXED_CAM, 60.0, w, h)
    want = H.HostKernel(pw.nodes, pw.sub_chunks).render_paths(cam, mats, w, h, spp=2, max_bounces=3, frame_index=4)
    world = shim.tree(xyz, ids)
    got = shim.render(world, [], None, None, cam, mats, w, h, 2, 3, 4)
    for k in PLANES:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert (got["ids"] == 0xFFFFFFFF).all()
    assert shim.render(world, [], None, None, cam, mats, w, h, 2, 3, 4, table=np.zeros(0, dtype=LIGHT))["color"].tobytes() == want["color"].tobytes()
    # with a table the G-buffer stays and the colour moves
    quads = LC.quads_of(LC.Case("mixed", (0, 0, 0), (32, 32, 32), d, m, mats))
    table, info = LT.host_from_quads(quads, mats)
    assert int(info["n_owned"][0]) == 2
    lit = shim.render(world, [], None, None, cam, mats, w, h, 2, 3, 4, table=table)
    for k in PLANES[1:]:
        assert lit[k].tobytes() == want[k].tobytes(), k
    assert (lit["color"] != want["color"]).any() and np.isfinite(lit["color"]).all()
    shim.lib.is_free(world)


# ---- 2. the light sample, bit for bit ----
def r_for_pick(pick: int, faces: int) -> int:
    """The smallest 32-bit r that selects unit face `pick` of `faces`."""
    r = -((-pick << 32) // faces)
    assert LR.pick_of(r, faces) == pick and r < 2 ** 32
    return r


@pytest.mark.parametrize("case", [c for c in LC.table() if c.n_lights], ids=[c.name for c in LC.table() if c.n_lights])
def test_light_sample_equals_the_numpy_restatement(shim, case):
    """Every light of the case, a cell of it, from points on all six normals around it, at two voxel sizes: q, Le and g of light_sample equal
    the float32 restatement bit for bit, and so does the answer "no term"."""
    mats = np.ascontiguousarray(case.materials)
    table, info = LT.host_from_quads(LC.quads_of(case), mats)
    faces = int(info["n_faces"][0])
    rng = np.random.default_rng(len(table))
    q, le, g = np.zeros(3, dtype=f32), np.zeros(3, dtype=f32), np.zeros(1, dtype=f32)
    normals = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=f32)
    with_term = without = 0
    for vs in (1.0, 0.5):
        area = f32(faces) * f32(vs) * f32(vs)
        for i in range(len(table)):
            light = table[i]
            off = int(rng.integers(0, int(light["du"]) * int(light["dv"])))
            pick = int(light["cum"]) + off
            r = r_for_pick(pick, faces)
            assert LR.find_light(table, pick) == i
            u1, u2 = f32(rng.random()), f32(rng.random())
            centre, nl = LR.sample_point(light, off, 0.5, 0.5, vs)
            for n in normals:
                # a surface point some way off in front of, beside or behind the light, facing along n
                hit_pos = (centre + nl * f32(vs) * f32(rng.uniform(-1.0, 6.0)) + rng.uniform(-5.0, 5.0, 3).astype(f32) * f32(vs)).astype(f32)
                has = shim.lib.lp_light_sample(_ptr(table), len(table), faces, float(area), _ptr(mats), len(mats), vs, _ptr(hit_pos), _ptr(n), r, float(u1), float(u2),
                                               _ptr(q), _ptr(le), _ptr(g))
                wq, wnl = LR.sample_point(light, off, u1, u2, vs)
                wg, _, _, _ = LR.geometry(hit_pos, n, wq, wnl, area)
                assert q.tobytes() == wq.tobytes()
                assert bool(has) == bool(wg > 0)
                if wg > 0:
                    want_le = mats["emission"][int(LR.material_index(light["material"], len(mats)))].astype(f32)
                    assert g.tobytes() == np.array([wg], dtype=f32).tobytes() and le.tobytes() == want_le.tobytes()
                    with_term += 1
                else:
                    without += 1
    print(f"{case.name}: {with_term} samples with a term, {without} without")
    assert with_term > 0 and without > 0


# ---- 3. what a diffuse bounce ray may count ----
def test_prev_diffuse_bookkeeping_by_scripted_lobes(shim):
    """Two tables over the same room, equal but for the material id their light names: GLOW2 (the patch's own id: owned) or its twin (the same
    emission under an id that does not occur in the world: nothing owned).  Both draw the same random numbers.  Owned, a diffuse bounce
    ray that finds the patch adds nothing; not owned, it adds throughput x emission on top.
      - grey walls (lobes mostly diffuse), 2 bounces: the twin's frame is >= the owned frame everywhere and > somewhere;
      - metal walls (every lobe specular, no hit eligible): both frames equal the frame without a table, byte for byte;
      - one bounce (no ray is ever a bounce ray): the two frames are equal."""
    mats = materials()
    w, h = 24, 18
    cam = W.camera_look_at(*ROOM_CAM, 70.0, w, h)
    d, m = room(GREY)
    world = shim.tree(*voxels_of(d, m))
    owned = shim.render(world, [], None, None, cam, mats, w, h, 4, 2, 1, table=room_table(GLOW2))["color"]
    twin = shim.render(world, [], None, None, cam, mats, w, h, 4, 2, 1, table=room_table(TWIN))["color"]
    assert (twin >= owned).all() and (twin > owned).any()
    print(f"grey walls: {int((twin > owned).any(-1).sum())} of {w * h} pixels hold a doubly counted hit in the twin's frame")
    one_a = shim.render(world, [], None, None, cam, mats, w, h, 4, 1, 1, table=room_table(GLOW2))["color"]
    one_b = shim.render(world, [], None, None, cam, mats, w, h, 4, 1, 1, table=room_table(TWIN))["color"]
    assert one_a.tobytes() == one_b.tobytes()
    shim.lib.is_free(world)
    d, m = room(MIRROR)
    world = shim.tree(*voxels_of(d, m))
    bare = shim.render(world, [], None, None, cam, mats, w, h, 4, 3, 1)["color"]
    for material in (GLOW2, TWIN):
        assert shim.render(world, [], None, None, cam, mats, w, h, 4, 3, 1, table=room_table(material))["color"].tobytes() == bare.tobytes()
    assert (bare[..., :3] > 0).any()
    shim.lib.is_free(world)


# ---- 4. sanitizers ----
def test_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "lit_paths_shim"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", "-DLIT_PATHS_SHIM_MAIN", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-o",
                    os.fspath(exe), os.fspath(SRC / "lit_paths_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    run = subprocess.run([os.fspath(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "lit_paths_shim: ok" in run.stdout, run.stdout + run.stderr
