"""CPU: the lit path loop over lattice instances whose models carry light tables (blok_amd/csrc/hip/path_core.h:
shade_pixel<…, kLit, kPlacedLit>, placed_light_sample) compiled for the host through tests/host_harness/model_lights_paths_shim.cpp.
Without a model table, and with tables that carry no light, it gives the lit body's bytes (the posed body's where there is no world
table either); with one bounce a frame over lit instances equals its set_lights twin byte for byte in every plane; with three bounces and
the same seeds it is never brighter than the twin and darker somewhere."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, INSTANCE_LIGHTS_INFO, LIGHT, MATERIAL, POSE
from tests import instance_oracle as IO
from tests import lights_reference as LR
from tests import model_lights_cases as MC
from tests.test_lit_paths_cpu import LitShim, _ptr, voxels_of
from tests.test_posed_instances_cpu import FLAGS, ROOT, SRC

f32 = np.float32
PLANES = ("color", "world_pos", "normal_roughness", "albedo_metallic")
WD, HT = 32, 24
CAM = ((4.5, 13.0, -7.0), (16.0, 3.0, 16.0))


class PlacedShim(LitShim):
    """LitShim's entries plus mlp_render: the frame with the models' light tables."""

    def __init__(self, out):
        subprocess.run(["g++", *FLAGS, "-shared", "-o", os.fspath(out), os.fspath(SRC / "model_lights_paths_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")],
                       check=True)
        L = C.CDLL(os.fspath(out))
        L.is_model.restype = C.c_void_p
        L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
        L.is_free.argtypes = [C.c_void_p]
        L.ss_set_scale.restype = C.c_int
        L.ss_set_scale.argtypes = [C.c_void_p, C.c_uint32]
        lead = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + \
               [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float]
        L.lp_render.argtypes = lead + [C.c_void_p] * 5
        L.mlp_render.argtypes = lead + [C.c_void_p, C.c_void_p] + [C.c_void_p] * 5 + [C.c_void_p, C.c_void_p]
        self.lib = L

    def tree(self, xyz, ids, scale_log2=0):
        h = super().tree(xyz, ids)
        assert self.lib.ss_set_scale(h, scale_log2) == 0
        return h

    def render_placed(self, world, models, inst, cam, mats, w, h, spp, bounces, frame, table=None, model_tables=None, vs=1.0):
        """The planes dict plus "ids", "header" and "icum"; table: the world's LIGHT records (None: none); model_tables: per model its LIGHT
        records or None."""
        planes = {k: np.zeros((h, w, 4), dtype=f32) for k in PLANES}
        ids = np.zeros((h, w), dtype=np.uint32)
        handles = (C.c_void_p * max(1, len(models)))(*[m.value for m in models])
        inst = np.ascontiguousarray(inst if inst is not None else [], dtype=INSTANCE).reshape(-1)
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
        model_tables = [None] * len(models) if model_tables is None else [None if t is None else np.ascontiguousarray(t, dtype=LIGHT) for t in model_tables]
        ptrs = (C.c_void_p * max(1, len(models)))(*[(t.ctypes.data if t is not None and len(t) else None) for t in model_tables])
        counts = np.array([0 if t is None else len(t) for t in model_tables] + [0], dtype=np.uint32)
        header = np.zeros(1, dtype=INSTANCE_LIGHTS_INFO)
        icum = np.zeros(len(inst) + 1, dtype=np.uint32)
        self.lib.mlp_render(world, handles, len(models), _ptr(inst), len(inst), None, 0, vs, _ptr(cam), _ptr(mats), len(mats), w, h, spp, bounces, frame,
                            _ptr(table) if n else None, n, _ptr(owned) if n else None, faces, area, ptrs, _ptr(counts), *[_ptr(planes[k]) for k in PLANES], _ptr(ids),
                            _ptr(header), _ptr(icum))
        planes.update(ids=ids, header=header, icum=icum)
        return planes


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return PlacedShim(tmp_path_factory.mktemp("placed") / "libmodel_lights_paths_shim.so")


def world_scene(world_patch):
    """A 32^3 box: a floor two voxels thick and, with world_patch, a glowing 3 x 3 patch let into it; (density, ids, the world's table)."""
    d = np.zeros((32, 32, 32), dtype=f32)
    m = np.zeros((32, 32, 32), dtype=np.uint32)
    d[:, 0:2, :], m[:, 0:2, :] = 1.0, MC.GREY
    table = np.zeros(0, dtype=LIGHT)
    if world_patch:
        m[20:23, 1, 8:11] = MC.GLOW2
        table = np.zeros(1, dtype=LIGHT)
        table["lo"], table["du"], table["dv"], table["material"], table["face"] = (8, 2, 20), 3, 3, MC.GLOW2, 2
    return d, m, table


def lantern_instances():
    """Model 0 a 3^3 lantern, model 1 the same at exponent 1; three instances in different orientations over the floor."""
    return np.array([IO.instance(0, (8, 6, 12)), IO.instance(0, (20, 9, 18), (2, 0, 1), 5), IO.instance(1, (18, 4, 6), (1, 0, 2), 2)], dtype=INSTANCE)


def twin_table(world_table, inst, model_tables, exponents):
    """[the world's table ..., then instance_light_record of every face, instance by instance], cum run again."""
    parts = [world_table]
    for rec in inst:
        m = int(rec["model"])
        parts.append(np.array([LT.instance_light_record(rec, exponents[m], face) for face in model_tables[m]], dtype=LIGHT))
    table = np.concatenate(parts)
    area = table["du"].astype(np.int64) * table["dv"]
    table["cum"] = np.concatenate([[0], np.cumsum(area)[:-1]])
    return table


def setup(shim, world_patch):
    d, m, world_table = world_scene(world_patch)
    mats = MC.materials()
    cube = MC.cube(3)
    glow = np.full(27, MC.GLOW, dtype=np.uint32)
    models = [shim.tree(cube, glow), shim.tree(cube, glow, 1)]
    lantern = LT.host_model_lights(cube, glow, mats)
    assert len(lantern) == 54
    cam = W.camera_look_at(*CAM, 60.0, WD, HT)
    return shim.tree(*voxels_of(d, m)), models, lantern_instances(), cam, mats, world_table, lantern


def same_planes(a, b, what, keys=PLANES + ("ids",)):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float((a[k] != b[k]).mean()))


@pytest.mark.parametrize("world_patch", [True, False], ids=["a world table", "no world table"])
def test_tables_without_light_give_the_lit_bodys_bytes(shim, world_patch):
    """No model table at all; a table for a model that no instance uses (A_inst = 0); and the disabled case.  Each against the frame
    without model tables: the lit body's with a world table, the posed body's with A_world = 0 too."""
    world, models, inst, cam, mats, world_table, lantern = setup(shim, world_patch)
    other = shim.tree(MC.cube(2), np.full(8, MC.GLOW, dtype=np.uint32))
    huge = shim.tree(MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32), 8)
    store = models + [other, huge]
    want = shim.render(world, store, inst, None, cam, mats, WD, HT, 2, 3, 5, table=world_table)
    none = shim.render_placed(world, store, inst, cam, mats, WD, HT, 2, 3, 5, table=world_table)
    same_planes(none, want, "no model table")
    unused = shim.render_placed(world, store, inst, cam, mats, WD, HT, 2, 3, 5, table=world_table, model_tables=[None, None, LT.host_model_lights(MC.cube(2), np.full(8, MC.GLOW, dtype=np.uint32), mats), None])
    assert int(unused["header"]["a_inst"][0]) == 0 and int(unused["header"]["a_total"][0]) == (9 if world_patch else 0) and not unused["icum"].any()
    same_planes(unused, want, "a table that no instance uses")
    far = np.zeros(1214, dtype=INSTANCE)
    far["model"], far["axis"], far["offset"] = 3, (0, 1, 2), (-30000, -30000, -30000)
    crowd = np.concatenate([inst, far])
    want = shim.render(world, store, crowd, None, cam, mats, WD // 2, HT // 2, 1, 2, 5, table=world_table)
    disabled = shim.render_placed(world, store, crowd, cam, mats, WD // 2, HT // 2, 1, 2, 5, table=world_table, model_tables=[lantern, lantern, None, lantern])
    assert int(disabled["header"]["disabled"][0]) == 1 and int(disabled["header"]["a_total"][0]) == (9 if world_patch else 0) and not disabled["icum"].any()
    same_planes(disabled, want, "disabled")


@pytest.mark.parametrize("world_patch", [True, False], ids=["a world table", "no world table"])
def test_one_bounce_frame_equals_the_set_lights_twin(shim, world_patch):
    world, models, inst, cam, mats, world_table, lantern = setup(shim, world_patch)
    lit = shim.render_placed(world, models, inst, cam, mats, WD, HT, 2, 1, 3, table=world_table, model_tables=[lantern, lantern])
    assert lit["icum"].tolist() == [0, 54, 108, 108 + 54 * 4] and int(lit["header"]["a_total"][0]) == (9 if world_patch else 0) + 324
    twin = shim.render(world, models, inst, None, cam, mats, WD, HT, 2, 1, 3, table=twin_table(world_table, inst, [lantern, lantern], [0, 1]))
    same_planes(lit, twin, "the twin")
    unlit = shim.render(world, models, inst, None, cam, mats, WD, HT, 2, 1, 3, table=world_table)
    same_planes(lit, unlit, "the G-buffer", PLANES[1:] + ("ids",))
    floor = unlit["world_pos"][..., 1] == f32(2.0)
    assert floor.sum() > 100 and lit["color"][floor][:, :3].sum() > unlit["color"][floor][:, :3].sum()


def test_three_bounces_never_brighter_than_the_twin_and_darker_somewhere(shim):
    world, models, inst, cam, mats, world_table, lantern = setup(shim, True)
    lit = shim.render_placed(world, models, inst, cam, mats, WD, HT, 4, 3, 7, table=world_table, model_tables=[lantern, lantern])
    twin = shim.render(world, models, inst, None, cam, mats, WD, HT, 4, 3, 7, table=twin_table(world_table, inst, [lantern, lantern], [0, 1]))
    same_planes(lit, twin, "the G-buffer", PLANES[1:] + ("ids",))
    darker = (lit["color"][..., :3] < twin["color"][..., :3]).any(-1)
    print(f"darker in {int(darker.sum())} of {WD * HT} pixels")
    assert (lit["color"][..., :3] <= twin["color"][..., :3]).all() and darker.sum() > 5
