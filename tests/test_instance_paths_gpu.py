"""GPU: path-traced frames with instances (blok_hip_trace_paths_instanced*, blok_hip_draw_frame_rt_instanced).

References: the world-only entries (no instances: the same bits), the world-only frame of a "baked" world that holds the instances'
voxels (identity placements: the same bits), trace_primary_instanced (the first-hit G-buffer and ids) and the host build of the instance
BVH (tests/host_harness/tlas_shim.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import world as W
from blok_amd._ffi import INSTANCE, INSTANCE_NONE, BlokError
from tests import instance_oracle as IO
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PLANES = ("color", "world_pos", "normal_roughness", "albedo_metallic")
TLAS_MAX = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def plate(nx=16, ny=2, nz=16, material=3):
    xyz = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    return xyz, np.full(len(xyz), material, dtype=np.uint32)


def tracer(pw, w, h, models):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(w, h).init()
    tr.add_world(pw)
    assert [tr.model_create(xyz, mats) for xyz, mats in models] == list(range(len(models)))
    return tr


def world_voxels(inst, mx):
    """An instance's model voxels in world coordinates (the voxel map of instance_oracle.world_records)."""
    out = np.zeros_like(mx)
    flip = int(inst["flip"])
    for k in range(3):
        a = int(inst["axis"][k])
        o = int(inst["offset"][a])
        out[:, a] = (o - 1 - mx[:, k]) if (flip >> k) & 1 else (o + mx[:, k])
    return out


def baked_world(table, models):
    """The 64^3 scene plus every instance's voxels in world coordinates, through the world's own edit path."""
    cm = W.ChunkManager(128, 1.0)
    cm.generate_scene(64, SEED)
    xyz, mats = [], []
    for inst in table:
        mx, mm = models[int(inst["model"])]
        xyz.append(world_voxels(inst, mx))
        mats.append(mm)
    cm.set_voxels(np.concatenate(xyz), np.concatenate(mats))
    cm.rebuild_dirty_chunks()
    return cm.pack_chunks_to_gpu_svo(W.scene_materials(SEED))


def test_no_instances_is_the_world_only_frame(torch_cuda, scene64):
    cm, pw = scene64
    w, h = 160, 120
    tr = tracer(pw, w, h, [plate()])
    cam = W.scene_camera(64, 0, w, h, SEED)
    empty = np.zeros(0, dtype=INSTANCE)
    for spp, bounces in ((8, 2), (4, 3), (1, 1)):
        want = tr.trace_paths(cam, spp, bounces, frame_index=3)
        got = tr.trace_paths_instanced(cam, empty, spp, bounces, frame_index=3)
        for k in PLANES:
            assert got[k].tobytes() == want[k].tobytes(), (k, spp, bounces)
        assert (got["ids"] == INSTANCE_NONE).all()
    plain = [tr.draw_frame_rt(cam)[0] for _ in range(3)]
    tr.post_reset()
    inst = [tr.draw_frame_rt_instanced(cam, empty) for _ in range(3)]
    for a, (b, count) in zip(plain, inst):
        assert (a == b).all()
    assert inst[-1][1] == 3
    tr.shutdown()


def floating_table():
    # a plate high above the 64^3 terrain (its sun map's cap lies below it) and a small block beside it, both clear of the world
    return np.array([IO.instance(0, (36, 76, 36)), IO.instance(1, (12, 80, 44))], dtype=INSTANCE)


@pytest.mark.parametrize("spp,bounces", [(4, 2), (2, 3)])
def test_identity_placements_equal_the_baked_world(torch_cuda, scene64, spp, bounces):
    """Instances placed at their own lattice: the frame equals the world-only frame of a world that holds their voxels, bit for bit, in
    every float4 plane and every reference-format plane (motion included), and the floating plate casts its shadow."""
    torch = torch_cuda
    cm, pw = scene64
    models = [plate(), plate(3, 3, 3, 5)]
    table = floating_table()
    baked = baked_world(table, models)
    w, h = 160, 128
    cam = W.camera_look_at((30.0, 130.0, 10.0), (30.0, 10.0, 34.0), 70.0, w, h)
    tr = tracer(pw, w, h, models)
    tb = tracer(baked, w, h, [])
    for t in (tr, tb):
        t.set_ray_batching(2)
    got = tr.trace_paths_instanced(cam, table, spp, bounces, frame_index=2)
    want = tb.trace_paths(cam, spp, bounces, frame_index=2)
    for k in PLANES:
        diff = (got[k] != want[k]).any(axis=2)
        assert not diff.any(), (k, diff.mean(), np.argwhere(diff)[:6].tolist())
    won = got["ids"] != INSTANCE_NONE
    assert won.sum() > 100 and set(np.unique(got["ids"][won])) == {0, 1}
    # the shadow: pixels the world-only frame of the same world lights are darker with the plate above them
    bare = tr.trace_paths_instanced(cam, table[:0], spp, bounces, frame_index=2)
    lum = lambda c: c[..., :3].sum(-1)
    darker = (lum(got["color"]) < 0.7 * lum(bare["color"])) & ~won
    assert darker.sum() > 50, darker.sum()
    # reference-format planes
    n = w * h
    vp = tr.camera_view_proj(cam)
    outs = []
    for t, tab in ((tr, table), (tb, None)):
        bufs = dict(color=torch.zeros(n * 4, dtype=torch.float32, device="cuda"), world_pos=torch.zeros(n * 4, dtype=torch.float32, device="cuda"),
                    nr=torch.zeros(n * 4, dtype=torch.int16, device="cuda"), am=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    motion=torch.zeros(n * 2, dtype=torch.int16, device="cuda"))
        args = dict(color_ptr=bufs["color"].data_ptr(), world_pos_ptr=bufs["world_pos"].data_ptr(), normal_roughness_h_ptr=bufs["nr"].data_ptr(),
                    albedo_metallic_u8_ptr=bufs["am"].data_ptr(), motion_h_ptr=bufs["motion"].data_ptr(), prev_view_proj=vp, spp=spp,
                    max_bounces=bounces, frame_index=2)
        if tab is None:
            t.trace_paths_ref_device(cam, **args)
        else:
            dev = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
            ids = torch.zeros(n, dtype=torch.int32, device="cuda")
            t.trace_paths_instanced_ref_device(cam, dev.data_ptr(), len(tab), ids_ptr=ids.data_ptr(), **args)
            torch.cuda.synchronize()
            assert (ids.cpu().numpy().view(np.uint32).reshape(h, w) == got["ids"]).all()
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in bufs.items()})
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    tr.shutdown()
    tb.shutdown()


def check_first_hit(tr, cam, table, spp=1, bounces=1):
    got = tr.trace_paths_instanced(cam, table, spp, bounces, frame_index=0)
    hits, ids, _ = tr.trace_primary_instanced(cam, table)
    assert (got["ids"] == ids).all(), np.argwhere(got["ids"] != ids)[:6].tolist()
    hit = hits["hit"] == 1
    t = got["world_pos"][..., 3]
    assert (t[hit] == hits["t"][hit]).all()
    assert (t[~hit] == 10000.0).all()
    # the face's normal, signed (face 2k: +axis k, 2k + 1: -axis k), turned against the ray where it points along it (hit.rchit; a ray
    # that starts inside a model's voxel)
    from tests import oracle_ffi as O
    face = hits["face"].astype(np.int64)
    normal = np.zeros(hits.shape + (3,), dtype=np.float32)
    for f in range(6):
        normal[face == f, f // 2] = 1.0 if f % 2 == 0 else -1.0
    d = O.primary_rays(cam, tr.width, tr.height)["dir"].reshape(hits.shape + (3,))
    normal = np.where(((normal * d).sum(-1) > 0)[..., None], -normal, normal)
    nr = got["normal_roughness"][..., :3]
    assert (nr[hit] == normal[hit]).all(), np.argwhere((nr != normal).any(-1) & hit)[:6].tolist()
    # albedo and metallic from the material (the emission for an emissive one), as hit.rchit forms them
    mats = W.scene_materials(SEED)
    m = mats[np.minimum(np.minimum(hits["material_id"], 65535), len(mats) - 1)]
    emissive = m["emission"].sum(-1) > np.float32(0.01)
    albedo = np.where(emissive[..., None], m["emission"], m["albedo"]).astype(np.float32)
    metallic = ((m["flags"] >> 24) & 0xFF).astype(np.float32) / np.float32(255.0)
    am = got["albedo_metallic"]
    assert (am[hit][:, :3] == albedo[hit]).all() and (am[hit][:, 3] == metallic[hit]).all()
    return got, ids


def test_random_placements_first_hit_equals_trace_primary_instanced(torch_cuda, scene64):
    cm, pw = scene64
    models = IO.procedural_models()
    w, h = 192, 144
    tr = tracer(pw, w, h, models)
    cam = W.scene_camera(64, 0, w, h, SEED)
    table = IO.random_instances(64, len(models), -6, 66, seed=64)
    table[:48]["axis"] = [p for p, f in IO.SIGNED_PERMUTATIONS]
    table[:48]["flip"] = [f for p, f in IO.SIGNED_PERMUTATIONS]
    got, ids = check_first_hit(tr, cam, table, spp=4, bounces=2)
    assert (ids != INSTANCE_NONE).sum() > 500 and len(np.unique(ids[ids != INSTANCE_NONE])) > 10
    tr.shutdown()


def oriented_table():
    """48 instances, one per orientation, in a grid high above the 64^3 terrain.  Every model used fits in 13 voxels a side, so a box lies
    within 13 voxels of its offset whatever the orientation: 27 voxels apart, no two boxes touch and the baked world's voxels are exactly
    the instances'."""
    table = np.zeros(48, dtype=INSTANCE)
    for i, (p, f) in enumerate(IO.SIGNED_PERMUTATIONS):
        table[i] = IO.instance((0, 1, 3)[i % 3], (27 * (i % 8) - 80, 92, 27 * (i // 8) - 50), p, f)
    return table


def within_tolerance(got, ref):
    return np.abs(got - ref) <= 1e-4 + 1e-3 * np.abs(ref)


def test_all_orientations_colour_equals_the_baked_world_oracle(torch_cuda, scene64):
    """Instances in all 48 orientations over the terrain: the G-buffer equals the oracle's on the baked world exactly, the colour is
    within tests/test_paths.py's tolerance on >= 99.5 % of pixels with a mean error < 2e-4 (bounce origins round differently in local
    space, so a rare sample may take another path)."""
    from tests import oracle_ffi as O
    cm, pw = scene64
    models = IO.procedural_models()
    table = oriented_table()
    baked = baked_world(table, models)
    w, h = 192, 144
    cam = W.camera_look_at((14.0, 200.0, 17.0), (14.0, 0.0, 19.0), 90.0, w, h)
    tr = tracer(pw, w, h, models)
    got = tr.trace_paths_instanced(cam, table, 4, 2, frame_index=5)
    mats = W.scene_materials(SEED)
    ref, _ = O.render_paths(O.Lattice(baked.nodes, baked.sub_chunks), mats, cam, w, h, spp=4, max_bounces=2, frame_index=5, threads=16)
    for k in ("world_pos", "normal_roughness", "albedo_metallic"):
        diff = (got[k] != ref[k]).any(axis=2)
        assert not diff.any(), (k, diff.mean(), np.argwhere(diff)[:6].tolist())
    won = got["ids"] != INSTANCE_NONE
    assert won.mean() > 0.015 and len(np.unique(got["ids"][won])) > 30
    ok = within_tolerance(got["color"], ref["color"]).all(axis=2)
    assert ok.mean() >= 0.995, (ok.mean(), np.argwhere(~ok)[:8].tolist())
    assert np.abs(got["color"] - ref["color"]).mean() < 2e-4
    tr.shutdown()


@pytest.mark.parametrize("n", [1024, TLAS_MAX + 1])
def test_tlas_at_scale(torch_cuda, scene64, n):
    cm, pw = scene64
    models = IO.procedural_models()
    w, h = 160, 120
    tr = tracer(pw, w, h, models)
    cam = W.scene_camera(64, 1, w, h, SEED)
    table = IO.random_instances(n, len(models), -8, 70, seed=n)
    table[n // 2: n // 2 + 64] = table[:64]                         # duplicates: ties between instances
    _, ids = check_first_hit(tr, cam, table)
    assert (ids != INSTANCE_NONE).sum() > 1000
    tr.shutdown()


def test_device_tlas_equals_the_host_build(torch_cuda, scene64, tmp_path):
    torch = torch_cuda
    cm, pw = scene64
    models = IO.procedural_models()
    tr = tracer(pw, 64, 64, models)
    out = tmp_path / "libtlas_shim.so"
    src = ROOT / "tests" / "host_harness"
    subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-ffp-contract=off", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}",
                    f"-I{src}", "-shared", "-o", os.fspath(out), os.fspath(src / "tlas_shim.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    L.is_model.restype = C.c_void_p
    L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.is_free.argtypes = [C.c_void_p]
    L.ts_node_count.restype = C.c_uint32
    L.ts_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p]
    handles = []
    for xyz, mats in models:
        why = C.c_char_p()
        handles.append(L.is_model(C.c_void_p(xyz.ctypes.data), C.c_void_p(mats.ctypes.data), len(mats), C.byref(why)))
    arr = (C.c_void_p * len(handles))(*handles)
    for n in (1, 5, 300, TLAS_MAX):
        table = IO.random_instances(n, len(models) + 1, -8, 70, seed=n)    # model ids up to len(models): unknown ones are left out
        if n > 4:
            table[3] = table[1]
        host = np.zeros((L.ts_node_count(n), 8), dtype=np.int32)
        L.ts_build(arr, len(handles), C.c_void_p(table.ctypes.data), n, C.c_void_p(host.ctypes.data))
        dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        got = tr.debug_build_tlas(dev.data_ptr(), n)
        assert got.tobytes() == host.tobytes(), n
    for h in handles:
        L.is_free(h)
    tr.shutdown()


def test_sky_tiles_show_instances(torch_cuda, scene64):
    """Every ray of this camera leaves the 64^3 world upwards (the beam pre-pass reports no voxel for any tile); the plate above still
    shows in the G-buffer and the id plane."""
    cm, pw = scene64
    w, h = 128, 96
    tr = tracer(pw, w, h, [plate()])
    cam = W.camera_look_at((40.0, 100.0, 40.0), (44.0, 200.0, 44.0), 60.0, w, h)
    table = np.array([IO.instance(0, (36, 130, 36))], dtype=INSTANCE)
    bare = tr.trace_paths(cam, 2, 2)
    assert (bare["world_pos"][..., 3] == 10000.0).all()
    got, ids = check_first_hit(tr, cam, table, spp=2, bounces=2)
    assert (ids == 0).sum() > 500
    tr.shutdown()


def test_table_changes_in_stream_order_and_two_streams(torch_cuda, scene64):
    torch = torch_cuda
    cm, pw = scene64
    models = IO.procedural_models()
    w, h = 96, 64
    tr = tracer(pw, w, h, models)
    cam = W.scene_camera(64, 0, w, h, SEED)
    a = IO.random_instances(40, len(models), -6, 66, seed=1)
    b = IO.random_instances(40, len(models), -6, 66, seed=2)
    solo = {k: tr.trace_paths_instanced(cam, t, 2, 2, frame_index=1) for k, t in (("a", a), ("b", b))}
    n = w * h

    def launch(table_dev, count, stream=0):
        color = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
        ids = torch.zeros(n, dtype=torch.int32, device="cuda")
        tr.trace_paths_instanced_device(cam, table_dev.data_ptr(), count, color_ptr=color.data_ptr(), ids_ptr=ids.data_ptr(), spp=2,
                                        max_bounces=2, frame_index=1, stream=stream)
        return color, ids

    def check(color, ids, key):
        assert (color.cpu().numpy().reshape(h, w, 4) == solo[key]["color"]).all(), key
        assert (ids.cpu().numpy().view(np.uint32).reshape(h, w) == solo[key]["ids"]).all(), key

    table = torch.from_numpy(a.view(np.uint8).copy()).cuda()
    first = launch(table, len(a))
    table.copy_(torch.from_numpy(b.view(np.uint8).copy()))          # the next frame's table, in stream order, no synchronise
    second = launch(table, len(b))
    torch.cuda.synchronize()
    check(*first, "a")
    check(*second, "b")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ta = torch.from_numpy(a.view(np.uint8).copy()).cuda()
    tb = torch.from_numpy(b.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ra = launch(ta, len(a), s1.cuda_stream)
    with torch.cuda.stream(s2):
        rb = launch(tb, len(b), s2.cuda_stream)
    torch.cuda.synchronize()
    check(*ra, "a")
    check(*rb, "b")
    tr.shutdown()


def test_errors_and_skipped_instances(torch_cuda, scene64):
    torch = torch_cuda
    cm, pw = scene64
    models = IO.procedural_models()
    w, h = 64, 48
    tr = tracer(pw, w, h, models)
    cam = W.scene_camera(64, 0, w, h, SEED)
    bad = IO.random_instances(4, len(models), 0, 40, seed=9)
    bad[2]["flip"] = 8
    with pytest.raises(BlokError) as e:
        tr.trace_paths_instanced(cam, bad, 1, 1)
    assert e.value.status == -1 and "flip" in str(e.value)
    with pytest.raises(BlokError):
        tr.draw_frame_rt_instanced(cam, bad)
    # a motion plane without prevViewProj; no planes at all
    motion = torch.zeros(w * h * 2, dtype=torch.int16, device="cuda")
    with pytest.raises(BlokError):
        tr.trace_paths_instanced_ref_device(cam, 0, 0, motion_h_ptr=motion.data_ptr())
    rc = tr._lib.blok_hip_trace_paths_instanced_device(tr._ctx, C.c_void_p(cam.ctypes.data), 0, 0, w, h, 1, 1, 0, None, 0, None, None, None)
    assert rc != 0
    # device entry: an instance of a destroyed model is skipped
    table = IO.random_instances(30, len(models), -6, 60, seed=4)
    keep = table[table["model"] != 2]
    want = tr.trace_paths_instanced(cam, keep, 2, 2)
    tr.model_destroy(2)
    dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    color = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
    tr.trace_paths_instanced_device(cam, dev.data_ptr(), len(table), color_ptr=color.data_ptr(), spp=2, max_bounces=2)
    torch.cuda.synchronize()
    assert (color.cpu().numpy().reshape(h, w, 4) == want["color"]).all()
    tr.shutdown()
