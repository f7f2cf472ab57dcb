"""GPU: posed models in the path-traced frame (include/blok_hip.h, "Path-traced frames with poses": blok_hip_trace_paths_posed*,
blok_hip_draw_frame_rt_posed) over the world and the case table of tests/pose_cases.py.

References, all exact: the instanced entries (no poses; the same placements as lattice instances), trace_primary_posed (the first hit),
a numpy float32 restatement of the normal rule, and trace_rays_posed for the shadow rays formed from the frame's own planes."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import pose as P
from blok_amd._ffi import GBuffer, INSTANCE, INSTANCE_NONE, POSE, POSE_ID, BlokError
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests import pose_cases as PC
from tests import pose_oracle as PO

pytestmark = pytest.mark.gpu

f32 = np.float32
VOXEL_SIZES = [1.0, 0.5]
PLANES = ("color", "world_pos", "normal_roughness", "albedo_metallic")
BLOK_ERR_INVALID_ARG = -1
N_CASES = len(PC.table(1.0))
TLAS_MAX = 4096
AXIS_NORMALS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=f32) + f32(0.0)
SUN = np.array([0.5, 0.8, 0.3], dtype=f32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def make_tracer(vs, w=PC.WD, h=PC.HT):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(w, h).init()
    if vs != 1.0:
        tr.set_voxel_size(vs)
    tr.add_world(PC.world(vs))
    for (xyz, mats), e in zip(PC.models(), PC.EXPONENTS):
        tr.model_set_scale(tr.model_create(xyz, mats), e)
    return tr


@pytest.fixture(scope="module")
def tracers(torch_cuda):
    out = {vs: make_tracer(vs) for vs in VOXEL_SIZES}
    yield out
    for tr in out.values():
        tr.shutdown()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() if len(a) else torch.zeros(1, dtype=torch.uint8, device="cuda")


def is_pose(ids):
    return (ids != INSTANCE_NONE) & ((ids & POSE_ID) != 0)


def same_planes(a, b, what, keys=PLANES):
    for k in keys:
        diff = (a[k] != b[k]).any(axis=2)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float(diff.mean()), np.argwhere(diff)[:6].tolist())


def ref_planes(torch, n):
    return dict(color=torch.zeros(n * 4, dtype=torch.float32, device="cuda"), world_pos=torch.zeros(n * 4, dtype=torch.float32, device="cuda"),
                nr=torch.zeros(n * 4, dtype=torch.int16, device="cuda"), am=torch.zeros(n, dtype=torch.int32, device="cuda"),
                motion=torch.zeros(n * 2, dtype=torch.int16, device="cuda"), ids=torch.zeros(n, dtype=torch.int32, device="cuda"))


def ref_args(bufs, vp, spp, bounces, frame_index):
    return dict(color_ptr=bufs["color"].data_ptr(), world_pos_ptr=bufs["world_pos"].data_ptr(), normal_roughness_h_ptr=bufs["nr"].data_ptr(),
                albedo_metallic_u8_ptr=bufs["am"].data_ptr(), motion_h_ptr=bufs["motion"].data_ptr(), prev_view_proj=vp, ids_ptr=bufs["ids"].data_ptr(),
                spp=spp, max_bounces=bounces, frame_index=frame_index)


# ---- 1. no poses: the instanced entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp,bounces", [(4, 2), (1, 1)])
def test_no_poses_gives_the_bytes_of_the_instanced_entries(torch_cuda, tracers, spp, bounces):
    torch = torch_cuda
    tr = tracers[1.0]
    case = PC.table(1.0)[11]                                   # the mixed case's instances
    cam = case.camera(PC.WD, PC.HT)
    n = PC.WD * PC.HT
    vp = tr.camera_view_proj(cam)
    for inst in (case.instances, case.instances[:0]):
        want = tr.trace_paths_instanced(cam, inst, spp, bounces, frame_index=3)
        got = tr.trace_paths_posed(cam, inst, None, spp, bounces, frame_index=3)
        same_planes(got, want, "host entry")
        assert got["ids"].tobytes() == want["ids"].tobytes()
        d_inst = dev(torch, inst)
        # the float4 device entry
        outs = []
        for posed in (False, True):
            b = {k: torch.zeros(n * 4, dtype=torch.float32, device="cuda") for k in PLANES}
            ids = torch.zeros(n, dtype=torch.int32, device="cuda")
            args = dict(color_ptr=b["color"].data_ptr(), world_pos_ptr=b["world_pos"].data_ptr(), normal_roughness_ptr=b["normal_roughness"].data_ptr(),
                        albedo_metallic_ptr=b["albedo_metallic"].data_ptr(), ids_ptr=ids.data_ptr(), spp=spp, max_bounces=bounces, frame_index=3)
            if posed:
                tr.trace_paths_posed_device(cam, d_inst.data_ptr(), len(inst), 0, 0, **args)
            else:
                tr.trace_paths_instanced_device(cam, d_inst.data_ptr(), len(inst), **args)
            torch.cuda.synchronize()
            outs.append([b[k].cpu().numpy().tobytes() for k in PLANES] + [ids.cpu().numpy().tobytes()])
        assert outs[0] == outs[1]
        assert outs[1][0] == want["color"].tobytes() and outs[1][4] == want["ids"].tobytes()
        # the reference-format device entry
        outs = []
        for posed in (False, True):
            b = ref_planes(torch, n)
            if posed:
                tr.trace_paths_posed_ref_device(cam, d_inst.data_ptr(), len(inst), 0, 0, **ref_args(b, vp, spp, bounces, 3))
            else:
                tr.trace_paths_instanced_ref_device(cam, d_inst.data_ptr(), len(inst), **ref_args(b, vp, spp, bounces, 3))
            torch.cuda.synchronize()
            outs.append({k: v.cpu().numpy().tobytes() for k, v in b.items()})
        assert outs[0] == outs[1]
    assert (want["ids"] == INSTANCE_NONE).all() and (tr.trace_paths_instanced(cam, case.instances, 1, 1)["ids"] == 0).any()
    # the chain: three frames
    tr.post_reset()
    a = [tr.draw_frame_rt_instanced(cam, case.instances, spp, bounces) for _ in range(3)]
    tr.post_reset()
    b = [tr.draw_frame_rt_posed(cam, case.instances, None, spp, bounces) for _ in range(3)]
    tr.post_reset()
    for (x, nx), (y, ny) in zip(a, b):
        assert x.tobytes() == y.tobytes() and nx == ny
    assert b[-1][1] == 3


# ---- 2. lattice poses: the same placements as instances -------------------------------------------------------------------------------------------
def oriented_placements(vs):
    """The 48 orientations, one placement each, over the small world; the models of the case table (one at scale exponent 2) and a sixth,
    the ball at model_set_scale 1."""
    rng = np.random.default_rng(9)
    return np.array([IO.instance((0, 1, 2, 3, 4, 5)[i % 6], rng.integers(-30, 50, size=3) + (0, 25, 0), p, f) for i, (p, f) in enumerate(IO.SIGNED_PERMUTATIONS)],
                    dtype=INSTANCE)


@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_poses_from_instances_equal_the_instanced_frame_in_every_plane(torch_cuda, vs):
    """Shadows, bounces, the use of random numbers and the chain, pinned exactly: a pose made by blok_pose_from_instance walks the lattice
    instance's ray, and its normal by the rule is the instance's axis normal bit for bit."""
    torch = torch_cuda
    tr = make_tracer(vs)
    xyz, mats = PC.models()[PC.BALL]
    tr.model_set_scale(tr.model_create(xyz, mats), 1)
    table = oriented_placements(vs)
    poses = np.concatenate([P.from_instance(inst, vs) for inst in table])
    tr.check_instances(table)
    tr.check_poses(poses)
    cam = PC.W.camera_look_at((90.0 * vs, 90.0 * vs, -70.0 * vs), (10.0 * vs, 25.0 * vs, 10.0 * vs), 60.0, PC.WD, PC.HT)
    n = PC.WD * PC.HT
    vp = tr.camera_view_proj(cam)
    d_inst, d_pose = dev(torch, table), dev(torch, poses)
    for spp, bounces in ((4, 2), (2, 3)):
        want = tr.trace_paths_instanced(cam, table, spp, bounces, frame_index=2)
        got = tr.trace_paths_posed(cam, None, poses, spp, bounces, frame_index=2)
        same_planes(got, want, f"vs {vs} ({spp}, {bounces})")
        won = want["ids"] != INSTANCE_NONE
        assert won.sum() > 500 and len(np.unique(want["ids"][won])) > 20
        assert ((got["ids"] == INSTANCE_NONE) == ~won).all() and (got["ids"][won] == (POSE_ID | want["ids"][won])).all()
        outs = []
        for posed in (False, True):
            b = ref_planes(torch, n)
            if posed:
                tr.trace_paths_posed_ref_device(cam, 0, 0, d_pose.data_ptr(), len(poses), **ref_args(b, vp, spp, bounces, 2))
            else:
                tr.trace_paths_instanced_ref_device(cam, d_inst.data_ptr(), len(table), **ref_args(b, vp, spp, bounces, 2))
            torch.cuda.synchronize()
            outs.append({k: v.cpu().numpy() for k, v in b.items()})
        for k in ("color", "world_pos", "nr", "am", "motion"):
            assert outs[0][k].tobytes() == outs[1][k].tobytes(), (k, spp, bounces)
        assert (outs[1]["ids"].view(np.uint32).reshape(PC.HT, PC.WD) == got["ids"]).all()
        assert outs[1]["color"].tobytes() == got["color"].tobytes()
    # half as instances, half as poses: still the same frame
    mixed = tr.trace_paths_posed(cam, table[:24], poses[24:], 4, 2, frame_index=2)
    same_planes(mixed, tr.trace_paths_instanced(cam, np.concatenate([table[:24], table[24:]]), 4, 2, frame_index=2), "mixed tables")
    tr.post_reset()
    a = [tr.draw_frame_rt_instanced(cam, table, 2, 2) for _ in range(3)]
    tr.post_reset()
    b = [tr.draw_frame_rt_posed(cam, None, poses, 2, 2) for _ in range(3)]
    for (x, nx), (y, ny) in zip(a, b):
        assert x.tobytes() == y.tobytes() and nx == ny
    tr.shutdown()


# ---- 3. the first hit under general poses ------------------------------------------------------------------------------------------------------------
def normal_rule(p, face):
    """include/blok_hip.h, "The normal of a posed hit", in numpy float32 (every operation rounds once)."""
    k, n = face >> 1, face & 1
    v = (f32(-1.0) if n else f32(1.0)) * np.asarray(p["m"], dtype=f32)[k]
    with np.errstate(all="ignore"):
        q = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if not q > 0:
            return AXIS_NORMALS[PO.shade_face(p, face)]
        return v / np.sqrt(q) + f32(0.0)


def expected_normals(hits, ids, poses, dirs):
    """The normal plane of the first hits: the axis normal of a world or instance record's face, the rule's normal of a pose's local face,
    turned against the primary ray where (n.x d.x + n.y d.y) + n.z d.z > 0 in float32."""
    face = hits["face"].astype(np.int64)
    normal = AXIS_NORMALS[np.minimum(face, 5)].copy()
    posed = is_pose(ids) & (hits["hit"] == 1)
    for j in np.unique(ids[posed] & 0x7FFFFFFF):
        for f in range(6):
            sel = posed & ((ids & 0x7FFFFFFF) == j) & (face == f)
            if sel.any():
                normal[sel] = normal_rule(poses[int(j)], f)
    d = dirs.astype(f32)
    dot = (normal[..., 0] * d[..., 0] + normal[..., 1] * d[..., 1]) + normal[..., 2] * d[..., 2]
    assert dot.dtype == f32
    return np.where((dot > 0)[..., None], -normal, normal)


def check_first_hit(tr, case, vs, spp=1, bounces=1):
    cam = case.camera(tr.width, tr.height)
    got = tr.trace_paths_posed(cam, case.instances, case.poses, spp, bounces, frame_index=0)
    hits, ids, _ = tr.trace_primary_posed(cam, case.instances, case.poses)
    assert (got["ids"] == ids).all(), np.argwhere(got["ids"] != ids)[:6].tolist()
    hit = hits["hit"] == 1
    t = got["world_pos"][..., 3]
    assert (t[hit] == hits["t"][hit]).all() and (t[~hit] == 10000.0).all()
    dirs = O.primary_rays(cam, tr.width, tr.height)["dir"].reshape(hits.shape + (3,))
    want = expected_normals(hits, ids, case.poses, dirs)
    nr = got["normal_roughness"][..., :3]
    bad = (nr.view(np.uint32) != want.view(np.uint32)).any(-1) & hit
    assert not bad.any(), (case.name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), nr[bad][:2], want[bad][:2])
    mats = PC.world(vs).materials
    m = mats[np.minimum(np.minimum(hits["material_id"], 65535), len(mats) - 1)]
    emissive = m["emission"].sum(-1) > f32(0.01)
    albedo = np.where(emissive[..., None], m["emission"], m["albedo"]).astype(f32)
    metallic = ((m["flags"] >> 24) & 0xFF).astype(f32) / f32(255.0)
    am = got["albedo_metallic"]
    assert (am[hit][:, :3] == albedo[hit]).all() and (am[hit][:, 3] == metallic[hit]).all()
    return got, hits, ids


@pytest.mark.parametrize("vs", VOXEL_SIZES)
@pytest.mark.parametrize("n", range(N_CASES))
def test_first_hit_equals_trace_primary_posed_with_true_normals(torch_cuda, tracers, n, vs):
    case = PC.table(vs)[n]
    got, hits, ids = check_first_hit(tracers[vs], case, vs, spp=2 if n % 2 else 1, bounces=1 + n % 3)
    if n < 9:
        assert is_pose(ids).mean() >= 0.05, (case.name, is_pose(ids).mean())
    if n in (0, 1, 5):                                          # a turned pose shows normals that are no axis
        nr = got["normal_roughness"][..., :3][is_pose(ids)]
        assert (np.count_nonzero(nr, axis=1) > 1).mean() > 0.5
    assert np.isfinite(got["color"]).all()


# ---- 4. the pose tree is an optimisation -----------------------------------------------------------------------------------------------------
def mixed_table(vs):
    t = PC.table(vs)
    inst = t[11].instances                                          # two lattice instances
    poses = np.concatenate([t[0].poses, t[2].poses, t[5].poses, t[12].poses])      # yaw 30, scale 0.5, the shear, the 70 rods
    return inst, poses, t[6].poses                                  # ... and the rank-2 pose


def test_frames_with_and_without_the_pose_tree_are_identical(torch_cuda, tracers, tmp_path):
    from tests import test_posed_paths_cpu as CPU
    torch = torch_cuda
    vs = 1.0
    tr = tracers[vs]
    inst, poses, flat = mixed_table(vs)
    case = PC.table(vs)[12]                                          # the rods' view
    views = [case.camera(PC.WD, PC.HT), PC.table(vs)[0].camera(PC.WD, PC.HT)]
    shim = CPU.Shim(CPU.build_shim(tmp_path / "libpose_tlas_shim.so"))
    seen_poses = seen_instances = 0
    for table in (poses, np.concatenate([poses[:2], flat, poses[2:]])):
        for cam in views:
            frames = []
            for enabled in (0, 1):
                tr.set_pose_tlas(enabled)
                frames.append(tr.trace_paths_posed(cam, inst, table, 4, 2, frame_index=9))
            tr.set_pose_tlas(1)
            same_planes(frames[0], frames[1], f"{len(table)} poses", PLANES)
            assert frames[0]["ids"].tobytes() == frames[1]["ids"].tobytes()
            seen_poses += int(is_pose(frames[1]["ids"]).sum())
            seen_instances += int((~is_pose(frames[1]["ids"]) & (frames[1]["ids"] != INSTANCE_NONE)).sum())
        # the device tree is the host build, byte for byte
        cam = views[0]
        d_table = dev(torch, table)
        got = tr.debug_build_pose_tlas(cam, d_table.data_ptr(), len(table))
        want = CPU.build_tree(shim, table, vs, np.asarray(cam[0]["pos"], dtype=f32))
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
        assert got[0][0] == (1 if len(table) > len(poses) else 0)    # the header's linear flag with the rank-2 pose
    assert seen_poses > 400 and seen_instances > 40


# ---- 5. shadows under a turned pose --------------------------------------------------------------------------------------------------------------
def shadow_rays(planes):
    """The shadow ray of every pixel from the frame's own planes, as the path loop forms it (path_core.h: so = hit_pos + n * 0.001, the
    kernel's sun direction, [0.001, 1000)), in numpy float32."""
    pos = planes["world_pos"][..., :3].astype(f32)
    n = planes["normal_roughness"][..., :3].astype(f32)
    sun = SUN / np.sqrt((SUN[0] * SUN[0] + SUN[1] * SUN[1]) + SUN[2] * SUN[2])
    rays = np.zeros(pos.shape[:2], dtype=O.RAY)
    rays["org"] = pos + n * f32(0.001)
    rays["dir"] = sun
    rays["tmin"] = 0.001
    rays["tmax"] = 1000.0
    n_dot_l = (n[..., 0] * sun[0] + n[..., 1] * sun[1]) + n[..., 2] * sun[2]
    return rays.reshape(-1), n_dot_l


def plate_model():
    xyz = np.stack(np.meshgrid(np.arange(24), np.arange(2), np.arange(24), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    return xyz, np.full(len(xyz), 7, dtype=np.uint32)


@pytest.mark.parametrize("sun_map", [True, False])
def test_shadows_under_and_on_a_turned_plate(torch_cuda, sun_map):
    """A plate turned by 30 degrees about y and 20 about x floats above the world's ground plate, one sample, one bounce: a pixel's colour is
    the sun's term or nothing.  On non-emissive first hits that face the sun, RGB is exactly 0 where the pixel's own shadow ray (formed here
    from the frame's planes) reports a voxel through trace_rays_posed, and > 0 where it does not: the two sets are equal."""
    vs = 1.0
    tr = make_tracer(vs)
    model = tr.model_create(*plate_model())
    tr.set_sun_map(sun_map)
    pos = (10.0, 16.0, 10.0)
    pose = P.rotation(model, np.radians(30.0), np.radians(20.0), 0.0, 1.0, (12.0, 1.0, 12.0), pos)
    cam = PC.W.camera_look_at((10.0, 48.0, -22.0), (10.0, 6.0, 12.0), 60.0, PC.WD, PC.HT)
    got = tr.trace_paths_posed(cam, None, pose, 1, 1, frame_index=0)
    rays, n_dot_l = shadow_rays(got)
    hits, _ = tr.trace_rays_posed(rays, None, pose)
    world_only, _ = tr.trace_rays_instanced(rays, np.zeros(0, dtype=INSTANCE))
    occluded = (hits["hit"] == 1).reshape(PC.HT, PC.WD)
    by_world = (world_only["hit"] == 1).reshape(PC.HT, PC.WD)
    mats = PC.world(vs).materials
    first, ids, _ = tr.trace_primary_posed(cam, None, pose)
    m = mats[np.minimum(first["material_id"], len(mats) - 1)]
    plain = (first["hit"] == 1) & ~(m["emission"].sum(-1) > f32(0.01)) & (m["albedo"].max(-1) > 0) & (n_dot_l > 0)
    dark = (got["color"][..., :3] == 0).all(-1)
    lit = (got["color"][..., :3] > 0).any(-1)
    assert (dark[plain] == occluded[plain]).all(), np.argwhere(plain & (dark != occluded))[:8].tolist()
    assert (lit[plain] == ~occluded[plain]).all()
    assert (plain & occluded & ~by_world & ~is_pose(ids)).sum() >= 50, "pixels occluded by the pose alone"
    assert (plain & is_pose(ids)).sum() >= 50, "pose pixels that face the sun"
    tr.shutdown()


# ---- 6. bounce rays see poses ----------------------------------------------------------------------------------------------------------------
def test_bounce_rays_see_an_emissive_turned_cube(torch_cuda):
    """A small turned cube of an emissive material (a material table of the test's own) hangs in front of a world wall, four samples, two
    bounces, one frame index.  World pixels whose first hit and whose shadow answer the cube leaves unchanged differ, with and without it,
    only in what their bounce rays report: on at least 30 of them the cube's light makes the colour brighter."""
    from blok_amd.tracer import HipTracer
    glow = 200
    mats = PC.W.scene_materials(PC.SEED).copy()
    mats["emission"][glow] = (20.0, 18.0, 12.0)
    xyz, ids = PC.world_voxels()
    wall = np.array([(24, y, z) for y in range(1, 24) for z in range(-6, 28)], dtype=np.int32)
    cm = PC.W.ChunkManager(128, 1.0)
    cm.set_voxels(np.concatenate([xyz, wall]), np.concatenate([ids, np.full(len(wall), 9, dtype=np.uint32)]))
    cm.rebuild_dirty_chunks()
    tr = HipTracer(PC.WD, PC.HT).init()
    tr.add_world(cm.pack_chunks_to_gpu_svo(mats))
    cube = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    model = tr.model_create(cube, np.full(len(cube), glow, dtype=np.uint32))
    pose = P.rotation(model, np.radians(30.0), np.radians(20.0), 0.0, 1.0, (3.0, 3.0, 3.0), (17.0, 11.0, 11.0))
    cam = PC.W.camera_look_at((-8.0, 14.0, 11.0), (24.0, 10.0, 11.0), 60.0, PC.WD, PC.HT)
    none = np.zeros(0, dtype=POSE)
    with_cube = tr.trace_paths_posed(cam, None, pose, 4, 2, frame_index=7)
    without = tr.trace_paths_posed(cam, None, none, 4, 2, frame_index=7)
    same_first = ~is_pose(with_cube["ids"]) & (with_cube["world_pos"] == without["world_pos"]).all(-1) & (without["world_pos"][..., 3] < 9999.0)
    rays, _ = shadow_rays(without)
    a, _ = tr.trace_rays_posed(rays, None, pose)
    b, _ = tr.trace_rays_posed(rays, None, none)
    same_shadow = (a["hit"] == b["hit"]).reshape(PC.HT, PC.WD)
    lum = lambda c: c[..., :3].astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
    brighter = same_first & same_shadow & (lum(with_cube["color"]) > lum(without["color"]))
    assert is_pose(with_cube["ids"]).sum() > 50 and (same_first & same_shadow).sum() > 500
    assert brighter.sum() >= 30, int(brighter.sum())
    tr.shutdown()


# ---- 7. scale --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1024, TLAS_MAX + 1])
def test_many_poses_first_hit_equals_trace_primary_posed(torch_cuda, count):
    from blok_amd.tracer import HipTracer
    vs = 1.0
    w, h = 64, 48
    tr = HipTracer(w, h).init()
    tr.add_world(PC.world(vs))
    xyz = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    model = tr.model_create(xyz, np.arange(1, 28, dtype=np.uint32))
    rng = np.random.default_rng(count)
    poses = np.concatenate([P.rotation(model, *rng.uniform(-3.0, 3.0, size=3), float(rng.uniform(0.5, 2.0)), (1.5, 1.5, 1.5),
                                       tuple(rng.uniform((-40, 4, -40), (60, 50, 60)))) for _ in range(count)])
    case = PC.Case("many", np.zeros(0, dtype=INSTANCE), poses, (10.0, 60.0, -70.0), (10.0, 15.0, 10.0))
    got, hits, ids = check_first_hit(tr, case, vs)
    assert is_pose(ids).sum() > 200 and len(np.unique(ids[is_pose(ids)])) > 100
    tr.shutdown()


# ---- 8. plumbing ------------------------------------------------------------------------------------------------------------------------------
def test_a_rectangle_is_the_crop_of_the_frame(torch_cuda):
    tr = make_tracer(1.0, *PC.BIG)
    case = PC.table(1.0)[11]
    cam = case.camera(*PC.BIG)
    x0, y0, w, h = PC.RECT
    full = tr.trace_paths_posed(cam, case.instances, case.poses, 2, 2, frame_index=1)
    part = tr.trace_paths_posed(cam, case.instances, case.poses, 2, 2, frame_index=1, rect=PC.RECT)
    for k in PLANES + ("ids",):
        assert part[k].tobytes() == np.ascontiguousarray(full[k][y0:y0 + h, x0:x0 + w]).tobytes(), k
    assert is_pose(part["ids"]).sum() > 50 and (part["ids"] == 0).any()
    tr.shutdown()


def test_two_streams_and_a_table_changed_in_stream_order(torch_cuda, tracers):
    torch = torch_cuda
    tr = tracers[1.0]
    first, second = PC.table(1.0)[0], PC.table(1.0)[1]
    cam = first.camera(PC.WD, PC.HT)
    want = {}
    for name, case in (("first", first), ("second", second)):
        p = tr.trace_paths_posed(cam, None, case.poses, 2, 2, frame_index=4)
        want[name] = (p["color"].tobytes(), p["normal_roughness"].tobytes(), p["ids"].tobytes())
    assert want["first"] != want["second"]
    n = PC.WD * PC.HT
    staged = {name: dev(torch, case.poses) for name, case in (("first", first), ("second", second))}
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            table = staged["first"].clone()
            outs = []
            for name in ("first", "second"):
                color = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
                normal = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
                ids = torch.zeros(n, dtype=torch.int32, device="cuda")
                table.copy_(staged[name], non_blocking=True)                   # the same device table, rewritten in stream order
                tr.trace_paths_posed_device(cam, 0, 0, table.data_ptr(), 1, color_ptr=color.data_ptr(), normal_roughness_ptr=normal.data_ptr(),
                                            ids_ptr=ids.data_ptr(), spp=2, max_bounces=2, frame_index=4, stream=stream.cuda_stream)
                outs.append((name, color, normal, ids))
        stream.synchronize()
        for name, color, normal, ids in outs:
            assert (color.cpu().numpy().tobytes(), normal.cpu().numpy().tobytes(), ids.cpu().numpy().tobytes()) == want[name], name
        tr.release_stream(stream.cuda_stream)


def test_errors_name_the_first_bad_pose_and_touch_nothing(torch_cuda, tracers):
    tr = tracers[1.0]
    lib, ctx = tr._lib, tr._ctx
    case = PC.table(1.0)[0]
    good = case.poses[0]
    cam = np.ascontiguousarray(case.camera(PC.WD, PC.HT))
    n = PC.WD * PC.HT
    bad = []
    for field, at, value, text in (("m", (1, 2), np.nan, "not finite"), ("m", (0, 0), 1025.0, "1024"), ("pivot", (1,), -2.0 ** 20 - 1.0, "pivot"),
                                   ("local", (0,), 2.0 ** 21, "local")):
        p = good.copy()
        p[field][at] = value
        bad.append((p, text))
    p = good.copy()
    p["model"] = 99
    bad.append((p, "unknown model 99"))
    planes = [np.full(n * 4, 7.0, dtype=f32) for _ in range(4)]
    ids = np.full(n, 7, dtype=np.uint32)
    rgba = np.full(n, 7, dtype=np.uint32)
    g = GBuffer(*[a.ctypes.data for a in planes])
    import ctypes as C
    for p, text in bad:
        table = np.array([good, good, p, p], dtype=POSE)
        calls = (lambda: lib.blok_hip_trace_paths_posed(ctx, _ffi.ptr(cam), 0, 0, PC.WD, PC.HT, 2, 2, 0, None, 0, _ffi.ptr(table), 4, C.byref(g), _ffi.ptr(ids)),
                 lambda: lib.blok_hip_draw_frame_rt_posed(ctx, _ffi.ptr(cam), 2, 2, None, None, 0, _ffi.ptr(table), 4, _ffi.ptr(rgba), None))
        for call in calls:
            assert call() == BLOK_ERR_INVALID_ARG
            message = lib.blok_hip_last_error(ctx).decode()
            assert "pose 2:" in message and text in message, message
        assert all((a == 7.0).all() for a in planes) and (ids == 7).all() and (rgba == 7).all()
    table = np.array([good], dtype=POSE)
    # the instanced entries' checks, in their order and with their texts
    assert lib.blok_hip_trace_paths_posed(ctx, _ffi.ptr(cam), 0, 0, PC.WD, PC.HT, 2, 2, 0, None, 0, _ffi.ptr(table), 1, None, None) == BLOK_ERR_INVALID_ARG
    assert "null planes" in lib.blok_hip_last_error(ctx).decode()
    assert lib.blok_hip_trace_paths_posed(ctx, _ffi.ptr(cam), 90, 0, PC.WD, PC.HT, 2, 2, 0, None, 0, _ffi.ptr(table), 1, C.byref(g), None) == BLOK_ERR_INVALID_ARG
    assert "rectangle outside the frame" in lib.blok_hip_last_error(ctx).decode()
    assert lib.blok_hip_trace_paths_posed(ctx, _ffi.ptr(cam), 0, 0, PC.WD, PC.HT, 0, 2, 0, None, 0, _ffi.ptr(table), 1, C.byref(g), None) == BLOK_ERR_INVALID_ARG
    assert "bad path-trace arguments" in lib.blok_hip_last_error(ctx).decode()
    assert lib.blok_hip_trace_paths_posed_device(ctx, _ffi.ptr(cam), 0, 0, PC.WD, PC.HT, 2, 2, 0, None, 0, None, 3, C.byref(g), None, None) == BLOK_ERR_INVALID_ARG
    assert "null pose table" in lib.blok_hip_last_error(ctx).decode()
    assert lib.blok_hip_trace_paths_posed_device(ctx, _ffi.ptr(cam), 0, 0, PC.WD, PC.HT, 2, 2, 0, None, 2, None, 0, C.byref(g), None, None) == BLOK_ERR_INVALID_ARG
    assert "null instance table" in lib.blok_hip_last_error(ctx).decode()
    with pytest.raises(BlokError) as e:
        tr.trace_paths_posed(cam, np.array([IO.instance(99, (0, 0, 0))], dtype=INSTANCE), table, 1, 1)
    assert "instance 0:" in str(e.value)
    assert all((a == 7.0).all() for a in planes) and (ids == 7).all()


def test_device_tables_skip_an_unusable_pose_and_need_no_instances(torch_cuda, tracers):
    torch = torch_cuda
    tr = tracers[1.0]
    case = PC.table(1.0)[0]
    good = case.poses[0]
    nan, unknown, far = good.copy(), good.copy(), good.copy()
    nan["m"][0, 0] = np.nan
    unknown["model"] = 1000
    far["pivot"][2] = 2.0 ** 21
    table = np.array([nan, unknown, far, good], dtype=POSE)
    cam = case.camera(PC.WD, PC.HT)
    want = tr.trace_paths_posed(cam, None, case.poses, 2, 2, frame_index=6)           # n_instances == 0 with a pose
    won = want["ids"] == POSE_ID
    assert won.sum() > 300
    n = PC.WD * PC.HT
    b = {k: torch.zeros(n * 4, dtype=torch.float32, device="cuda") for k in PLANES}
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_table = dev(torch, table)
    tr.trace_paths_posed_device(cam, 0, 0, d_table.data_ptr(), 4, color_ptr=b["color"].data_ptr(), world_pos_ptr=b["world_pos"].data_ptr(),
                                normal_roughness_ptr=b["normal_roughness"].data_ptr(), albedo_metallic_ptr=b["albedo_metallic"].data_ptr(),
                                ids_ptr=ids.data_ptr(), spp=2, max_bounces=2, frame_index=6)
    torch.cuda.synchronize()
    for k in PLANES:
        assert b[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    got_ids = ids.cpu().numpy().view(np.uint32).reshape(PC.HT, PC.WD)
    assert (got_ids[won] == (POSE_ID | 3)).all() and (got_ids[~won] == want["ids"][~won]).all()
