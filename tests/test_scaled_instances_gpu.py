"""GPU: instanced models at power-of-two scales (include/blok_hip.h, "Scaled models"; blok_hip_model_set_scale).

References: the oracle composition over per-model voxel sizes (tests/scaled_instance_oracle.py), numpy integer geometry (no oracle), the
same table without the calls (scale 0), a reduced level installed as a world at voxel size 4 (the LOD chain), trace_primary_instanced
and the host build of the instance BVH (the path-traced frame), a float64 slab test (the shadow) and the object-motion formula of
tests/test_instance_motion_gpu.py.  Every comparison is exact unless stated otherwise; frames are at most 96 x 64."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import columns as COL
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, INSTANCE_NONE, BlokError
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests import scaled_instance_oracle as SO
from tests.conftest import SEED, records_equal
from tests.test_scaled_instances_cpu import aimed_rays, box_of, build_shim, handle_array, shim_model

pytestmark = pytest.mark.gpu

WD, HT = 96, 64
EXPONENTS = (0, 1, 2, 3)
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def models():
    return IO.procedural_models()


@functools.lru_cache(maxsize=None)
def small_world(voxel_size):
    """A ground plate and a seeded cloud of voxels above it, in a lattice of the given voxel size (computed once per size, never changed)."""
    rng = np.random.default_rng(5)
    cm = W.ChunkManager(128, voxel_size)
    wall = np.array([(x, 0, z) for x in range(-40, 60) for z in range(-40, 60)], dtype=np.int32)
    pts = rng.integers(-40, 60, size=(1500, 3)).astype(np.int32)
    xyz = np.concatenate([wall, pts])
    cm.set_voxels(xyz, rng.integers(1, 60, size=len(xyz)).astype(np.uint32))
    cm.rebuild_dirty_chunks()
    return cm.pack_chunks_to_gpu_svo(W.scene_materials(SEED))


def make_tracer(pw, models, exponents, voxel_size=1.0, w=WD, h=HT):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(w, h).init()
    if voxel_size != 1.0:
        tr.set_voxel_size(voxel_size)
    tr.add_world(pw)
    ids = [tr.model_create(xyz, mats) for xyz, mats in models]
    assert ids == list(range(len(models)))
    for m, e in zip(ids, exponents):
        assert tr.model_scale(m) == 0
        tr.model_set_scale(m, e)
        assert tr.model_scale(m) == e
    return tr


def mixed_table(n_models):
    """24 instances: every model (so every exponent) six times, varied orientations, offsets that are no multiples of the cell sizes; some sunk
    into the ground plate and the cloud, some overlapping each other, one exact duplicate (a tie between instances)."""
    rng = np.random.default_rng(12)
    picks = [IO.SIGNED_PERMUTATIONS[i] for i in rng.permutation(48)[:24]]
    table = np.array([IO.instance(i % n_models, rng.integers(-30, 50, size=3), p, f) for i, (p, f) in enumerate(picks)], dtype=INSTANCE)
    table[20]["offset"] = table[3]["offset"] + (5, -3, 2)          # overlaps instance 3 (the same model: model ids repeat every four)
    table[21]["offset"] = (11, 1, 13)                                # sunk into the plate
    table[22]["offset"] = (-7, -2, 21)
    table[23] = table[5]                                              # a duplicate: the lower index wins every tie
    return table


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel_size", [1.0, 0.5])
def test_frames_and_rays_equal_the_oracle_composition(torch_cuda, models, voxel_size):
    vs = voxel_size
    pw = small_world(vs)
    omodels = [SO.scaled_model(xyz, mats, e, vs) for (xyz, mats), e in zip(models, EXPONENTS)]
    tr = make_tracer(pw, models, EXPONENTS, vs)
    table = mixed_table(len(models))
    tr.check_instances(table)
    lattice = O.Lattice(pw.nodes, pw.sub_chunks)
    won_by = set()
    for cam in (W.camera_look_at((90.0 * vs, 70.0 * vs, -70.0 * vs), (10.0 * vs, 5.0 * vs, 10.0 * vs), 60.0, WD, HT),
                W.camera_look_at((3.3 * vs, 20.2 * vs, 7.7 * vs), (40.0 * vs, 0.0, 31.0 * vs), 95.0, WD, HT)):
        rays = O.primary_rays(cam, WD, HT)
        world, _ = lattice.trace(rays, threads=8)
        want, want_ids = SO.compose(world, rays, table, omodels, EXPONENTS, vs)
        hits, ids, rgba = tr.trace_primary_instanced(cam, table)
        bad = np.flatnonzero(~records_equal(hits.reshape(-1), want) | (ids.reshape(-1) != want_ids))
        assert bad.size == 0, f"{bad.size} pixels differ; first {bad[:4]}: got {hits.reshape(-1)[bad[:2]]} {ids.reshape(-1)[bad[:2]]}, want {want[bad[:2]]} {want_ids[bad[:2]]}"
        assert (rgba.reshape(-1) == IO.shade(want, pw.materials)).all()
        won = want_ids != INSTANCE_NONE
        assert won.sum() > 500 and (world["hit"][won] == 1).sum() > 50 and (want_ids == INSTANCE_NONE).sum() > 200
        won_by |= set(int(table[i]["model"]) for i in np.unique(want_ids[won]))
        assert not (want_ids == 23).any()
    assert won_by == {0, 1, 2, 3}                                    # every exponent is on screen
    boxes = [box_of(xyz) for xyz, _ in models]
    rays = aimed_rays(table, boxes, EXPONENTS, vs, per_instance=100, n_miss=100, seed=3, reach=150.0)
    world, _ = lattice.trace(rays, threads=8)
    want, want_ids = SO.compose(world, rays, table, omodels, EXPONENTS, vs)
    hits, ids = tr.trace_rays_instanced(rays, table)
    assert records_equal(hits, want).all() and (ids == want_ids).all()
    assert (want_ids != INSTANCE_NONE).sum() > 800 and len(np.unique(want_ids)) > 15
    tr.shutdown()


# ---- 2. closed form, no oracle ---------------------------------------------------------------------------------------------------------------
CELLS = np.array([(0, 0, 0), (2, 1, 0), (1, 3, 2), (2, 1, 1)], dtype=np.int32)          # model cells; material = 10 + index
CELL = 8                                                                               # e = 3


def closed_form_table():
    """48 instances of the one model, one per orientation, in a grid above the world's cloud; the model reaches 4 cells = 32 voxels from
    its offset at most, the grid is 80 apart: no two boxes touch.  Offsets are no multiples of 8."""
    return np.array([IO.instance(0, (80 * (i % 8) - 300 + (3 * i) % 7, 200 + i % 5, 80 * (i // 8) - 220 + (5 * i) % 7), p, f)
                     for i, (p, f) in enumerate(IO.SIGNED_PERMUTATIONS)], dtype=INSTANCE)


def cell_boxes(table):
    """(instance, cell, lo[3]) of every cell of every instance, in world voxels, by the header's rule."""
    out = []
    for i, inst in enumerate(table):
        for c, v in enumerate(CELLS):
            lo = np.zeros(3, dtype=np.int64)
            for k in range(3):
                a, o = int(inst["axis"][k]), int(inst["offset"][int(inst["axis"][k])])
                lo[a] = o - (int(v[k]) + 1) * CELL if (int(inst["flip"]) >> k) & 1 else o + int(v[k]) * CELL
            out.append((i, c, lo))
    return out


def closed_form_rays(table):
    """Axis-parallel rays through every cell of every instance from both sides of every axis, from integer-plus-half origins 4.5 and 20.5
    voxels before the cell (left out where that point lies inside another cell), and per ray (t, material, voxel, face, instance) of the first
    cell on its line over all cells of all instances: integer comparisons only."""
    boxes = cell_boxes(table)
    los = np.array([b[2] for b in boxes])
    rays, want = [], []
    for i, c, lo in boxes:
        for axis in range(3):
            for sign in (1, -1):
                for back in (4.5, 20.5):
                    org = lo + 3.5                                                  # inside the cell on the two other axes
                    org[axis] = (lo[axis] - back) if sign > 0 else (lo[axis] + CELL + back)
                    if ((los <= np.floor(org)) & (np.floor(org) < los + CELL)).all(axis=1).any():
                        continue
                    others = [a for a in range(3) if a != axis]
                    on_line = ((los[:, others] <= np.floor(org[others])) & (np.floor(org[others]) < los[:, others] + CELL)).all(axis=1)
                    ahead = (los[:, axis] > org[axis]) if sign > 0 else (los[:, axis] + CELL < org[axis])
                    cand = np.flatnonzero(on_line & ahead)
                    first = cand[np.argmin(los[cand, axis] * sign)]
                    plane = los[first, axis] if sign > 0 else los[first, axis] + CELL
                    direction = [0.0, 0.0, 0.0]
                    direction[axis] = float(sign)
                    rays.append((tuple(org), 0.001, tuple(direction), 10000.0))
                    want.append((float(abs(plane - org[axis])), 10 + boxes[first][1], tuple(int(v) for v in los[first]), 2 * axis + (1 if sign > 0 else 0),
                                 boxes[first][0]))
    return np.array(rays, dtype=_ffi.RAY), want


def test_axis_parallel_rays_hit_the_cells_of_integer_geometry(torch_cuda):
    pw = small_world(1.0)
    tr = make_tracer(pw, [(CELLS, 10 + np.arange(len(CELLS), dtype=np.uint32))], (3,))
    table = closed_form_table()
    tr.check_instances(table)
    rays, want = closed_form_rays(table)
    assert len(rays) > 2000 and (rays["org"][:, 1] > 100).all()                 # the world's cloud ends below 60: nothing else is hit
    assert all(float(np.float32(t)) == t for t, *_ in want)                     # every t is exactly representable
    hits, ids = tr.trace_rays_instanced(rays, table)
    for h, i, (t, mat, voxel, face, inst) in zip(hits, ids, want):
        got = (int(h["hit"]), float(h["t"]), int(h["material_id"]), tuple(int(v) for v in h["voxel"]), int(h["face"]), int(i))
        assert got == (1, t, mat, voxel, face, inst), (got, (t, mat, voxel, face, inst))
    tr.shutdown()


# ---- 3. scale 0 is today's -------------------------------------------------------------------------------------------------------------------
def test_set_scale_zero_changes_no_byte(torch_cuda, models):
    pw = small_world(1.0)
    table = mixed_table(len(models))
    cams = (W.camera_look_at((90.0, 70.0, -70.0), (10.0, 5.0, 10.0), 60.0, WD, HT), W.camera_look_at((3.3, 20.2, 7.7), (40.0, 0.0, 31.0), 95.0, WD, HT))
    frames = []
    for with_calls in (False, True):
        from blok_amd.tracer import HipTracer
        tr = HipTracer(WD, HT).init()
        tr.add_world(pw)
        for xyz, mats in models:
            m = tr.model_create(xyz, mats)
            if with_calls:
                tr.model_set_scale(m, 0)
        out = []
        for cam in cams:
            hits, ids, rgba = tr.trace_primary_instanced(cam, table)
            paths = tr.trace_paths_instanced(cam, table, 2, 2, frame_index=1)
            out.append(b"".join(a.tobytes() for a in (hits, ids, rgba, paths["color"], paths["world_pos"], paths["ids"])))
        frames.append(out)
        tr.shutdown()
    assert frames[0] == frames[1]


# ---- 4. the LOD chain ------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_a_reduced_level_as_a_scaled_instance_equals_the_coarse_world(torch_cuda, keyed):
    from blok_amd.tracer import HipTracer
    origin, shape = (-5, -3, -2), (32, 32, 32)
    rng = np.random.default_rng(44)
    d = (rng.random(shape[::-1]) < 0.08).astype(np.float32)
    m = np.where(d > 0, rng.integers(1, 4, size=shape[::-1]), 0).astype(np.uint32)
    fine, coarse = HipTracer(WD, HT).init(), HipTracer(WD, HT).init()
    try:
        fine.set_volume_layout(keyed)
        fine.volume_create(origin, shape)
        fine.volume_upload(d, m)
        info = fine.volume_reduce(None, None, 2, _ffi.LOD_VOTE_EXPOSED)
        n, ids = fine.volume_lod_download(2, 0), fine.volume_lod_download(2, 2)
        clo = np.array([int(c) for c in info["level"][0][1]["clo"]])
        model = fine.volume_lod_model(2, 1)
        assert fine.model_scale(model) == 0 and fine.last_capture_voxels == int((n >= 1).sum()) > 100
        fine.model_set_scale(model, 2)
        fine.volume_upload(np.zeros_like(d), np.zeros_like(m))                  # the fine voxels leave: an emptied volume is an empty world
        fine.volume_rebuild()
        table = np.array([IO.instance(model, clo * 4)], dtype=INSTANCE)
        fine.check_instances(table)
        coarse.set_voxel_size(4.0)
        coarse.add_dense(np.where(n >= 1, ids, 0).astype(np.uint32), tuple(int(c) for c in clo))
        total = 0
        for pos, target in (((60.25, 50.5, -40.75), (11.0, 13.0, 14.0)), ((10.25, 12.5, 13.75), (40.0, 30.0, -20.0)), ((-30.5, 70.0, 60.25), (12.0, 10.0, 12.0))):
            cam = W.camera_look_at(pos, target, 70.0, WD, HT)                   # positions on the 1/4 grid: o - offset is exact
            got, got_ids, _ = fine.trace_primary_instanced(cam, table)
            want = coarse.draw_frame(cam)
            assert got["hit"].tobytes() == want["hit"].tobytes()
            hit = want["hit"] == 1
            for k in ("t", "material_id", "face"):
                assert got[k][hit].tobytes() == want[k][hit].tobytes(), k
            assert (got["voxel"][hit].astype(np.int64) == 4 * want["voxel"][hit].astype(np.int64)).all()
            assert ((got_ids == 0) == hit).all()
            total += int(hit.sum())
        assert total > 3000
    finally:
        fine.shutdown()
        coarse.shutdown()


# ---- 5. path-traced ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4097])
def test_path_first_hits_equal_trace_primary_instanced(torch_cuda, scene64, models, n):
    from tests.test_instance_paths_gpu import check_first_hit
    _, pw = scene64
    tr = make_tracer(pw, models, EXPONENTS)
    # (the cameras look at the field from far outside it; the winners below were counted with the oracle composition)
    reach, eye = ((-40, 100), (32.0, 170.0, -150.0)) if n == 64 else ((-150, 214), (32.0, 420.0, -380.0))
    cam = W.camera_look_at(eye, (32.0, 20.0, 32.0), 60.0, WD, HT)
    table = IO.random_instances(n, len(models), *reach, seed=n)
    table[:48]["axis"] = [p for p, f in IO.SIGNED_PERMUTATIONS]
    table[:48]["flip"] = [f for p, f in IO.SIGNED_PERMUTATIONS]
    table[n // 2: n // 2 + 8] = table[:8]                                       # duplicates: ties between instances
    _, ids = check_first_hit(tr, cam, table, spp=2, bounces=2)
    won = ids[ids != INSTANCE_NONE]
    assert len(won) > 3000 and len(np.unique(won)) > 40 and {int(table[i]["model"]) for i in np.unique(won)} == {0, 1, 2, 3}
    tr.shutdown()


def test_device_bvh_equals_the_host_build_with_scales(torch_cuda, scene64, models, tmp_path):
    torch = torch_cuda
    _, pw = scene64
    tr = make_tracer(pw, models, EXPONENTS)
    shim = build_shim(tmp_path / "libscaled_instance_shim.so")
    handles = [shim_model(shim, xyz, mats, e) for (xyz, mats), e in zip(models, EXPONENTS)]
    arr = handle_array(handles)
    for n in (1, 7, 300, 4096):
        table = IO.random_instances(n, len(models) + 1, -300, 300, seed=n)        # model ids up to len(models): unknown ones are left out
        if n > 4:
            table[3] = table[1]
            table[2]["offset"] = (32768 - 40, 0, 0)                               # model 2 (e = 2) reaches 80 voxels or more: off the lattice
            table[2]["model"], table[2]["axis"], table[2]["flip"] = 2, (0, 1, 2), 0
        host = np.zeros((shim.ts_node_count(n), 8), dtype=np.int32)
        shim.ss_build(arr, len(handles), C.c_void_p(table.ctypes.data), n, 1.0, C.c_void_p(host.ctypes.data))
        dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        got = tr.debug_build_tlas(dev.data_ptr(), n)
        assert got.tobytes() == host.tobytes(), n
        if n > 4:
            assert int(host[0, 7]) < n                                            # (the header's usable count: some were left out)
    for h in handles:
        shim.is_free(h)
    tr.shutdown()


def slab(o, d, lo, hi, t0, t1):
    """float64: does o + t d, t in [t0, t1), meet the box [lo, hi)?  Per ray."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (lo - o) / d, (hi - o) / d
    return np.maximum(np.minimum(a, b).max(axis=1), t0) < np.minimum(np.maximum(a, b).min(axis=1), t1)


def test_a_floating_scaled_cell_casts_its_shadow(torch_cuda):
    """A flat ground, one model voxel at e = 3 (an 8^3 cube) floating above it, one sample, no bounce.  Each ground pixel's shadow segment
    is rebuilt from the G-buffer (path_core.h: origin = position + 0.001 n, towards the sun, [0.001, 1000)) and slab-tested in float64
    against the cube.  The pose was chosen on the CPU (pixel centres on the plane y = 1): 603 shadowed pixels, 19 within 0.05 voxel of
    the cube's surface."""
    from blok_amd.tracer import HipTracer
    cm = W.ChunkManager(128, 1.0)
    ground = np.array([(x, 0, z) for x in range(64) for z in range(64)], dtype=np.int32)
    cm.set_voxels(ground, np.full(len(ground), 3, dtype=np.uint32))
    cm.rebuild_dirty_chunks()
    pw = cm.pack_chunks_to_gpu_svo(W.scene_materials(SEED))
    tr = HipTracer(WD, HT).init()
    tr.add_world(pw)
    model = tr.model_create([(0, 0, 0)], [5])
    tr.model_set_scale(model, 3)
    lo = np.array([28.0, 12.0, 28.0])
    table = np.array([IO.instance(model, (28, 12, 28))], dtype=INSTANCE)
    cam = W.camera_look_at((30.3, 36.0, 12.2), (22.0, 1.0, 26.5), 40.0, WD, HT)
    got = tr.trace_paths_instanced(cam, table, 1, 1, frame_index=0)
    bare = tr.trace_paths_instanced(cam, table[:0], 1, 1, frame_index=0)
    on_ground = (got["ids"] == INSTANCE_NONE) & (got["world_pos"][..., 3] < 10000.0)
    assert (got["ids"] == 0).sum() > 100 and on_ground.sum() > 3000
    pos = got["world_pos"][..., :3].astype(np.float64).reshape(-1, 3)
    normal = got["normal_roughness"][..., :3].astype(np.float64).reshape(-1, 3)
    sun = np.array([0.5, 0.8, 0.3], dtype=np.float32)
    sun = (sun / np.sqrt((sun * sun).sum(dtype=np.float32))).astype(np.float64)
    origin = pos + 0.001 * normal
    direction = np.broadcast_to(sun, origin.shape)
    meets = slab(origin, direction, lo + 0.05, lo + 8 - 0.05, 0.001, 1000.0).reshape(HT, WD) & on_ground
    near = slab(origin, direction, lo - 0.05, lo + 8 + 0.05, 0.001, 1000.0).reshape(HT, WD) & on_ground
    clear = on_ground & ~near
    left_out = near & ~meets
    print(f"shadowed {meets.sum()}, left out {left_out.sum()}, clear {clear.sum()}")
    assert meets.sum() > 300 and left_out.sum() <= 0.05 * meets.sum()
    lum = lambda c: c[..., :3].sum(-1)
    assert (lum(got["color"])[meets] < lum(bare["color"])[meets]).all()
    assert got["color"][clear].tobytes() == bare["color"][clear].tobytes()
    tr.shutdown()


# ---- 6. object motion --------------------------------------------------------------------------------------------------------------------------
def test_a_scaled_instance_that_moves_gets_the_formulas_motion(torch_cuda, scene64):
    from tests.test_instance_motion_gpu import dev_table, erode, object_motion, plate, ref_planes, trace_ref
    torch = torch_cuda
    _, pw = scene64
    tr = make_tracer(pw, [plate(16, 1, 16)], (1,))                             # a 32 x 2 x 32 voxel plate of 2-voxel cells
    cam = W.camera_look_at((44.0, 130.0, 20.0), (44.0, 10.0, 46.0), 70.0, WD, HT)
    prev_cam = W.camera_look_at((45.0, 129.0, 21.0), (44.0, 10.0, 46.0), 70.0, WD, HT)
    prev_vp = tr.camera_view_proj(prev_cam)
    prev = np.array([IO.instance(0, (25, 70, 31))], dtype=INSTANCE)
    cur = prev.copy()
    cur[0]["offset"] = prev[0]["offset"] + (3, 0, -2)
    tc, tp = dev_table(torch, cur), dev_table(torch, prev)
    n = WD * HT
    P = ref_planes(torch, n)
    trace_ref(tr, cam, P, tc, 1, prev_vp, 1)
    m2 = torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda")
    tr.instance_motion_device(P["world_pos"].data_ptr(), P["ids"].data_ptr(), tc.data_ptr(), 1, tp.data_ptr(), 1, prev_vp,
                              motion_h_ptr=P["motion"].data_ptr(), motion_ptr=m2.data_ptr())
    torch.cuda.synchronize()
    ids = P["ids"].cpu().numpy().view(np.uint32).reshape(HT, WD)
    wp = P["world_pos"].cpu().numpy().reshape(HT, WD, 4)
    tracked, want = object_motion(wp, ids, cur, prev, prev_vp, frame_w=WD, frame_h=HT)
    assert tracked.sum() > 150 and (tracked == (ids == 0)).all()
    got_h = P["motion"].cpu().numpy().view(np.uint16).reshape(HT, WD, 2)
    got_f = m2.cpu().numpy().reshape(HT, WD, 2)
    assert got_f[tracked].tobytes() == want[tracked].tobytes()
    assert np.array_equal(got_h[tracked], want[tracked].astype(np.float16).view(np.uint16))
    assert (np.abs(got_f[tracked]) > 1e-3).all() and (got_f[~tracked] == -7.0).all()
    # the frame entry: history accumulates on the resting plate, and starts over after set_scale (to the same exponent, even)
    for k in range(3):
        tr.draw_frame_rt_instanced_motion(cam, cur, spp=2)
    _, ids, _ = tr.trace_primary_instanced(cam, cur)
    plate_px = erode(ids == 0, 2)
    assert plate_px.sum() > 50 and (tr.denoise_state()[2][plate_px] >= 3).all()
    tr.model_set_scale(0, 1)
    tr.draw_frame_rt_instanced_motion(cam, cur, spp=2)
    assert (tr.denoise_state()[2][plate_px] == 1).all()
    tr.draw_frame_rt_instanced_motion(cam, cur, spp=2)
    assert (tr.denoise_state()[2][plate_px] == 2).all()
    tr.shutdown()


# ---- 7. errors and life ------------------------------------------------------------------------------------------------------------------------
def test_check_instances_names_the_first_instance_over_a_limit(torch_cuda, models):
    from blok_amd.tracer import HipTracer
    tr = make_tracer(small_world(1.0), models, EXPONENTS)
    good = mixed_table(len(models))[:6]
    box_hi = int(models[3][0][:, 0].max()) + 1                                 # model 3 (e = 3) ends box_hi cells from its offset on x
    edge = IO.instance(3, (32768 - 8 * box_hi, 0, 0))
    tr.check_instances(np.concatenate([good, np.array([edge], dtype=INSTANCE)]))       # a span ending exactly at 32768
    over = edge.copy()
    over["offset"][0] += 1
    rays = aimed_rays(good, [box_of(x) for x, _ in models], EXPONENTS, 1.0, 2, 0, 1)
    cam = W.camera_look_at((90.0, 70.0, -70.0), (10.0, 5.0, 10.0), 60.0, WD, HT)
    table = np.concatenate([good, np.array([over, over], dtype=INSTANCE)])
    for call in (lambda: tr.check_instances(table), lambda: tr.trace_primary_instanced(cam, table), lambda: tr.trace_rays_instanced(rays, table),
                 lambda: tr.trace_paths_instanced(cam, table, 1, 1)):
        with pytest.raises(BlokError) as e:
            call()
        assert e.value.status == BLOK_ERR_INVALID_ARG and "instance 6:" in str(e.value) and "lattice" in str(e.value)
    tr.model_set_scale(3, 0)
    tr.check_instances(table)                                                   # at scale 0 the same table is far inside
    for bad in (9, 10, 0xFFFFFFFF):
        with pytest.raises(BlokError) as e:
            tr.model_set_scale(3, bad)
        assert e.value.status == BLOK_ERR_INVALID_ARG and tr.model_scale(3) == 0
    tr.shutdown()
    # the limit of the model's voxel size: vs * 2^e = 256 passes, 512 is named
    big = HipTracer(WD, HT).init()
    big.set_voxel_size(64.0)
    big.add_dense(np.ones((2, 2, 2), dtype=np.uint32))
    a, b = big.model_create([(0, 0, 0)], [1]), big.model_create([(0, 0, 0), (1, 0, 0)], [1, 2])
    big.model_set_scale(a, 2)
    big.model_set_scale(b, 3)
    big.check_instances(np.array([IO.instance(a, (0, 0, 0))] * 3, dtype=INSTANCE))
    with pytest.raises(BlokError) as e:
        big.check_instances(np.array([IO.instance(a, (0, 0, 0)), IO.instance(a, (5, 5, 5)), IO.instance(b, (0, 0, 0)), IO.instance(b, (9, 9, 9))], dtype=INSTANCE))
    assert e.value.status == BLOK_ERR_INVALID_ARG and "instance 2:" in str(e.value) and "256" in str(e.value)
    big.shutdown()


@LAYOUTS
def test_volume_entries_refuse_scaled_models(torch_cuda, keyed):
    from blok_amd.tracer import HipTracer
    from blok_amd import stamp as ST
    rng = np.random.default_rng(8)
    shape = (24, 16, 20)
    d = (rng.random(shape[::-1]) < 0.3).astype(np.float32)
    m = np.where(d > 0, rng.integers(1, 9, size=shape[::-1]), 0).astype(np.uint32)
    tr = HipTracer(WD, HT).init()
    tr.set_volume_layout(keyed)
    tr.volume_create((-3, 2, 5), shape)
    tr.volume_upload(d, m)
    plain = tr.model_create([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [4, 5, 6])
    scaled = tr.model_create([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [4, 5, 6])
    tr.model_set_scale(scaled, 1)
    place = lambda model: np.concatenate([ST.placement((2, 6, 9), model=plain), ST.placement((4, 8, 11), (2, 1, 0), 3, model=model)])
    # the scale-0 twin passes everywhere (on a copy of the state: the volume is restored afterwards)
    assert tr.volume_stamp_models(place(plain)) > 0
    tr.volume_upload(d, m)
    tr.volume_sweep_models(place(plain), 3, 8)
    tr.volume_column_field()
    params = COL.scatter_params(seed=3, flags=_ffi.SCATTER_ANY_MATERIAL, cell_log2=2)
    kept = tr.volume_scatter_models(params, COL.scatter_entries([(plain, 1, (0, 0, 0), 0)]))
    kept_table = tr.volume_scatter_download()
    assert int(kept["n_placed"][0]) > 0
    for call in (lambda: tr.volume_stamp_models(place(scaled)), lambda: tr.volume_stamp_models(place(scaled), _ffi.STAMP_ERASE),
                 lambda: tr.volume_sweep_models(place(scaled), 3, 8),
                 lambda: tr.volume_scatter_models(params, COL.scatter_entries([(plain, 1, (0, 0, 0), 0), (scaled, 2, (0, 0, 0), 0)]))):
        with pytest.raises(BlokError) as e:
            call()
        assert e.value.status == BLOK_ERR_UNSUPPORTED, str(e.value)
        got_d, got_m = tr.volume_download()
        assert got_d.tobytes() == d.tobytes() and got_m.tobytes() == m.tobytes()
    assert tr.volume_scatter_info().tobytes() == kept.tobytes() and tr.volume_scatter_download().tobytes() == kept_table.tobytes()
    assert tr.model_create([(0, 0, 0)], [1]) == scaled + 1                       # no id was consumed
    tr.model_set_scale(scaled, 0)                                                 # back at scale 0 the model is taken again
    assert tr.volume_stamp_models(place(scaled)) > 0
    tr.shutdown()


def test_the_size_limit_follows_the_worlds_voxel_size(torch_cuda):
    """One cell at e = 8 over a single-voxel dense world: vm = 256 at voxel size 1 (traced), 512 at voxel size 2 (the host table is refused,
    the device table's instance skipped), 256 again behind a world of voxel size 1.  The device entries never see a host check: what they
    skip is what the model store wrote into its device copy of the descriptors when the world was installed."""
    torch = torch_cuda
    from blok_amd.tracer import HipTracer
    tr = HipTracer(WD, HT).init()
    far_voxel = np.zeros((1, 1, 1), dtype=np.uint32) + 1
    model = tr.model_create([(0, 0, 0)], [2])
    tr.model_set_scale(model, 8)
    table = np.array([IO.instance(model, (-128, -128, 300))], dtype=INSTANCE)          # the cube [-128, 128)^2 x [300, 556), voxels
    dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    ids = torch.zeros(WD * HT, dtype=torch.int32, device="cuda")
    won = []
    for vs in (1.0, 2.0, 1.0, 0.5):
        tr.set_voxel_size(vs)
        tr.add_dense(far_voxel, (-2000, -2000, -2000))
        cam = W.camera_look_at((0.0, 0.0, 0.0), (0.0, 0.0, 400.0 * vs), 60.0, WD, HT)
        tr.trace_primary_instanced_device(cam, dev.data_ptr(), 1, 0, 0, ids.data_ptr())
        torch.cuda.synchronize()
        won.append(int((ids.cpu().numpy().view(np.uint32) == 0).sum()))
        if vs == 2.0:
            with pytest.raises(BlokError) as e:
                tr.check_instances(table)
            assert e.value.status == BLOK_ERR_INVALID_ARG and "instance 0:" in str(e.value) and "256" in str(e.value)
        else:
            tr.check_instances(table)
    assert won[0] > 500 and won[1] == 0 and won[2] == won[0] and won[3] > 500, won
    tr.shutdown()


def test_scale_follows_the_models_life(torch_cuda):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(WD, HT).init()
    a = tr.model_create([(0, 0, 0)], [1])
    b = tr.model_create([(0, 0, 0), (1, 1, 1)], [1, 2])
    assert (tr.model_scale(a), tr.model_scale(b)) == (0, 0)
    tr.model_set_scale(a, 8)
    tr.model_set_scale(b, 5)
    assert (tr.model_scale(a), tr.model_scale(b)) == (8, 5)
    nodes, mats, info = tr.model_download(b)                                      # the download reports what it reported: model voxels
    assert info["lo"] == (0, 0, 0) and info["hi"] == (2, 2, 2) and len(mats) == 2
    tr.model_destroy(a)
    for call in (lambda: tr.model_scale(a), lambda: tr.model_set_scale(a, 1), lambda: tr.model_scale(b + 1), lambda: tr.model_set_scale(b + 7, 0)):
        with pytest.raises(BlokError) as e:
            call()
        assert e.value.status == BLOK_ERR_INVALID_ARG
    assert tr._lib.blok_hip_model_scale(tr._ctx, b, None) == BLOK_ERR_INVALID_ARG
    c = tr.model_create([(0, 0, 0)], [1])
    assert c == b + 1 and tr.model_scale(c) == 0 and tr.model_scale(b) == 5       # ids are never reused; a new model starts at scale 0
    tr.shutdown()
