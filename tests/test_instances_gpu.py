"""GPU: instanced voxel models (include/blok_hip.h) against the oracle composition (tests/instance_oracle.py), bit for bit.

Every expected record and instance id comes from the existing oracle: each model traced alone on rays moved into its local space in
numpy, mapped back and composed with the world's records by the tie rule.  RGBA8 must be shade_rgba of the expected records."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import world as W
from blok_amd._ffi import INSTANCE, INSTANCE_NONE
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests.conftest import SEED, edge_case_rays, random_rays, records_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def models():
    return IO.procedural_models()


@pytest.fixture(scope="module")
def oracle_models(models):
    return [IO.OracleModel(xyz, mats) for xyz, mats in models]


def make_tracer(pw, w, h, models, voxel_size=1.0):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(w, h).init()
    if voxel_size != 1.0:
        tr.set_voxel_size(voxel_size)
    tr.add_world(pw)
    ids = [tr.model_create(xyz, mats) for xyz, mats in models]
    assert ids == list(range(len(models)))
    return tr


def expected_frame(pw, cam, w, h, table, omodels, rect=None, voxel_size=1.0):
    x0, y0, rw, rh = rect if rect is not None else (0, 0, w, h)
    rays = O.primary_rays(cam, w, h, x0, y0, rw, rh)
    world, _ = O.Lattice(pw.nodes, pw.sub_chunks).trace(rays, threads=8)
    hits, ids = IO.compose(world, rays, table, omodels, voxel_size)
    return world, hits, ids


def check_frame(tr, pw, cam, table, omodels, rect=None, voxel_size=1.0):
    w, h = tr.width, tr.height
    world, want, want_ids = expected_frame(pw, cam, w, h, table, omodels, rect, voxel_size)
    hits, ids, rgba = tr.trace_primary_instanced(cam, table, rect)
    bad = np.flatnonzero(~records_equal(hits.reshape(-1), want) | (ids.reshape(-1) != want_ids))
    assert bad.size == 0, f"{bad.size} pixels differ; first {bad[:4]}: got {hits.reshape(-1)[bad[:2]]} {ids.reshape(-1)[bad[:2]]}, want {want[bad[:2]]} {want_ids[bad[:2]]}"
    assert (rgba.reshape(-1) == IO.shade(want, pw.materials)).all()
    return world, want, want_ids


def camera_inside(table, i, models, w, h):
    """A camera inside instance i's world box, looking along +x."""
    inst = table[i]
    xyz = models[int(inst["model"])][0]
    lo = np.zeros(3)
    hi = np.zeros(3)
    for k in range(3):
        a = int(inst["axis"][k])
        o = int(inst["offset"][a])
        mlo, mhi = xyz[:, k].min(), xyz[:, k].max() + 1
        lo[a], hi[a] = ((o - mhi, o - mlo) if (int(inst["flip"]) >> k) & 1 else (o + mlo, o + mhi))
    c = (lo + hi) / 2 + 0.37
    return W.camera_look_at(tuple(c), tuple(c + np.array([10.0, -2.0, 3.0])), 70.0, w, h)


def test_no_instances_and_off_screen_equal_the_plain_entry(torch_cuda, scene64, models):
    torch = torch_cuda
    cm, pw = scene64
    w, h = 256, 192
    tr = make_tracer(pw, w, h, models)
    cam = W.scene_camera(64, 0, w, h, SEED)
    pos, fwd = cam["pos"][0].astype(np.float64), cam["fwd"][0].astype(np.float64)
    behind = np.round(pos - 200 * fwd).astype(np.int32)
    side = np.round(pos + 40 * fwd + 400 * cam["right"][0]).astype(np.int32)
    off = np.array([IO.instance(i % len(models), behind + 17 * i, p, f) for i, (p, f) in enumerate(IO.SIGNED_PERMUTATIONS[:20])] +
                   [IO.instance(i % len(models), side + 13 * i) for i in range(10)], dtype=INSTANCE)
    n = w * h
    ref_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    ref_rgba = torch.zeros(n, dtype=torch.int32, device="cuda")
    tr.draw_frame_device(cam, ref_hits.data_ptr(), ref_rgba.data_ptr())
    dev_off = torch.from_numpy(off.view(np.uint8).copy()).cuda()
    for table_ptr, count in ((0, 0), (dev_off.data_ptr(), len(off))):
        hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        rgba = torch.zeros(n, dtype=torch.int32, device="cuda")
        ids = torch.zeros(n, dtype=torch.int32, device="cuda")
        tr.trace_primary_instanced_device(cam, table_ptr, count, hits.data_ptr(), rgba.data_ptr(), ids.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(hits, ref_hits) and torch.equal(rgba, ref_rgba)
        assert (ids.cpu().numpy().view(np.uint32) == INSTANCE_NONE).all()
        # RGBA8 alone and ids alone
        rgba2 = torch.zeros(n, dtype=torch.int32, device="cuda")
        tr.trace_primary_instanced_device(cam, table_ptr, count, 0, rgba2.data_ptr(), 0)
        ids2 = torch.zeros(n, dtype=torch.int32, device="cuda")
        tr.trace_primary_instanced_device(cam, table_ptr, count, 0, 0, ids2.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(rgba2, ref_rgba) and (ids2.cpu().numpy().view(np.uint32) == INSTANCE_NONE).all()
    tr.shutdown()


@pytest.mark.parametrize("scene", ["scene64", "scene256"])
def test_frames_equal_the_oracle_composition(request, torch_cuda, scene, models, oracle_models):
    cm, pw = request.getfixturevalue(scene)
    n = 64 if scene == "scene64" else 256
    w, h = 240, 176
    tr = make_tracer(pw, w, h, models)
    table = IO.random_instances(48, len(models), -6, n + 4, seed=n)
    # overlapping pairs and exact duplicates (ties between instances), instances sunk into the terrain
    extra = [table[3].copy(), table[5].copy()]
    extra[1]["offset"] = extra[1]["offset"] + 2
    extra += [IO.instance(0, (n // 3, 0, n // 3), (2, 0, 1), 5), IO.instance(1, (n // 2, 3, n // 2), (1, 2, 0), 3)]
    table = np.concatenate([table, np.array(extra, dtype=INSTANCE)])
    won_total = 0
    for pose in (0, 1, 2):
        cam = W.scene_camera(n, pose, w, h, SEED)
        _, want, ids = check_frame(tr, pw, cam, table, oracle_models)
        won_total += int((ids != INSTANCE_NONE).sum())
        check_frame(tr, pw, cam, table, oracle_models, rect=(37, 21, 150, 101))        # a sub-rectangle
    assert won_total > 1000
    # the camera inside an instance box, and an instance straddling the camera plane
    cam = camera_inside(table, 7, models, w, h)
    _, _, ids = check_frame(tr, pw, cam, table, oracle_models)
    cam = W.scene_camera(n, 0, w, h, SEED)
    pos, fwd, right = (cam[k][0].astype(np.float64) for k in ("pos", "fwd", "right"))
    beside = (np.round(pos + 8 * right + 2 * fwd) - (6, 4, 3)).astype(np.int32)        # its box reaches from behind the camera plane to in front
    corners = np.array([[beside[0] + (12 if c & 1 else 0), beside[1] + (9 if c & 2 else 0), beside[2] + (7 if c & 4 else 0)] for c in range(8)])
    depth = (corners - pos) @ fwd
    assert depth.min() < 0 < depth.max()
    straddle = np.concatenate([table, np.array([IO.instance(0, beside)], dtype=INSTANCE)])
    _, _, ids = check_frame(tr, pw, cam, straddle, oracle_models)
    assert (ids == len(straddle) - 1).sum() > 1000
    tr.shutdown()


def test_bin_overflow_stays_exact(torch_cuda, scene64, models, oracle_models):
    cm, pw = scene64
    w, h = 128, 96
    tr = make_tracer(pw, w, h, models)
    cam = W.scene_camera(64, 0, w, h, SEED)
    pos, fwd = cam["pos"][0].astype(np.float64), cam["fwd"][0].astype(np.float64)
    centre = np.round(pos + 40 * fwd).astype(np.int32)
    rng = np.random.default_rng(9)
    table = np.array([IO.instance(int(rng.integers(len(models))), centre + rng.integers(-6, 6, size=3), *IO.SIGNED_PERMUTATIONS[i % 48])
                      for i in range(150)], dtype=INSTANCE)                  # far more than a bin's 63 on the central tiles
    _, _, ids = check_frame(tr, pw, cam, table, oracle_models)
    assert len(np.unique(ids[ids != INSTANCE_NONE])) > 20
    tr.shutdown()


def test_rays_instanced(torch_cuda, scene64, models, oracle_models):
    cm, pw = scene64
    tr = make_tracer(pw, 64, 64, models)
    table = IO.random_instances(40, len(models), -4, 60, seed=21)
    rays = np.concatenate([edge_case_rays(), random_rays(64, 8000, 23)])
    world, _ = O.Lattice(pw.nodes, pw.sub_chunks).trace(rays, threads=8)
    want, want_ids = IO.compose(world, rays, table, oracle_models)
    hits, ids = tr.trace_rays_instanced(rays, table)
    assert records_equal(hits, want).all() and (ids == want_ids).all()
    assert (want_ids != INSTANCE_NONE).sum() > 300
    hits0, ids0 = tr.trace_rays_instanced(rays, table[:0])
    assert records_equal(hits0, world).all() and (ids0 == INSTANCE_NONE).all()
    tr.shutdown()


def test_voxel_size_half(torch_cuda, models):
    vs = 0.5
    rng = np.random.default_rng(5)
    cm = W.ChunkManager(128, vs)
    wall = np.array([(x, 0, z) for x in range(-40, 60) for z in range(-40, 60)], dtype=np.int32)
    pts = rng.integers(-40, 60, size=(2000, 3)).astype(np.int32)
    xyz = np.concatenate([wall, pts])
    cm.set_voxels(xyz, rng.integers(1, 60, size=len(xyz)).astype(np.uint32))
    cm.rebuild_dirty_chunks()
    pw = cm.pack_chunks_to_gpu_svo(W.scene_materials(SEED))
    omodels = [IO.OracleModel(x, m, vs) for x, m in models]
    w, h = 200, 150
    tr = make_tracer(pw, w, h, models, vs)
    table = IO.random_instances(30, len(models), -30, 50, seed=31)
    for cam in (W.camera_look_at((70.0 * vs, 50.0 * vs, -60.0 * vs), (10.0 * vs, 0.0, 10.0 * vs), 60.0, w, h),
                W.camera_look_at((3.3 * vs, 20.2 * vs, 7.7 * vs), (40.0 * vs, 0.0, 31.0 * vs), 95.0, w, h)):
        _, _, ids = check_frame(tr, pw, cam, table, omodels, voxel_size=vs)
        assert (ids != INSTANCE_NONE).sum() > 100
    tr.shutdown()


def test_two_streams_in_flight(torch_cuda, scene64, models, oracle_models):
    torch = torch_cuda
    cm, pw = scene64
    w, h = 192, 128
    tr = make_tracer(pw, w, h, models)
    cams = [W.scene_camera(64, 0, w, h, SEED), W.scene_camera(64, 2, w, h, SEED)]
    tables = [IO.random_instances(40, len(models), -4, 60, seed=41), IO.random_instances(25, len(models), 0, 64, seed=42)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    dev_tables = [torch.from_numpy(t.view(np.uint8).copy()).cuda() for t in tables]
    torch.cuda.synchronize()
    for k in range(2):
        hits = torch.zeros((w * h, 4), dtype=torch.int32, device="cuda")
        ids = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        rgba = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        outs.append((hits, ids, rgba))
    for rep in range(3):
        for k in range(2):
            hits, ids, rgba = outs[k]
            tr.trace_primary_instanced_device(cams[k], dev_tables[k].data_ptr(), len(tables[k]), hits.data_ptr(), rgba.data_ptr(),
                                              ids.data_ptr(), stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        _, want, want_ids = expected_frame(pw, cams[k], w, h, tables[k], oracle_models)
        hits, ids, rgba = outs[k]
        got = hits.cpu().numpy().view(O.HIT).reshape(-1)
        assert records_equal(got, want).all() and (ids.cpu().numpy().view(np.uint32) == want_ids).all()
        assert (rgba.cpu().numpy().view(np.uint32) == IO.shade(want, pw.materials)).all()
    for s in streams:
        tr._check(tr._lib.blok_hip_release_stream(tr._ctx, __import__("ctypes").c_void_p(s.cuda_stream)))
    tr.shutdown()


def test_errors_leave_the_context_usable(torch_cuda, scene64, models, oracle_models):
    from blok_amd._ffi import BlokError
    from blok_amd.tracer import HipTracer
    cm, pw = scene64
    w, h = 96, 64
    empty = HipTracer(w, h).init()
    m = empty.model_create(*models[0])
    cam = W.scene_camera(64, 0, w, h, SEED)
    with pytest.raises(BlokError) as e:
        empty.trace_primary_instanced(cam, np.array([IO.instance(m, (0, 0, 0))], dtype=INSTANCE))
    assert e.value.status == -4                              # no world
    empty.shutdown()
    tr = make_tracer(pw, w, h, models)
    good = IO.random_instances(10, len(models), 0, 60, seed=51)
    doomed = tr.model_create(*models[1])
    tr.model_destroy(doomed)
    bad_axis = IO.instance(0, (0, 0, 0), (0, 0, 1))
    bad_res = IO.instance(0, (0, 0, 0))
    bad_res["reserved"][2] = 7
    cases = [IO.instance(99, (0, 0, 0)), IO.instance(doomed, (0, 0, 0)), bad_axis, bad_res, IO.instance(0, (32765, 0, 0)),
             IO.instance(0, (0, -32768, 0), (0, 1, 2), 2)]
    rays = random_rays(64, 100, 1)
    for bad in cases:
        table = np.concatenate([good, np.array([bad], dtype=INSTANCE)])
        for call in (lambda: tr.trace_primary_instanced(cam, table), lambda: tr.trace_rays_instanced(rays, table),
                     lambda: tr.check_instances(table)):
            with pytest.raises(BlokError) as e:
                call()
            assert e.value.status == -1
    with pytest.raises(BlokError):
        tr.model_destroy(doomed)
    check_frame(tr, pw, cam, good, oracle_models)            # still usable
    tr.shutdown()
