"""GPU: posed models (include/blok_hip.h, "Posed models"; blok_hip_trace_primary_posed*, blok_hip_trace_rays_posed*) over the case table
of tests/pose_cases.py.

References: the oracle composition (tests/pose_oracle.py on top of tests/scaled_instance_oracle.py), the unbinned rays kernel for the
binned frame, the instanced entries for an empty pose table and for poses made from instances.  Every comparison is exact.  Frames are
96 x 64 (3 x 2 bins) and 100 x 70 at (8, 8) of a 116 x 86 frame (ragged tiles and bins).  Section 6 holds the small cases that the kernel body
shared with the lattice instances makes easy to break: an overflowing bin, a rectangle off every grid, ids alone, who writes which id."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from blok_amd import pose as P
from blok_amd._ffi import HIT, INSTANCE, INSTANCE_NONE, POSE, POSE_ID, BlokError
from tests import instance_oracle as IO
from tests import oracle_ffi as O
from tests import pose_cases as PC
from tests import pose_oracle as PO
from tests import scaled_instance_oracle as SO
from tests.conftest import records_equal

pytestmark = pytest.mark.gpu

VOXEL_SIZES = [1.0, 0.5]
BLOK_ERR_INVALID_ARG = -1
N_CASES = len(PC.table(1.0))


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
    """Per voxel size: the 96 x 64 tracer and the 116 x 86 one, with the case table's models."""
    out = {vs: (make_tracer(vs), make_tracer(vs, *PC.BIG)) for vs in VOXEL_SIZES}
    yield out
    for pair in out.values():
        for tr in pair:
            tr.shutdown()


@functools.lru_cache(maxsize=None)
def oracle_models(vs):
    return tuple(PC.oracle_models(vs))


def frame_rays(case, full):
    """The primary rays of the frame's pixels, row major: the whole 96 x 64 frame, or the rectangle of the larger one."""
    if full:
        return O.primary_rays(case.camera(PC.WD, PC.HT), PC.WD, PC.HT)
    w, h = PC.BIG
    x0, y0, rw, rh = PC.RECT
    return O.primary_rays(case.camera(w, h), w, h).reshape(h, w)[y0:y0 + rh, x0:x0 + rw].reshape(-1).copy()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() if len(a) else torch.zeros(1, dtype=torch.uint8, device="cuda")


def assert_same(got, ids, want, want_ids, what):
    bad = np.flatnonzero(~records_equal(got, want) | (ids != want_ids))
    assert bad.size == 0, f"{what}: {bad.size} differ; first {bad[:4]}: got {got[bad[:2]]} {ids[bad[:2]]}, want {want[bad[:2]]} {want_ids[bad[:2]]}"


# ---- 1. oracle parity and conservative bins, every case ------------------------------------------------------------------------------------
@pytest.mark.parametrize("vs", VOXEL_SIZES)
@pytest.mark.parametrize("n", list(range(N_CASES)) + ["corner"])
def test_frames_and_rays_equal_the_oracle_and_the_bins_lose_nothing(torch_cuda, tracers, n, vs):
    torch = torch_cuda
    case = PC.corner_case(vs) if n == "corner" else PC.table(vs)[n]
    materials = PC.world(vs).materials
    for full, tr in zip((True, False), tracers[vs]):
        rect = None if full else PC.RECT
        w, h = (PC.WD, PC.HT) if full else PC.RECT[2:]
        cam = case.camera(tr.width, tr.height)
        rays = frame_rays(case, full)
        want, want_ids = PC.expected(case, vs, rays, oracle_models(vs))
        # the host entry
        hits, ids, rgba = tr.trace_primary_posed(cam, case.instances, case.poses, rect)
        assert_same(hits.reshape(-1), ids.reshape(-1), want, want_ids, f"{case.name} at vs {vs}, frame {w} x {h}")
        assert (rgba.reshape(-1) == PO.shade(want, want_ids, case.poses, materials)).all()
        # the bins are conservative: the unbinned rays kernel over the same pixels' rays gives the same bytes
        ray_hits, ray_ids = tr.trace_rays_posed(rays, case.instances, case.poses)
        assert ray_hits.tobytes() == hits.tobytes() and ray_ids.tobytes() == ids.tobytes()
        # the device entries: the same bytes
        d_inst, d_pose, d_rays = dev(torch, case.instances), dev(torch, case.poses), dev(torch, rays)
        d_hits = torch.zeros(w * h * 16, dtype=torch.uint8, device="cuda")
        d_rgba = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        d_ids = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        tr.trace_primary_posed_device(cam, d_inst.data_ptr(), len(case.instances), d_pose.data_ptr(), len(case.poses), d_hits.data_ptr(),
                                      d_rgba.data_ptr(), d_ids.data_ptr(), rect)
        torch.cuda.synchronize()
        assert d_hits.cpu().numpy().tobytes() == hits.tobytes() and d_ids.cpu().numpy().tobytes() == ids.tobytes()
        assert d_rgba.cpu().numpy().tobytes() == rgba.tobytes()
        d_hits.zero_(); d_ids.zero_()
        tr.trace_rays_posed_device(d_rays.data_ptr(), len(rays), d_inst.data_ptr(), len(case.instances), d_pose.data_ptr(), len(case.poses),
                                   d_hits.data_ptr(), d_ids.data_ptr())
        torch.cuda.synchronize()
        assert d_hits.cpu().numpy().tobytes() == hits.tobytes() and d_ids.cpu().numpy().tobytes() == ids.tobytes()
        # ids alone (the records go to the context's scratch)
        d_ids.zero_()
        tr.trace_primary_posed_device(cam, d_inst.data_ptr(), len(case.instances), d_pose.data_ptr(), len(case.poses), 0, 0, d_ids.data_ptr(), rect)
        torch.cuda.synchronize()
        assert d_ids.cpu().numpy().tobytes() == ids.tobytes()
    # aimed rays: hits from every side, not only the camera's
    rays = PC.aimed_rays(case, vs, per_entry=max(20, 1500 // max(1, len(case.poses) + len(case.instances))), n_miss=100, seed=70)
    want, want_ids = PC.expected(case, vs, rays, oracle_models(vs))
    hits, ids = tracers[vs][0].trace_rays_posed(rays, case.instances, case.poses)
    assert_same(hits, ids, want, want_ids, f"aimed rays of {case.name} at vs {vs}")


# ---- 2. an empty pose table is the instanced entry --------------------------------------------------------------------------------------------
def test_no_poses_gives_the_bytes_of_the_instanced_entries(torch_cuda, tracers):
    tr = tracers[1.0][0]
    case = PC.table(1.0)[11]                                   # the mixed case's instances
    cam = case.camera(PC.WD, PC.HT)
    for inst in (case.instances, case.instances[:0]):
        a = tr.trace_primary_instanced(cam, inst)
        b = tr.trace_primary_posed(cam, inst, None)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        rays = PC.aimed_rays(case, 1.0, 200, 50, 5)
        a = tr.trace_rays_instanced(rays, inst)
        b = tr.trace_rays_posed(rays, inst, None)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert (tr.trace_primary_instanced(cam, case.instances)[1] == 0).any()


# ---- 3. the 48 orientations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vs", VOXEL_SIZES)
def test_poses_from_instances_equal_the_instanced_entry(torch_cuda, tracers, vs):
    tr = tracers[vs][0]
    rng = np.random.default_rng(9)
    table = np.array([IO.instance(i % 5, rng.integers(-30, 50, size=3) + (0, 25, 0), p, f) for i, (p, f) in enumerate(IO.SIGNED_PERMUTATIONS)], dtype=INSTANCE)
    poses = np.concatenate([P.from_instance(inst, vs) for inst in table])
    tr.check_instances(table)
    tr.check_poses(poses)
    cam = PC.W.camera_look_at((90.0 * vs, 90.0 * vs, -70.0 * vs), (10.0 * vs, 25.0 * vs, 10.0 * vs), 60.0, PC.WD, PC.HT)
    a, a_ids, _ = tr.trace_primary_instanced(cam, table)
    b, b_ids, _ = tr.trace_primary_posed(cam, None, poses)
    a, a_ids, b, b_ids = a.reshape(-1), a_ids.reshape(-1), b.reshape(-1), b_ids.reshape(-1)
    for k in ("t", "material_id", "hit"):
        assert a[k].tobytes() == b[k].tobytes(), k
    won = a_ids != INSTANCE_NONE
    assert won.sum() > 500 and len(np.unique(a_ids[won])) > 20
    assert ((b_ids == INSTANCE_NONE) == ~won).all() and (b_ids[won] == (POSE_ID | a_ids[won])).all()
    for j in np.unique(a_ids[won]):
        sel = np.flatnonzero(a_ids == j)
        back = SO.world_records(b[sel], table[j], PC.EXPONENTS[int(table[j]["model"])])
        assert records_equal(back, a[sel]).all(), j


# ---- 4. streams, and a table changed between frames without a host synchronise ------------------------------------------------------------------
def test_two_streams_and_a_table_changed_in_stream_order(torch_cuda, tracers):
    torch = torch_cuda
    tr = tracers[1.0][0]
    first, second = PC.table(1.0)[0], PC.table(1.0)[1]
    cam = first.camera(PC.WD, PC.HT)
    want = {}
    for name, case in (("first", first), ("second", second)):
        hits, ids, rgba = tr.trace_primary_posed(cam, None, case.poses)
        want[name] = (hits.tobytes(), ids.tobytes(), rgba.tobytes())
    assert want["first"] != want["second"]
    n = PC.WD * PC.HT
    staged = {name: dev(torch, case.poses) for name, case in (("first", first), ("second", second))}
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            table = staged["first"].clone()
            outs = []
            for name in ("first", "second"):
                hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
                ids = torch.zeros(n, dtype=torch.int32, device="cuda")
                rgba = torch.zeros(n, dtype=torch.int32, device="cuda")
                table.copy_(staged[name], non_blocking=True)                   # the same device table, rewritten in stream order
                tr.trace_primary_posed_device(cam, 0, 0, table.data_ptr(), 1, hits.data_ptr(), rgba.data_ptr(), ids.data_ptr(), stream=stream.cuda_stream)
                outs.append((name, hits, ids, rgba))
        stream.synchronize()
        for name, hits, ids, rgba in outs:
            assert (hits.cpu().numpy().tobytes(), ids.cpu().numpy().tobytes(), rgba.cpu().numpy().tobytes()) == want[name], name
        tr.release_stream(stream.cuda_stream)


# ---- 5. the error table, outputs untouched ---------------------------------------------------------------------------------------------------
def test_errors_name_the_first_bad_pose_and_touch_nothing(torch_cuda, tracers):
    tr = tracers[1.0][0]
    lib, ctx = tr._lib, tr._ctx
    from blok_amd import _ffi
    good = PC.table(1.0)[0].poses[0]
    cam = PC.table(1.0)[0].camera(PC.WD, PC.HT)
    rays = np.ascontiguousarray(PC.aimed_rays(PC.table(1.0)[0], 1.0, 50, 0, 1))
    bad = []
    for field, at, value, text in (("m", (1, 2), np.nan, "not finite"), ("pivot", (0,), np.inf, "not finite"), ("local", (2,), -np.inf, "not finite"),
                                   ("m", (0, 0), 1025.0, "1024"), ("pivot", (1,), -2.0 ** 20 - 1.0, "pivot"), ("local", (0,), 2.0 ** 21, "local")):
        p = good.copy()
        p[field][at] = value
        bad.append((p, text))
    p = good.copy()
    p["model"] = 99
    bad.append((p, "unknown model 99"))
    for p, text in bad:
        table = np.array([good, good, p, p], dtype=POSE)
        n = PC.WD * PC.HT
        hits, ids, rgba = np.zeros(n, dtype=HIT), np.full(n, 7, dtype=np.uint32), np.full(n, 7, dtype=np.uint32)
        rhits, rids = np.zeros(len(rays), dtype=HIT), np.full(len(rays), 7, dtype=np.uint32)
        hits.view(np.uint8)[:] = 7
        rhits.view(np.uint8)[:] = 7
        before = [out.tobytes() for out in (hits, ids, rgba, rhits, rids)]
        calls = (lambda: lib.blok_hip_check_poses(ctx, _ffi.ptr(table), 4),
                 lambda: lib.blok_hip_trace_primary_posed(ctx, _ffi.ptr(np.ascontiguousarray(cam)), 0, 0, PC.WD, PC.HT, None, 0, _ffi.ptr(table), 4, _ffi.ptr(hits), _ffi.ptr(rgba), _ffi.ptr(ids)),
                 lambda: lib.blok_hip_trace_rays_posed(ctx, _ffi.ptr(rays), len(rays), None, 0, _ffi.ptr(table), 4, _ffi.ptr(rhits), _ffi.ptr(rids)))
        for call in calls:
            assert call() == BLOK_ERR_INVALID_ARG
            message = lib.blok_hip_last_error(ctx).decode()
            assert "pose 2:" in message and text in message, message
        assert [out.tobytes() for out in (hits, ids, rgba, rhits, rids)] == before
    with pytest.raises(BlokError) as e:
        tr.check_poses(np.array([good, bad[0][0]], dtype=POSE))
    assert e.value.status == BLOK_ERR_INVALID_ARG and "pose 1:" in str(e.value)
    # a null table with a count, and a bad instance beside good poses
    assert lib.blok_hip_check_poses(ctx, None, 3) == BLOK_ERR_INVALID_ARG
    with pytest.raises(BlokError) as e:
        tr.trace_primary_posed(cam, np.array([IO.instance(99, (0, 0, 0))], dtype=INSTANCE), np.array([good], dtype=POSE))
    assert "instance 0:" in str(e.value)
    tr.check_poses(np.array([good], dtype=POSE))


def test_device_tables_skip_what_the_host_check_refuses(torch_cuda, tracers):
    """A pose with a NaN, one of an unknown model and one beyond a bound, between good ones in a device table: the frame is the frame of the
    good ones alone, with their indices."""
    torch = torch_cuda
    tr = tracers[1.0][0]
    case = PC.table(1.0)[0]
    good = case.poses[0]
    nan, unknown, far = good.copy(), good.copy(), good.copy()
    nan["m"][0, 0] = np.nan
    unknown["model"] = 1000
    far["pivot"][2] = 2.0 ** 21
    table = np.array([nan, unknown, far, good], dtype=POSE)
    cam = case.camera(PC.WD, PC.HT)
    want_hits, want_ids, _ = tr.trace_primary_posed(cam, None, case.poses)
    n = PC.WD * PC.HT
    d_hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_table = dev(torch, table)
    tr.trace_primary_posed_device(cam, 0, 0, d_table.data_ptr(), 4, d_hits.data_ptr(), 0, d_ids.data_ptr())
    torch.cuda.synchronize()
    ids = d_ids.cpu().numpy().view(np.uint32)
    won = want_ids.reshape(-1) == POSE_ID
    assert won.sum() > 300 and d_hits.cpu().numpy().tobytes() == want_hits.tobytes()
    assert (ids[won] == POSE_ID | 3).all() and (ids[~won] == want_ids.reshape(-1)[~won]).all()


# ---- 6. what one kernel body for lattice instances and poses makes easy to break (placed_kernels.hip) ------------------------------------------
def test_more_poses_than_a_bin_lists_stay_exact(torch_cuda, tracers):
    """70 small rods whose boxes fall into bin (1, 0) of the 96 x 64 frame: the bin overflows (its pixels test every pose), and the frame is
    the unbinned rays kernel's and the oracle's, byte for byte."""
    tr = tracers[1.0][0]
    case = next(c for c in PC.table(1.0) if c.notes.get("overflow"))
    assert len(case.poses) == 70
    cam = case.camera(PC.WD, PC.HT)
    rays = frame_rays(case, True)
    per_pose = []
    want, want_ids = PC.expected(case, 1.0, rays, oracle_models(1.0), per_pose)
    x, y = np.meshgrid(np.arange(PC.WD), np.arange(PC.HT))
    in_bin = ((x // 32 == 1) & (y // 32 == 0)).reshape(-1)
    assert sum(1 for hit in per_pose if (hit & in_bin).any()) > 63, "more poses in the bin than its list holds"
    hits, ids, rgba = tr.trace_primary_posed(cam, None, case.poses)
    assert_same(hits.reshape(-1), ids.reshape(-1), want, want_ids, "the overflowing bin's frame")
    assert (rgba.reshape(-1) == PO.shade(want, want_ids, case.poses, PC.world(1.0).materials)).all()
    ray_hits, ray_ids = tr.trace_rays_posed(rays, None, case.poses)
    assert ray_hits.tobytes() == hits.tobytes() and ray_ids.tobytes() == ids.tobytes()
    assert len(np.unique(ids[(ids != INSTANCE_NONE)])) > 20 and (ids[ids != INSTANCE_NONE] & POSE_ID).all()


@pytest.mark.parametrize("n", [0, 11])                         # one pose; lattice instances and poses together
def test_a_rectangle_off_every_grid_is_the_full_frames_crop(torch_cuda, tracers, n):
    """A rectangle whose origin and size are multiples of neither the 8 x 8 tile nor the 32 x 32 bin: records, ids and RGBA8 are the crop of
    the full frame's."""
    tr = tracers[1.0][0]
    case = PC.table(1.0)[n]
    cam = case.camera(PC.WD, PC.HT)
    x0, y0, w, h = rect = (13, 9, 53, 37)
    full = tr.trace_primary_posed(cam, case.instances, case.poses)
    part = tr.trace_primary_posed(cam, case.instances, case.poses, rect)
    for whole, crop in zip(full, part):
        assert crop.shape == (h, w) and crop.tobytes() == np.ascontiguousarray(whole[y0:y0 + h, x0:x0 + w]).tobytes()
    assert (part[1] != INSTANCE_NONE).sum() > 100 and (part[1] == INSTANCE_NONE).any()


def test_ids_alone_with_poses_and_no_instances(torch_cuda, tracers):
    """Only the id plane is asked for, the lattice table is empty and the pose table is not: the records go to the stream's scratch, and
    the ids are those of the run with all three outputs."""
    torch = torch_cuda
    tr = tracers[1.0][0]
    case = PC.table(1.0)[1]
    cam = case.camera(PC.WD, PC.HT)
    _, want_ids, _ = tr.trace_primary_posed(cam, None, case.poses)
    d_pose = dev(torch, case.poses)
    d_ids = torch.full((PC.WD * PC.HT,), 7, dtype=torch.int32, device="cuda")
    tr.trace_primary_posed_device(cam, 0, 0, d_pose.data_ptr(), len(case.poses), 0, 0, d_ids.data_ptr())
    torch.cuda.synchronize()
    ids = d_ids.cpu().numpy().view(np.uint32)
    assert ((ids == INSTANCE_NONE) | (ids == POSE_ID | 0)).all() and (ids == POSE_ID | 0).sum() > 300
    assert ids.tobytes() == want_ids.tobytes()


def pixel_box(cam, corners, w, h):
    """(x0, x1, y0, y1) of the pixels that world points `corners` (all in front of the camera) project to: camera_plane_uv inverted."""
    pos, fwd, right, up = (np.asarray(cam[k], dtype=np.float64).reshape(3) for k in ("pos", "fwd", "right", "up"))
    d = np.asarray(corners, dtype=np.float64) - pos
    depth = d @ fwd
    assert (depth > 1.0).all()
    tan, aspect = float(np.ravel(cam["tan_half_fov"])[0]), float(np.ravel(cam["aspect"])[0])
    x = ((d @ right) / depth / (tan * aspect) + 1.0) * 0.5 * w - 0.5
    y = (1.0 - (d @ up) / depth / tan) * 0.5 * h - 0.5
    return x.min(), x.max(), y.min(), y.max()


def test_each_pass_writes_only_the_ids_it_owns(torch_cuda, tracers):
    """A lattice instance in the right third of the frame, a pose in the left third, nothing in the middle.  The lattice pass owns the id
    plane: it writes every pixel, also of a tile its bin leaves empty.  The posed pass writes only where a pose wins: the tiles that only the
    instance bin lists keep the instance's ids, the tiles neither bin lists are 0xFFFFFFFF."""
    torch = torch_cuda
    vs = 1.0
    tr = tracers[vs][0]
    inst = IO.instance(PC.ROD, (-8, 14, 18), (1, 0, 2), 2)
    p = PC.turned(PC.SLAB, vs, (35.0, 16.0, 18.0), yaw=30.0)
    case = PC.Case("own", np.array([inst], dtype=INSTANCE), np.array([p], dtype=POSE), (10.0, 22.0, -25.0), (10.0, 14.0, 15.0))
    cam = case.camera(PC.WD, PC.HT)
    # which bins list what, from the boxes alone: each box's pixels, 2 pixels wider than the bins' own margin, lie in one column of bins
    bx = PC.boxes()
    box = lambda lo, hi: [[float((hi if c >> k & 1 else lo)[k]) for k in range(3)] for c in range(8)]
    lo, hi = SO.world_span(inst, bx[PC.ROD][0], bx[PC.ROD][1], PC.EXPONENTS[PC.ROD])
    ix0, ix1, _, _ = pixel_box(cam, np.array(box(lo, hi)) * vs, PC.WD, PC.HT)
    px0, px1, _, _ = pixel_box(cam, box(*PO.preimage_box(p, bx[PC.SLAB][0], bx[PC.SLAB][1], vs)), PC.WD, PC.HT)
    assert 64 + 3 <= ix0 and ix1 <= 95 - 3 and px1 <= 31 - 3, (ix0, ix1, px0, px1)
    want, want_ids = PC.expected(case, vs, frame_rays(case, True), oracle_models(vs))
    _, inst_ids, _ = tr.trace_primary_instanced(cam, case.instances)
    n = PC.WD * PC.HT
    d_hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_ids = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    d_inst, d_pose = dev(torch, case.instances), dev(torch, case.poses)
    tr.trace_primary_posed_device(cam, d_inst.data_ptr(), 1, d_pose.data_ptr(), 1, d_hits.data_ptr(), 0, d_ids.data_ptr())
    torch.cuda.synchronize()
    ids = d_ids.cpu().numpy().view(np.uint32).reshape(PC.HT, PC.WD)
    assert_same(d_hits.cpu().numpy().view(HIT), ids.reshape(-1), want, want_ids, "one instance, one pose")
    assert (ids[:, 64:] == inst_ids[:, 64:]).all() and (ids[:, 64:] == 0).sum() > 15 and ((ids[:, 64:] == 0) | (ids[:, 64:] == INSTANCE_NONE)).all()
    assert (ids[:, 32:64] == INSTANCE_NONE).all()
    assert (ids[:, :32] == POSE_ID | 0).sum() > 100 and ((ids[:, :32] == POSE_ID | 0) | (ids[:, :32] == INSTANCE_NONE)).all()


def test_abi_version(torch_cuda):
    from blok_amd import _ffi
    assert _ffi.hip_lib().blok_hip_abi_version() >= (1 << 16) | 22
