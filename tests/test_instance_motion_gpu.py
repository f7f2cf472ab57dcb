"""GPU: object motion of moving instances (blok_hip_instance_motion_device, blok_hip_denoise_instanced_ref_device,
blok_hip_draw_frame_rt_instanced_motion).

References: numpy's object motion from the path kernel's own world-position, id and table data (tests/test_instance_motion_cpu.py restates
the map), the non-motion entries (an unmoved table: the same bits), and the passes called one by one."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import world as W
from blok_amd._ffi import INSTANCE, INSTANCE_NONE, BlokError
from tests import instance_oracle as IO
from tests.test_instance_motion_cpu import numpy_map

pytestmark = pytest.mark.gpu

WD, HT = 128, 96


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def plate(nx=16, ny=2, nz=16, material=3):
    xyz = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    return xyz, np.full(len(xyz), material, dtype=np.uint32)


MODELS = [plate(), plate(3, 3, 3, 5), plate()]                 # model 2: the same voxels as model 0 under another id


def tracer(pw, models=MODELS, w=WD, h=HT):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(w, h).init()
    tr.add_world(pw)
    assert [tr.model_create(xyz, mats) for xyz, mats in models] == list(range(len(models)))
    return tr


def top_camera(w=WD, h=HT):
    return W.camera_look_at((44.0, 130.0, 20.0), (44.0, 10.0, 46.0), 70.0, w, h)


def dev_table(torch, table):
    return torch.from_numpy(np.ascontiguousarray(table, dtype=INSTANCE).view(np.uint8).copy()).cuda()


def object_motion(world_pos, ids, cur, prev, prev_vp, vs=1.0, x0=0, y0=0, frame_w=WD, frame_h=HT):
    """(tracked mask, float32 motion (h, w, 2)) restated in numpy: cu - project_prev(prev_view_proj, p_prev), post_core.h's operations."""
    h, w = ids.shape
    tracked = np.zeros((h, w), bool)
    mo = np.zeros((h, w, 2), np.float32)
    M = np.asarray(prev_vp, np.float32)
    f32 = np.float32
    for i in np.unique(ids[ids != INSTANCE_NONE]):
        i = int(i)
        if i >= len(prev) or int(prev[i]["model"]) != int(cur[i]["model"]):
            continue
        sel = ids == i
        p = world_pos[sel][:, :3].astype(np.float32)
        q, _ = numpy_map(cur[i], prev[i], vs, p, np.zeros_like(p))
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        cx = ((M[0] * x + M[4] * y) + M[8] * z) + M[12]
        cy = ((M[1] * x + M[5] * y) + M[9] * z) + M[13]
        cw = ((M[3] * x + M[7] * y) + M[11] * z) + M[15]
        pu, pv = (cx / cw) * f32(0.5) + f32(0.5), (cy / cw) * f32(0.5) + f32(0.5)
        yy, xx = np.nonzero(sel)
        cu = ((xx + x0).astype(np.float32) + f32(0.5)) / f32(frame_w)
        cv = ((yy + y0).astype(np.float32) + f32(0.5)) / f32(frame_h)
        mo[sel, 0] = cu - pu
        mo[sel, 1] = cv - pv
        tracked |= sel
    return tracked, mo


def ref_planes(torch, n):
    return dict(color=torch.zeros((n, 4), dtype=torch.float32, device="cuda"), world_pos=torch.zeros((n, 4), dtype=torch.float32, device="cuda"),
                nr=torch.zeros((n, 4), dtype=torch.int16, device="cuda"), alb=torch.zeros(n, dtype=torch.int32, device="cuda"),
                motion=torch.zeros((n, 2), dtype=torch.int16, device="cuda"), ids=torch.zeros(n, dtype=torch.int32, device="cuda"))


def trace_ref(tr, cam, P, table_dev, n_inst, prev_vp, frame, spp=2, rect=None, stream=0):
    tr.trace_paths_instanced_ref_device(cam, table_dev.data_ptr() if n_inst else 0, n_inst, P["color"].data_ptr(), P["world_pos"].data_ptr(),
                                        P["nr"].data_ptr(), P["alb"].data_ptr(), P["motion"].data_ptr(), prev_vp, P["ids"].data_ptr(),
                                        spp=spp, max_bounces=2, frame_index=frame, rect=rect, stream=stream)


def moved_tables():
    # two plates above the terrain (its top is below y = 60)
    prev = np.array([IO.instance(0, (36, 70, 36)), IO.instance(0, (6, 66, 44))], dtype=INSTANCE)
    cur = prev.copy()
    cur[0]["offset"] = (39, 72, 35)                              # translated
    cur[1] = IO.instance(0, (22, 66, 60), (2, 1, 0), 5)          # turned half a turn in place: the same box, every point elsewhere
    return cur, prev


# ------------------------------------------------------------------------------------------------ the motion kernel
@pytest.mark.parametrize("rect", [None, (16, 8, 96, 72)])
def test_instance_motion_kernel_equals_numpy(torch_cuda, scene64, rect):
    torch = torch_cuda
    _, pw = scene64
    tr = tracer(pw)
    x0, y0, w, h = rect if rect is not None else (0, 0, WD, HT)
    n = w * h
    cam, prev_cam = top_camera(), W.camera_look_at((45.0, 129.0, 21.0), (44.0, 10.0, 46.0), 70.0, WD, HT)
    prev_vp = tr.camera_view_proj(prev_cam)
    cur, prev = moved_tables()
    tc, tp = dev_table(torch, cur), dev_table(torch, prev)
    P = ref_planes(torch, n)
    trace_ref(tr, cam, P, tc, len(cur), prev_vp, 1, rect=rect)
    torch.cuda.synchronize()
    before = P["motion"].cpu().numpy().copy()
    m2 = torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda")
    tr.instance_motion_device(P["world_pos"].data_ptr(), P["ids"].data_ptr(), tc.data_ptr(), len(cur), tp.data_ptr(), len(prev), prev_vp,
                              motion_h_ptr=P["motion"].data_ptr(), motion_ptr=m2.data_ptr(), rect=rect)
    torch.cuda.synchronize()
    ids = P["ids"].cpu().numpy().view(np.uint32).reshape(h, w)
    wp = P["world_pos"].cpu().numpy().reshape(h, w, 4)
    tracked, want = object_motion(wp, ids, cur, prev, prev_vp, x0=x0, y0=y0)
    assert tracked.sum() > 200 and set(np.unique(ids[tracked]).tolist()) == {0, 1}
    got_h = P["motion"].cpu().numpy().view(np.uint16).reshape(h, w, 2)
    got_f = m2.cpu().numpy().reshape(h, w, 2)
    assert np.array_equal(got_h[tracked], want[tracked].astype(np.float16).view(np.uint16))
    assert got_f[tracked].tobytes() == want[tracked].tobytes()
    assert (np.abs(got_f[tracked]) > 1e-4).any()
    assert got_h[~tracked].tobytes() == before.view(np.uint16).reshape(h, w, 2)[~tracked].tobytes()
    assert (got_f[~tracked] == -7.0).all()
    tr.shutdown()


# ------------------------------------------------------------------------------------------------ the frame entry
def camera_path(k):
    return W.camera_look_at((44.0 + 0.7 * k, 130.0 - 0.5 * k, 20.0 + 0.4 * k), (44.0, 10.0, 46.0), 70.0, WD, HT)


def test_unmoved_table_is_the_non_motion_frame_and_no_instances_the_world_frame(torch_cuda, scene64):
    _, pw = scene64
    cur, _ = moved_tables()
    a, b = tracer(pw), tracer(pw)
    for k in range(6):
        got, fa = a.draw_frame_rt_instanced_motion(camera_path(k), cur, spp=2)
        want, fb = b.draw_frame_rt_instanced(camera_path(k), cur, spp=2)
        assert fa == fb == k + 1
        assert got.tobytes() == want.tobytes(), k
        for x, y in zip(a.denoise_state(), b.denoise_state()):
            assert x.tobytes() == y.tobytes(), k
    a.post_reset(); b.post_reset()
    empty = np.zeros(0, dtype=INSTANCE)
    for k in range(3):
        got, _ = a.draw_frame_rt_instanced_motion(camera_path(k), empty, spp=2)
        want, _ = b.draw_frame_rt(camera_path(k), spp=2)
        assert got.tobytes() == want.tobytes(), k
        for x, y in zip(a.denoise_state(), b.denoise_state()):
            assert x.tobytes() == y.tobytes(), k
    a.shutdown(); b.shutdown()


def moving_table(k):
    return np.array([IO.instance(0, (30 + 3 * k, 62 + 3 * k, 36)), IO.instance(1, (20, 80, 60 - 2 * k))], dtype=INSTANCE)


def test_entry_is_the_composition_of_the_passes(torch_cuda, scene64):
    torch = torch_cuda
    _, pw = scene64
    one, many = tracer(pw), tracer(pw)
    n = WD * HT
    P = ref_planes(torch, n)
    den = torch.zeros((n, 4), dtype=torch.float32, device="cuda"); taa = torch.zeros_like(den)
    ldr = torch.zeros(n, dtype=torch.int32, device="cuda"); sharp = torch.zeros_like(ldr)
    prev_dev, n_prev = None, 0
    for k in range(5):
        cam = camera_path(k)
        table = moving_table(k)
        got, frames = one.draw_frame_rt_instanced_motion(cam, table, spp=2)
        assert frames == k + 1
        cur_dev = dev_table(torch, table)
        prev_vp = many.camera_view_proj(camera_path(max(k - 1, 0)))
        many.set_taa_jitter(W.taa_jitter(k))
        trace_ref(many, cam, P, cur_dev, len(table), prev_vp, k)
        many.set_taa_jitter(None)
        many.instance_motion_device(P["world_pos"].data_ptr(), P["ids"].data_ptr(), cur_dev.data_ptr(), len(table),
                                    prev_dev.data_ptr() if n_prev else 0, n_prev, prev_vp, motion_h_ptr=P["motion"].data_ptr())
        many.denoise_instanced_ref_device(P["color"].data_ptr(), P["world_pos"].data_ptr(), P["nr"].data_ptr(), P["motion"].data_ptr(), prev_vp, k,
                                          den.data_ptr(), P["ids"].data_ptr(), cur_dev.data_ptr(), len(table),
                                          prev_dev.data_ptr() if n_prev else 0, n_prev)
        many.taa_device(den.data_ptr(), taa.data_ptr(), k)
        many.tonemap_device(taa.data_ptr(), ldr.data_ptr())
        many.sharpen_device(ldr.data_ptr(), sharp.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(got.reshape(-1), sharp.cpu().numpy().view(np.uint32)), k
        for x, y in zip(one.denoise_state(), many.denoise_state()):
            assert x.tobytes() == y.tobytes(), k
        prev_dev, n_prev = cur_dev, len(table)
    one.shutdown(); many.shutdown()


def erode(mask, r):
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out &= np.roll(np.roll(mask, dy, 0), dx, 1)
    out[:r] = out[-r:] = False
    out[:, :r] = out[:, -r:] = False
    return out


def run_sequence(tr, tables, cam, motion):
    """Draw the frames; per frame the id footprint of the plate (instance 0) and the denoiser's state."""
    out = []
    for t in tables:
        if motion:
            tr.draw_frame_rt_instanced_motion(cam, t, spp=2)
        else:
            tr.draw_frame_rt_instanced(cam, t, spp=2)
        _, ids, _ = tr.trace_primary_instanced(cam, t)
        out.append((ids == 0, tr.denoise_state()))
    return out


@pytest.mark.parametrize("kind", ["rising", "turning"])
def test_a_moving_plate_accumulates_history(torch_cuda, scene64, kind):
    """The behaviour the feature exists for: a camera at rest, a plate moving 3 voxels per frame (or turned 90 degrees in place every
    frame) for 8 frames.  With object motion its pixels keep accumulating; camera-only motion rejects the history of a moving plate."""
    _, pw = scene64
    cam = top_camera()
    if kind == "rising":
        tables = [np.array([IO.instance(0, (30 + 3 * k, 62 + 3 * k, 36))], dtype=INSTANCE) for k in range(8)]
    else:
        # a 16 x 16 plate turned about the vertical through its centre: the same box, every local point elsewhere
        tables = [np.array([IO.instance(0, (36, 62, 36)) if k % 2 == 0 else IO.instance(0, (36, 62, 52), (2, 1, 0), 1)], dtype=INSTANCE)
                  for k in range(8)]
    tr = tracer(pw)
    new = run_sequence(tr, tables, cam, True)
    inside = erode(new[-1][0], 2) & erode(new[-2][0], 2)
    assert inside.sum() > 100
    hist = new[-1][1][2]
    assert (hist[inside] >= 6).all(), np.unique(hist[inside])
    # its motion output is the object motion (the exact value: test_instance_motion_kernel_equals_numpy); a turn moves points off the centre
    mo = new[-1][1][4]
    assert (np.abs(mo[inside]).max(axis=-1) > 1e-3).mean() > 0.5
    if kind == "rising":
        tr.post_reset()
        old = run_sequence(tr, tables, cam, False)
        assert (old[-1][1][2][inside] == 1).all()
    tr.shutdown()


def test_untracked_instances_start_without_history(torch_cuda, scene64):
    _, pw = scene64
    cam = top_camera()
    base = IO.instance(0, (36, 62, 36))
    block = IO.instance(0, (54, 64, 40))                                                 # a second plate
    tables = [np.array([base], INSTANCE)] * 3 + [np.array([base, block], INSTANCE)]      # the block appears at frame 3
    swapped = base.copy(); swapped["model"] = 2                                           # the plate changes model at frame 4
    tables.append(np.array([swapped, block], INSTANCE))
    tr = tracer(pw)
    for k, t in enumerate(tables):
        tr.draw_frame_rt_instanced_motion(cam, t, spp=2)
        _, ids, _ = tr.trace_primary_instanced(cam, t)
        hist = tr.denoise_state()[2]
        plate_px, block_px = erode(ids == 0, 2), erode(ids == 1, 2)
        assert plate_px.sum() > 100
        if k == 3:
            assert block_px.sum() > 50 and (hist[block_px] == 1).all()
            assert (hist[plate_px] >= 3).all()
        if k == 4:
            assert (hist[plate_px] == 1).all()
            assert (hist[block_px] == 2).all()
    tr.shutdown()


# ------------------------------------------------------------------------------------------------ errors, streams
def test_errors(torch_cuda, scene64):
    torch = torch_cuda
    _, pw = scene64
    tr = tracer(pw)
    cur, prev = moved_tables()
    tc, tp = dev_table(torch, cur), dev_table(torch, prev)
    P = ref_planes(torch, WD * HT)
    vp = tr.camera_view_proj(top_camera())
    wp, ids, mh = P["world_pos"].data_ptr(), P["ids"].data_ptr(), P["motion"].data_ptr()
    bad = [dict(ids=0), dict(cur=0), dict(prev=0), dict(mh=0), dict(rect=(0, 0, WD + 1, HT)), dict(rect=(WD - 8, 0, 16, 8)), dict(vp=None)]
    for b in bad:
        a = dict(ids=ids, cur=tc.data_ptr(), prev=tp.data_ptr(), mh=mh, rect=None, vp=vp) | b
        with pytest.raises(BlokError) as e:
            tr.instance_motion_device(wp, a["ids"], a["cur"], len(cur), a["prev"], len(prev), a["vp"], motion_h_ptr=a["mh"], rect=a["rect"])
        assert e.value.status == -1, b
    den = torch.zeros((WD * HT, 4), dtype=torch.float32, device="cuda")
    for b in (dict(ids=0), dict(cur=0), dict(prev=0)):
        a = dict(ids=ids, cur=tc.data_ptr(), prev=tp.data_ptr()) | b
        with pytest.raises(BlokError) as e:
            tr.denoise_instanced_ref_device(P["color"].data_ptr(), wp, P["nr"].data_ptr(), mh, vp, 0, den.data_ptr(), a["ids"], a["cur"], len(cur),
                                            a["prev"], len(prev))
        assert e.value.status == -1, b
    wrong = cur.copy(); wrong[1]["flip"] = 8
    with pytest.raises(BlokError) as e:
        tr.draw_frame_rt_instanced_motion(top_camera(), wrong, spp=1)
    assert e.value.status == -1
    tr.shutdown()


def test_tables_change_in_stream_order(torch_cuda, scene64):
    torch = torch_cuda
    _, pw = scene64
    tr = tracer(pw)
    cam = top_camera()
    vp = tr.camera_view_proj(W.camera_look_at((45.0, 129.0, 21.0), (44.0, 10.0, 46.0), 70.0, WD, HT))
    cur, prev = moved_tables()
    P = ref_planes(torch, WD * HT)
    tc0 = dev_table(torch, cur)
    trace_ref(tr, cam, P, tc0, len(cur), vp, 1)
    torch.cuda.synchronize()
    other = prev.copy(); other[0]["offset"] = (30, 70, 30); other[1]["flip"] = 2
    want = []
    for t in (prev, other):
        m = torch.zeros((WD * HT, 2), dtype=torch.float32, device="cuda")
        tt = dev_table(torch, t)
        tr.instance_motion_device(P["world_pos"].data_ptr(), P["ids"].data_ptr(), tc0.data_ptr(), len(cur), tt.data_ptr(), len(t), vp,
                                  motion_ptr=m.data_ptr())
        torch.cuda.synchronize()
        want.append(m.cpu().numpy())
    assert (want[0] != 0).any() and want[0].tobytes() != want[1].tobytes()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tc, tp = dev_table(torch, cur), dev_table(torch, prev)
        m = [torch.zeros((WD * HT, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
        tr.instance_motion_device(P["world_pos"].data_ptr(), P["ids"].data_ptr(), tc.data_ptr(), len(cur), tp.data_ptr(), len(prev), vp,
                                  motion_ptr=m[0].data_ptr(), stream=s.cuda_stream)
        tp.copy_(torch.from_numpy(other.view(np.uint8).copy()))          # the next table, in stream order, no synchronise
        tr.instance_motion_device(P["world_pos"].data_ptr(), P["ids"].data_ptr(), tc.data_ptr(), len(cur), tp.data_ptr(), len(prev), vp,
                                  motion_ptr=m[1].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    for got, w in zip(m, want):
        assert got.cpu().numpy().tobytes() == w.tobytes()
    tr.release_stream(s.cuda_stream)
    tr.shutdown()
