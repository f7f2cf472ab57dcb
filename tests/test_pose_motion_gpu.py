"""GPU: object motion for posed models (blok_hip_posed_motion_device, blok_hip_denoise_posed_ref_device,
blok_hip_draw_frame_rt_posed_motion, blok_hip_debug_pose_motion_records; include/blok_hip.h, "Object motion for posed models").

References: the host helper's records (tests/test_pose_motion_cpu.py holds those against numpy float64), numpy's object motion from the path
kernel's own world-position and id planes and the tables (tests/pose_motion_reference.py, tests/test_instance_motion_gpu.py), the entries
without object motion (an unmoved table: the same bits), and the passes called one by one."""
from __future__ import annotations

import math

import numpy as np
import pytest

from blok_amd import pose as P
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, INSTANCE_NONE, POSE, POSE_ID, BlokError
from tests import instance_oracle as IO
from tests import pose_motion_reference as R
from tests.test_instance_motion_gpu import MODELS, camera_path, dev_table, erode, moved_tables, object_motion, ref_planes, top_camera, tracer
from tests.test_pose_motion_cpu import case_poses, causes

pytestmark = pytest.mark.gpu

WD, HT = 128, 96
PLATE_CENTRE = (8.0, 1.0, 8.0)                   # of the 16 x 2 x 16 plate (models 0 and 2), in its own voxels
BLOCK_CENTRE = (1.5, 1.5, 1.5)                   # of the 3^3 block (model 1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def plate_pose(yaw_degrees, position, model=0, pitch_degrees=0.0, scale=1.0):
    return P.rotation(model, math.radians(yaw_degrees), math.radians(pitch_degrees), 0.0, scale, PLATE_CENTRE if model != 1 else BLOCK_CENTRE, position)[0]


def dev_poses(torch, table):
    return torch.from_numpy(np.ascontiguousarray(table, dtype=POSE).view(np.uint8).copy()).cuda()


def host_records(cur, prev, usable=None):
    out = [P.motion_record(c, prev[i] if i < len(prev) else None, True if usable is None else usable[i]) for i, c in enumerate(cur)]
    return np.concatenate(out) if out else np.zeros(0, dtype=R.POSE_MOTION)


def trace_posed_ref(tr, cam, B, inst_dev, n_inst, poses_dev, n_poses, prev_vp, frame, spp=2, rect=None, stream=0):
    tr.trace_paths_posed_ref_device(cam, inst_dev.data_ptr() if n_inst else 0, n_inst, poses_dev.data_ptr() if n_poses else 0, n_poses,
                                    B["color"].data_ptr(), B["world_pos"].data_ptr(), B["nr"].data_ptr(), B["alb"].data_ptr(), B["motion"].data_ptr(),
                                    prev_vp, B["ids"].data_ptr(), spp=spp, max_bounces=2, frame_index=frame, rect=rect, stream=stream)


# ------------------------------------------------------------------------------------------------ the prepare kernel
def test_prepare_kernel_equals_the_host_helper_on_seventy_poses(torch_cuda, scene64):
    """More than one wave, not a multiple of 64; every state and every cause of an untracked pose (a model that is not usable: a destroyed
    one, and an id beyond the store)."""
    _, pw = scene64
    tr = tracer(pw)
    dead = tr.model_create(*MODELS[1])
    tr.model_destroy(dead)
    rows = []
    for name, (cur, prev, usable, state) in causes().items():
        cur, prev = cur.copy(), (None if prev is None else prev.copy())
        if not usable:
            cur["model"] = prev["model"] = dead
        rows.append((cur, prev, usable, state))
    beyond = [r for r in rows if r[1] is None]
    rows = [r for r in rows if r[1] is not None]
    poses = case_poses()
    k = 0
    while len(rows) + len(beyond) < 69:
        rows.append((poses[k % len(poses)], poses[(k * 5 + 1) % len(poses)], True, None)); k += 1
    gone = rows[0][0].copy(); gone["model"] = 9                       # beyond the store, on both sides
    rows.append((gone, gone.copy(), False, 0))
    rows += [(c, None, u, s) for c, _, u, s in beyond]                 # the table's tail: beyond n_prev
    assert len(rows) == 70
    cur = np.array([r[0] for r in rows], dtype=POSE)
    prev = np.array([r[1] for r in rows if r[1] is not None], dtype=POSE)
    assert len(prev) == 70 - len(beyond) and len(beyond) >= 1
    got = tr.debug_pose_motion_records(cur, prev)
    want = host_records(cur, prev, [r[2] for r in rows])
    for i, r in enumerate(rows):
        assert got[i].tobytes() == want[i].tobytes(), (i, got[i], want[i])
        if r[3] is not None:
            assert int(got[i]["state"]) == r[3], i
    assert {0, 1, 2} == set(got["state"].tolist()) and (got["state"] == 2).sum() > 20
    assert len(tr.debug_pose_motion_records(cur[:0], prev)) == 0
    tr.shutdown()


# ------------------------------------------------------------------------------------------------ the motion kernel
def mixed_tables():
    """Two instances (one translated, one turned in place) and three poses: a plate turned and lifted, a block turned about two axes and
    moved, and a plate that changed model (untracked)."""
    cur_i, prev_i = moved_tables()
    prev_i = prev_i.copy(); cur_i = cur_i.copy()
    prev_p = np.array([plate_pose(15.0, (63.0, 72.0, 36.0)), plate_pose(0.0, (58.0, 80.0, 51.0), model=1, scale=2.0),
                       plate_pose(40.0, (66.0, 66.0, 54.0), model=2)], dtype=POSE)
    cur_p = np.array([plate_pose(22.0, (64.0, 74.5, 36.5)), plate_pose(30.0, (59.0, 80.5, 50.0), model=1, pitch_degrees=20.0, scale=2.0),
                      plate_pose(40.0, (66.0, 66.0, 54.0), model=0)], dtype=POSE)
    return cur_i, prev_i, cur_p, prev_p


@pytest.mark.parametrize("frame,rect", [((WD, HT), None), ((WD, HT), (16, 8, 96, 72)), ((116, 86), (8, 8, 100, 70))])
def test_posed_motion_kernel_equals_numpy(torch_cuda, scene64, frame, rect):
    torch = torch_cuda
    _, pw = scene64
    fw, fh = frame
    tr = tracer(pw, w=fw, h=fh)
    x0, y0, w, h = rect if rect is not None else (0, 0, fw, fh)
    n = w * h
    cam = W.camera_look_at((44.0, 130.0, 20.0), (44.0, 10.0, 46.0), 70.0, fw, fh)
    prev_vp = tr.camera_view_proj(W.camera_look_at((45.0, 129.0, 21.0), (44.0, 10.0, 46.0), 70.0, fw, fh))
    cur_i, prev_i, cur_p, prev_p = mixed_tables()
    ti, tpi, tp, tpp = dev_table(torch, cur_i), dev_table(torch, prev_i), dev_poses(torch, cur_p), dev_poses(torch, prev_p)
    B = ref_planes(torch, n)
    trace_posed_ref(tr, cam, B, ti, len(cur_i), tp, len(cur_p), prev_vp, 1, rect=rect)
    torch.cuda.synchronize()
    before = B["motion"].cpu().numpy().copy()
    m2 = torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda")
    tr.posed_motion_device(B["world_pos"].data_ptr(), B["ids"].data_ptr(), ti.data_ptr(), len(cur_i), tpi.data_ptr(), len(prev_i),
                           tp.data_ptr(), len(cur_p), tpp.data_ptr(), len(prev_p), prev_vp, motion_h_ptr=B["motion"].data_ptr(),
                           motion_ptr=m2.data_ptr(), rect=rect)
    torch.cuda.synchronize()
    ids = B["ids"].cpu().numpy().view(np.uint32).reshape(h, w)
    wp = B["world_pos"].cpu().numpy().reshape(h, w, 4)
    records = host_records(cur_p, prev_p)
    assert records["state"].tolist() == [2, 2, 0]
    t_inst, want_inst = object_motion(wp, ids, cur_i, prev_i, prev_vp, x0=x0, y0=y0, frame_w=fw, frame_h=fh)
    t_pose, want_pose = R.pose_object_motion(wp, ids, records, prev_vp, x0, y0, fw, fh)
    assert not (t_inst & t_pose).any()
    tracked = t_inst | t_pose
    want = np.where(t_pose[..., None], want_pose, want_inst)
    assert t_pose.sum() >= 200 and t_inst.sum() > 100, (int(t_pose.sum()), int(t_inst.sum()))
    assert set(np.unique(ids[t_pose]).tolist()) == {POSE_ID | 0, POSE_ID | 1} and (ids == (POSE_ID | 2)).sum() > 50
    got_h = B["motion"].cpu().numpy().view(np.uint16).reshape(h, w, 2)
    got_f = m2.cpu().numpy().reshape(h, w, 2)
    assert np.array_equal(got_h[tracked], want[tracked].astype(np.float16).view(np.uint16))
    assert got_f[tracked].tobytes() == want[tracked].tobytes()
    assert (np.abs(got_f[t_pose]) > 1e-4).any()
    assert got_h[~tracked].tobytes() == before.view(np.uint16).reshape(h, w, 2)[~tracked].tobytes()
    assert (got_f[~tracked] == -7.0).all()
    tr.shutdown()


# ------------------------------------------------------------------------------------------------ the frame entry
def test_unmoved_poses_give_the_posed_frame_and_no_poses_the_instanced_motion_frame(torch_cuda, scene64):
    _, pw = scene64
    cur_i, prev_i, cur_p, _ = mixed_tables()
    a, b = tracer(pw), tracer(pw)
    for k in range(6):
        got, fa = a.draw_frame_rt_posed_motion(camera_path(k), cur_i, cur_p, spp=2)
        want, fb = b.draw_frame_rt_posed(camera_path(k), cur_i, cur_p, spp=2)
        assert fa == fb == k + 1
        assert got.tobytes() == want.tobytes(), k
        for x, y in zip(a.denoise_state(), b.denoise_state()):
            assert x.tobytes() == y.tobytes(), k
    a.post_reset(); b.post_reset()
    for k in range(4):
        table = prev_i if k % 2 else cur_i                            # the instances move
        got, _ = a.draw_frame_rt_posed_motion(camera_path(k), table, None, spp=2)
        want, _ = b.draw_frame_rt_instanced_motion(camera_path(k), table, spp=2)
        assert got.tobytes() == want.tobytes(), k
        for x, y in zip(a.denoise_state(), b.denoise_state()):
            assert x.tobytes() == y.tobytes(), k
    a.shutdown(); b.shutdown()


def moving_tables(k):
    inst = np.array([IO.instance(0, (30 + 3 * k, 62 + 3 * k, 36)), IO.instance(1, (20, 80, 60 - 2 * k))], dtype=INSTANCE)
    poses = np.array([plate_pose(10.0 + 7.0 * k, (64.0, 70.0 + 2.5 * k, 40.0)), plate_pose(5.0 * k, (58.0 + k, 82.0, 52.0), model=1, pitch_degrees=3.0 * k, scale=2.0)],
                     dtype=POSE)
    return inst, poses


def test_entry_is_the_composition_of_the_passes(torch_cuda, scene64):
    torch = torch_cuda
    _, pw = scene64
    one, many = tracer(pw), tracer(pw)
    n = WD * HT
    B = ref_planes(torch, n)
    den = torch.zeros((n, 4), dtype=torch.float32, device="cuda"); taa = torch.zeros_like(den)
    ldr = torch.zeros(n, dtype=torch.int32, device="cuda"); sharp = torch.zeros_like(ldr)
    prev_i, prev_p, n_prev_i, n_prev_p = None, None, 0, 0
    for k in range(5):
        cam = camera_path(k)
        inst, poses = moving_tables(k)
        got, frames = one.draw_frame_rt_posed_motion(cam, inst, poses, spp=2)
        assert frames == k + 1
        cur_i, cur_p = dev_table(torch, inst), dev_poses(torch, poses)
        prev_vp = many.camera_view_proj(camera_path(max(k - 1, 0)))
        many.set_taa_jitter(W.taa_jitter(k))
        trace_posed_ref(many, cam, B, cur_i, len(inst), cur_p, len(poses), prev_vp, k)
        many.set_taa_jitter(None)
        tables = (cur_i.data_ptr(), len(inst), prev_i.data_ptr() if n_prev_i else 0, n_prev_i,
                  cur_p.data_ptr(), len(poses), prev_p.data_ptr() if n_prev_p else 0, n_prev_p)
        many.posed_motion_device(B["world_pos"].data_ptr(), B["ids"].data_ptr(), *tables, prev_vp, motion_h_ptr=B["motion"].data_ptr())
        many.denoise_posed_ref_device(B["color"].data_ptr(), B["world_pos"].data_ptr(), B["nr"].data_ptr(), B["motion"].data_ptr(), prev_vp, k,
                                      den.data_ptr(), B["ids"].data_ptr(), *tables)
        many.taa_device(den.data_ptr(), taa.data_ptr(), k)
        many.tonemap_device(taa.data_ptr(), ldr.data_ptr())
        many.sharpen_device(ldr.data_ptr(), sharp.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(got.reshape(-1), sharp.cpu().numpy().view(np.uint32)), k
        for x, y in zip(one.denoise_state(), many.denoise_state()):
            assert x.tobytes() == y.tobytes(), k
        prev_i, prev_p, n_prev_i, n_prev_p = cur_i, cur_p, len(inst), len(poses)
    one.shutdown(); many.shutdown()


# ------------------------------------------------------------------------------------------------ it accumulates
def plate_sequence(kind, frames=8):
    if kind == "lifted":
        return [np.array([plate_pose(0.0, (44.0, 63.0 + 3.0 * k, 44.0))], dtype=POSE) for k in range(frames)]
    return [np.array([plate_pose(7.0 * k, (44.0, 63.0 + 2.5 * k, 44.0))], dtype=POSE) for k in range(frames)]


def run_sequence(tr, tables, cam, motion):
    """Draw the frames; per frame the id footprint of pose 0 and the denoiser's state."""
    out = []
    for t in tables:
        if motion:
            tr.draw_frame_rt_posed_motion(cam, None, t, spp=2)
        else:
            tr.draw_frame_rt_posed(cam, None, t, spp=2)
        _, ids, _ = tr.trace_primary_posed(cam, None, t)
        out.append((ids == (POSE_ID | 0), tr.denoise_state()))
    return out


@pytest.mark.parametrize("kind", ["lifted", "turned"])
def test_a_moving_posed_plate_accumulates_history(torch_cuda, scene64, kind):
    """The behaviour the feature exists for: a camera at rest, the plate given as a pose and per frame (a) lifted by 3 voxels or (b) turned by
    7 degrees about its centre and lifted by 2.5, for 8 frames.  With object motion its interior pixels keep accumulating (the statistic and
    threshold of tests/test_instance_motion_gpu.py's rising plate); without, a lifted plate holds 1: pos_ok needs less than 2 voxels."""
    _, pw = scene64
    cam = top_camera()
    tables = plate_sequence(kind)
    tr = tracer(pw)
    new = run_sequence(tr, tables, cam, True)
    inside = erode(new[-1][0], 2) & erode(new[-2][0], 2)
    assert inside.sum() > 100
    hist = new[-1][1][2]
    print(kind, "history on the interior:", np.unique(hist[inside], return_counts=True))
    assert (hist[inside] >= 6).all(), np.unique(hist[inside], return_counts=True)
    mo = new[-1][1][4]
    assert (np.abs(mo[inside]).max(axis=-1) > 1e-3).mean() > 0.5
    if kind == "lifted":
        tr.post_reset()
        old = run_sequence(tr, tables, cam, False)
        assert (old[-1][1][2][inside] == 1).all()
    tr.shutdown()


def test_untracked_poses_start_without_history(torch_cuda, scene64):
    _, pw = scene64
    cam = top_camera()
    base = plate_pose(10.0, (44.0, 63.0, 44.0))
    second = plate_pose(0.0, (66.0, 66.0, 40.0))
    one_table, two = np.array([base], POSE), np.array([base, second], POSE)
    swapped = two.copy(); swapped[0]["model"] = 2                     # the same voxels under another id
    steps = [("motion", one_table)] * 3 + [("motion", two), ("motion", swapped), ("motion", swapped), ("plain", swapped), ("motion", swapped),
                                           ("motion", swapped), ("scale", swapped), ("motion", swapped)]
    # step -> (plate, second).  1: every interior pixel restarts.  Otherwise the history goes on: at least that length on nine interior pixels in
    # ten (the crease between two faces of a resting plate may restart under the TAA jitter, in the existing pass as here).
    expect = {3: (3, 1), 4: (1, 2), 5: (2, 3), 7: (1, 1), 8: (2, 2), 10: (1, 1)}
    tr = tracer(pw)
    for k, (how, t) in enumerate(steps):
        if how == "scale":
            tr.model_set_scale(1, 0)                                   # any set_scale empties the previous tables
            continue
        (tr.draw_frame_rt_posed_motion if how == "motion" else tr.draw_frame_rt_posed)(cam, None, t, spp=2)
        _, ids, _ = tr.trace_primary_posed(cam, None, t)
        hist = tr.denoise_state()[2]
        plate_px, second_px = erode(ids == (POSE_ID | 0), 2), erode(ids == (POSE_ID | 1), 2)
        assert plate_px.sum() > 100
        if k in expect:
            assert second_px.sum() > 50
            for px, want in zip((plate_px, second_px), expect[k]):
                if want == 1:
                    assert (hist[px] == 1).all(), (k, np.unique(hist[px], return_counts=True))
                else:
                    assert (hist[px] >= want).mean() > 0.9, (k, want, np.unique(hist[px], return_counts=True))
    tr.shutdown()


# ------------------------------------------------------------------------------------------------ errors, streams
def test_errors_leave_outputs_untouched(torch_cuda, scene64):
    torch = torch_cuda
    _, pw = scene64
    tr = tracer(pw)
    cur_i, prev_i, cur_p, prev_p = mixed_tables()
    ti, tpi, tp, tpp = dev_table(torch, cur_i), dev_table(torch, prev_i), dev_poses(torch, cur_p), dev_poses(torch, prev_p)
    B = ref_planes(torch, WD * HT)
    vp = tr.camera_view_proj(top_camera())
    trace_posed_ref(tr, top_camera(), B, ti, len(cur_i), tp, len(cur_p), vp, 0)
    wp, ids, mh = B["world_pos"].data_ptr(), B["ids"].data_ptr(), B["motion"].data_ptr()
    m2 = torch.full((WD * HT, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = B["motion"].cpu().numpy().tobytes()
    good = dict(wp=wp, ids=ids, cur=ti.data_ptr(), prev=tpi.data_ptr(), curp=tp.data_ptr(), prevp=tpp.data_ptr(), mh=mh, m=m2.data_ptr(), rect=None, vp=vp)
    bad = [dict(wp=0), dict(ids=0), dict(cur=0), dict(prev=0), dict(curp=0), dict(prevp=0), dict(mh=0, m=0), dict(rect=(0, 0, WD + 1, HT)),
           dict(rect=(WD - 8, 0, 16, 8)), dict(vp=None)]
    messages = []
    for b in bad:
        a = good | b
        with pytest.raises(BlokError) as e:
            tr.posed_motion_device(a["wp"], a["ids"], a["cur"], len(cur_i), a["prev"], len(prev_i), a["curp"], len(cur_p), a["prevp"], len(prev_p), a["vp"],
                                   motion_h_ptr=a["mh"], motion_ptr=a["m"], rect=a["rect"])
        assert e.value.status == -1, b
        messages.append(str(e.value))
    # the instanced entry's texts, in its order
    with pytest.raises(BlokError) as e:
        tr.instance_motion_device(wp, ids, 0, len(cur_i), tpi.data_ptr(), len(prev_i), vp, motion_h_ptr=mh)
    assert str(e.value) == messages[2] == messages[3]
    assert "null pose table" in messages[4] and "null pose table" in messages[5]
    with pytest.raises(BlokError) as e:                                # a null instance table is named before a null pose table
        tr.posed_motion_device(wp, ids, 0, len(cur_i), tpi.data_ptr(), len(prev_i), 0, len(cur_p), tpp.data_ptr(), len(prev_p), vp, motion_h_ptr=mh)
    assert str(e.value) == messages[2]
    den = torch.full((WD * HT, 4), -3.0, dtype=torch.float32, device="cuda")
    for b in (dict(ids=0), dict(cur=0), dict(prev=0), dict(curp=0), dict(prevp=0), dict(vp=None)):
        a = good | b
        with pytest.raises(BlokError) as e:
            tr.denoise_posed_ref_device(B["color"].data_ptr(), wp, B["nr"].data_ptr(), mh, a["vp"], 0, den.data_ptr(), a["ids"], a["cur"], len(cur_i),
                                        a["prev"], len(prev_i), a["curp"], len(cur_p), a["prevp"], len(prev_p))
        assert e.value.status == -1, b
    torch.cuda.synchronize()
    assert B["motion"].cpu().numpy().tobytes() == before and (m2 == -7.0).all() and (den == -3.0).all()
    # host tables: a bad pose is named as check_poses names it, a bad instance as check_instances does; the frame counter stays
    _, frames = tr.draw_frame_rt_posed_motion(top_camera(), cur_i, cur_p, spp=1)
    wrong = cur_p.copy(); wrong[1]["m"][0][0] = np.nan
    with pytest.raises(BlokError) as named:
        tr.check_poses(wrong)
    with pytest.raises(BlokError) as e:
        tr.draw_frame_rt_posed_motion(top_camera(), cur_i, wrong, spp=1)
    assert e.value.status == -1 and str(e.value) == str(named.value) and "pose 1" in str(e.value)
    wrong_i = cur_i.copy(); wrong_i[1]["flip"] = 8
    with pytest.raises(BlokError) as e:
        tr.draw_frame_rt_posed_motion(top_camera(), wrong_i, cur_p, spp=1)
    assert e.value.status == -1 and "instance 1" in str(e.value)
    assert tr.draw_frame_rt_posed_motion(top_camera(), cur_i, cur_p, spp=1)[1] == frames + 1
    tr.shutdown()


def test_tables_change_in_stream_order(torch_cuda, scene64):
    torch = torch_cuda
    _, pw = scene64
    tr = tracer(pw)
    cam = top_camera()
    vp = tr.camera_view_proj(W.camera_look_at((45.0, 129.0, 21.0), (44.0, 10.0, 46.0), 70.0, WD, HT))
    cur_i, prev_i, cur_p, prev_p = mixed_tables()
    B = ref_planes(torch, WD * HT)
    ti0, tp0 = dev_table(torch, cur_i), dev_poses(torch, cur_p)
    trace_posed_ref(tr, cam, B, ti0, len(cur_i), tp0, len(cur_p), vp, 1)
    torch.cuda.synchronize()
    other = prev_p.copy(); other[0] = plate_pose(-20.0, (62.0, 71.0, 37.0)); other[1]["pivot"][1] += 1.5
    want = []
    for t in (prev_p, other):
        m = torch.zeros((WD * HT, 2), dtype=torch.float32, device="cuda")
        tt = dev_poses(torch, t)
        tr.posed_motion_device(B["world_pos"].data_ptr(), B["ids"].data_ptr(), ti0.data_ptr(), len(cur_i), 0, 0, tp0.data_ptr(), len(cur_p),
                               tt.data_ptr(), len(t), vp, motion_ptr=m.data_ptr())
        torch.cuda.synchronize()
        want.append(m.cpu().numpy())
    assert (want[0] != 0).any() and want[0].tobytes() != want[1].tobytes()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ti, tp, tpp = dev_table(torch, cur_i), dev_poses(torch, cur_p), dev_poses(torch, prev_p)
        m = [torch.zeros((WD * HT, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
        tr.posed_motion_device(B["world_pos"].data_ptr(), B["ids"].data_ptr(), ti.data_ptr(), len(cur_i), 0, 0, tp.data_ptr(), len(cur_p),
                               tpp.data_ptr(), len(prev_p), vp, motion_ptr=m[0].data_ptr(), stream=s.cuda_stream)
        tpp.copy_(torch.from_numpy(other.view(np.uint8).copy()))          # the next table, in stream order, no synchronise
        tr.posed_motion_device(B["world_pos"].data_ptr(), B["ids"].data_ptr(), ti.data_ptr(), len(cur_i), 0, 0, tp.data_ptr(), len(cur_p),
                               tpp.data_ptr(), len(prev_p), vp, motion_ptr=m[1].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    for got, w in zip(m, want):
        assert got.cpu().numpy().tobytes() == w.tobytes()
    tr.release_stream(s.cuda_stream)
    tr.shutdown()
