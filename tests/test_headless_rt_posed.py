"""The headless driver's --rt-posed (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: drawFrameRtPosed): two models of
tests/golden/vox_reference_models.tar.xz go through the path-traced chain as posed models over the generated scene.  The written PPM goes
against the Python API's draw_frame_rt_posed of blok_amd.pose.rotation(...) for the camera the driver prints, after the same number of
frames, byte for byte; and the flag's refusals."""
import math
import re
import subprocess

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import pose as P
from blok_amd import world as W
from blok_amd._ffi import CAMERA, INSTANCE_NONE, POSE_ID
from tests.test_headless_pose import HT, N, WD, placements, vox_models  # noqa: F401  (vox_models: the fixture)


@pytest.mark.gpu
def test_driver_path_traces_two_posed_models_like_the_python_api(tmp_path, vox_models):  # noqa: F811
    from blok_amd.tracer import HipTracer
    exe = b.build_tools()
    spots = placements(vox_models)
    args = []
    for (path, _, _), (at, yaw, scale) in zip(vox_models, spots):
        args += ["--pose", f"{path}@{at[0]},{at[1]},{at[2]},{yaw},{scale}"]
    out = tmp_path / "rt_posed.ppm"
    spp = 2
    run = subprocess.run([str(exe), "--n", str(N), "--size", f"{WD}x{HT}", "--frames", "1", "--spp", str(spp), "--rt-posed", "--out", str(out)] + args,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "path trace" in run.stdout and "poses won" not in run.stdout
    cam = np.zeros(1, dtype=CAMERA)
    cam.view(np.float32)[:] = [np.float32(v) for v in re.search(r"pose: camera (.*)", run.stdout).group(1).split()]
    # the same frames through the Python API: --frames 1 draws the timed frame and the written one, both at the printed camera
    cm = W.ChunkManager(128, 1.0)
    cm.generate_scene(N)
    cm.rebuild_dirty_chunks()
    tr = HipTracer(WD, HT).init()
    tr.add_world(cm.pack_chunks_to_gpu_svo(W.scene_materials()))
    poses = []
    for (_, xyz, palette), (at, yaw, scale) in zip(vox_models, spots):
        lo, hi = xyz.min(axis=0), xyz.max(axis=0) + 1
        centre = tuple((int(a) + int(c)) / 2.0 for a, c in zip(lo, hi))
        poses.append(P.rotation(tr.model_create(xyz, palette), yaw=math.radians(yaw), scale=scale, pivot_local=centre, position=at))
    poses = np.concatenate(poses)
    for _ in range(2):
        rgba, frames = tr.draw_frame_rt_posed(cam, None, poses, spp, 2)
    assert frames == 2
    tr.post_reset()
    bare = [tr.draw_frame_rt(cam, spp, 2)[0] for _ in range(2)][-1]
    ids = tr.trace_paths_posed(cam, None, poses, 1, 1)["ids"]
    tr.shutdown()
    won = (ids != INSTANCE_NONE) & ((ids & POSE_ID) != 0)
    assert all((ids == (POSE_ID | j)).sum() > 20 for j in range(2))
    assert (rgba[won] != bare[won]).mean() > 0.5                  # the models are in the frame
    head = f"P6\n{WD} {HT}\n255\n".encode()
    data = out.read_bytes()
    assert data.startswith(head)
    want = np.stack([rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255], axis=-1).astype(np.uint8)
    assert data[len(head):] == want.tobytes()


def test_the_flag_is_refused_without_a_pose_and_with_what_pose_refuses(tmp_path):
    exe = b.build_tools()
    run = subprocess.run([str(exe), "--n", "64", "--rt-posed"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--rt-posed" in run.stderr and "give at least one --pose" in run.stderr, run.stderr
    for extra in (["--far", "2"], ["--vox", "m.vox"], ["--devices", "0,1"]):
        run = subprocess.run([str(exe), "--n", "64", "--rt-posed", "--pose", "m.vox@1,2,3,30"] + extra, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--rt-posed path-traces its --pose models over the generated scene" in run.stderr, (extra, run.stderr)
    run = subprocess.run([str(exe), "--n", "64", "--rt-posed", "--pose", "m.vox@1,2,3"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--pose takes FILE.vox@X,Y,Z,YAW_DEG[,SCALE]" in run.stderr, run.stderr
    # --rt with --pose keeps its refusal, with or without the new flag
    run = subprocess.run([str(exe), "--n", "64", "--rt", "--pose", "m.vox@1,2,3,30"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "takes no pose table" in run.stderr, run.stderr
