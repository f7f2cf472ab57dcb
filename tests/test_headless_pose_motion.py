"""The headless driver's --rt-posed --pose-motion [--pose-spin DEG] (tools/blok_headless.cpp over include/blok/hip_tracer.hpp:
drawFrameRtPosedMotion): two models of tests/golden/vox_reference_models.tar.xz go through the path-traced chain as posed models that yaw by
DEG per drawn frame, with object motion.  The written PPM goes against the Python API's draw_frame_rt_posed_motion driven with the same poses
and the cameras the driver prints, byte for byte; and the flag's refusals."""
import math
import re
import subprocess

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import pose as P
from blok_amd import world as W
from blok_amd._ffi import CAMERA
from tests.test_headless_pose import HT, N, WD, placements, vox_models  # noqa: F401  (vox_models: the fixture)

SPIN, FRAMES, SPP = 5.0, 4, 2


@pytest.mark.gpu
def test_driver_spins_two_posed_models_like_the_python_api(tmp_path, vox_models):  # noqa: F811
    from blok_amd.tracer import HipTracer
    exe = b.build_tools()
    spots = placements(vox_models)
    args = []
    for (path, _, _), (at, yaw, scale) in zip(vox_models, spots):
        args += ["--pose", f"{path}@{at[0]},{at[1]},{at[2]},{yaw},{scale}"]
    out = tmp_path / "pose_motion.ppm"
    run = subprocess.run([str(exe), "--n", str(N), "--size", f"{WD}x{HT}", "--frames", str(FRAMES), "--spp", str(SPP), "--rt-posed", "--pose-motion",
                          "--pose-spin", str(SPIN), "--out", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    printed = re.findall(r"pose: frame (\d+) camera (.*)", run.stdout)
    assert [int(f) for f, _ in printed] == list(range(FRAMES + 1))     # the timed frames, then the written one
    cams = []
    for _, text in printed:
        cam = np.zeros(1, dtype=CAMERA)
        cam.view(np.float32)[:] = [np.float32(v) for v in text.split()]
        cams.append(cam)
    assert cams[0].tobytes() != cams[1].tobytes() and cams[-1].tobytes() == cams[-2].tobytes()
    # the same frames through the Python API
    cm = W.ChunkManager(128, 1.0)
    cm.generate_scene(N)
    cm.rebuild_dirty_chunks()
    tr = HipTracer(WD, HT).init()
    tr.add_world(cm.pack_chunks_to_gpu_svo(W.scene_materials()))
    placed = []
    for (_, xyz, palette), (at, yaw, scale) in zip(vox_models, spots):
        lo, hi = xyz.min(axis=0), xyz.max(axis=0) + 1
        centre = tuple((int(a) + int(c)) / 2.0 for a, c in zip(lo, hi))
        placed.append((tr.model_create(xyz, palette), yaw, scale, centre, at))
    table = lambda f: np.concatenate([P.rotation(m, yaw=math.radians(yaw + f * SPIN), scale=scale, pivot_local=centre, position=at)
                                      for m, yaw, scale, centre, at in placed])
    for f, cam in enumerate(cams):
        rgba, frames = tr.draw_frame_rt_posed_motion(cam, None, table(f), SPP, 2)
    assert frames == FRAMES + 1
    hist_motion = tr.denoise_state()[2]
    # the same sequence without object motion differs: the flag chose the other entry
    tr.post_reset()
    for f, cam in enumerate(cams):
        plain, _ = tr.draw_frame_rt_posed(cam, None, table(f), SPP, 2)
    hist_plain = tr.denoise_state()[2]
    tr.shutdown()
    assert hist_motion.tobytes() != hist_plain.tobytes()
    head = f"P6\n{WD} {HT}\n255\n".encode()
    data = out.read_bytes()
    assert data.startswith(head)
    want = np.stack([rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255], axis=-1).astype(np.uint8)
    assert data[len(head):] == want.tobytes()


def test_the_flags_are_refused_without_rt_posed(tmp_path):
    exe = b.build_tools()
    for flags in (["--pose-motion"], ["--pose-motion", "--pose-spin", "5"], ["--pose-spin", "5"], ["--rt", "--pose-motion"]):
        run = subprocess.run([str(exe), "--n", "64"] + flags, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "give --rt-posed" in run.stderr, (flags, run.stderr)
    run = subprocess.run([str(exe), "--n", "64", "--rt-posed", "--pose-spin", "5", "--pose", "m.vox@1,2,3,30"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "give --pose-motion" in run.stderr, run.stderr
    run = subprocess.run([str(exe), "--n", "64", "--rt-posed", "--pose-motion"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "give at least one --pose" in run.stderr, run.stderr
