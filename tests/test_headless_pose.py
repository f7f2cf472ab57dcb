"""The headless driver's --pose FILE.vox@X,Y,Z,YAW_DEG[,SCALE] (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: createModel,
tracePrimaryPosed): two models of tests/golden/vox_reference_models.tar.xz traced as posed models over the generated scene.  The written
PPM and the printed count go against the Python API's frame (HipTracer.trace_primary_posed) of blok_amd.pose.rotation(...) for the camera the
driver prints, byte for byte; and the flag's refusals."""
import math
import re
import subprocess
import tarfile
from pathlib import Path

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import pose as P
from blok_amd import world as W
from blok_amd._ffi import CAMERA, INSTANCE_NONE, POSE_ID
from blok_amd.vox import VoxFile

GOLDEN = Path(__file__).resolve().parent / "golden"
N, WD, HT = 64, 64, 48


def quarter(v):
    return round(float(v) * 4.0) / 4.0


@pytest.fixture(scope="module")
def vox_models(tmp_path_factory):
    """[(path, voxels in the driver's local lattice (VOX z is up -> local y), palette index per voxel)] of two models."""
    out = tmp_path_factory.mktemp("pose")
    models = []
    with tarfile.open(GOLDEN / "vox_reference_models.tar.xz") as tar:
        for name in ("chr_knight.vox", "teapot.vox"):
            path = out / name
            path.write_bytes(tar.extractfile(name).read())
            vox = VoxFile.load_file(str(path))
            voxels = np.array(vox.model(0)[1]).reshape(-1, 4)         # a copy: the file's memory goes with close()
            vox.close()
            models.append((path, np.stack([voxels[:, 0], voxels[:, 2], voxels[:, 1]], axis=1).astype(np.int32), voxels[:, 3].astype(np.uint32)))
    return models


def placements(models):
    """Where the two models stand: in front of the scene's camera (pose 0), on the quarter-voxel grid so that the command line holds them exactly."""
    cam = W.scene_camera(N, 0, WD, HT)[0]
    pos, fwd, right = (np.array(cam[k], dtype=np.float64) for k in ("pos", "fwd", "right"))
    spots = [(pos + 30.0 * fwd - 6.0 * right, 30.0, 1.0), (pos + 60.0 * fwd + 25.0 * right, -110.0, 0.5)]
    return [(tuple(quarter(c) for c in at), yaw, scale) for at, yaw, scale in spots]


@pytest.mark.gpu
def test_driver_traces_two_posed_models_like_the_python_api(tmp_path, vox_models):
    from blok_amd.tracer import HipTracer
    exe = b.build_tools()
    spots = placements(vox_models)
    args = []
    for (path, _, _), (at, yaw, scale) in zip(vox_models, spots):
        spec = f"{path}@{at[0]},{at[1]},{at[2]},{yaw}" + ("" if scale == 1.0 else f",{scale}")       # the scale may be left out
        args += ["--pose", spec]
    out = tmp_path / "posed.ppm"
    run = subprocess.run([str(exe), "--n", str(N), "--size", f"{WD}x{HT}", "--frames", "1", "--out", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    cam = np.zeros(1, dtype=CAMERA)
    cam.view(np.float32)[:] = [np.float32(v) for v in re.search(r"pose: camera (.*)", run.stdout).group(1).split()]
    printed = re.search(r"pose: poses won (\d+) of (\d+) pixels", run.stdout)
    assert printed and int(printed.group(2)) == WD * HT, run.stdout
    # the same frame through the Python API
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
    tr.check_poses(poses)
    _, ids, rgba = tr.trace_primary_posed(cam, None, poses)
    plain = tr.draw_frame(cam)
    tr.shutdown()
    won = (ids != INSTANCE_NONE) & ((ids & POSE_ID) != 0)
    print(f"driver: {printed.group(1)} pixels; python: {int(won.sum())}, by pose {[int((ids == (POSE_ID | j)).sum()) for j in range(2)]}")
    assert int(printed.group(1)) == int(won.sum())
    assert all((ids == (POSE_ID | j)).sum() > 20 for j in range(2)) and (plain["hit"][~won] == 1).sum() > 200      # both models and the scene are on screen
    head = f"P6\n{WD} {HT}\n255\n".encode()
    data = out.read_bytes()
    assert data.startswith(head)
    want = np.stack([rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255], axis=-1).astype(np.uint8)
    assert data[len(head):] == want.tobytes()


def test_the_flag_is_refused_with_rt_and_without_its_grammar(tmp_path):
    exe = b.build_tools()
    run = subprocess.run([str(exe), "--n", "64", "--rt", "--pose", "model.vox@1,2,3,30"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--rt" in run.stderr and "takes no pose table" in run.stderr, run.stderr
    for bad in ("@1,2,3,0", "m.vox@1,2,3", "m.vox@1,2,3,0,1,5", "m.vox@1,2,3,0,0", "m.vox@1,2,3,0,-2", "m.vox@1,2,x,0,1", "m.vox@1,2,3,nan"):
        run = subprocess.run([str(exe), "--n", "64", "--pose", bad], capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--pose takes FILE.vox@X,Y,Z,YAW_DEG[,SCALE]" in run.stderr, (bad, run.stderr)


@pytest.mark.gpu
def test_the_flag_needs_a_file_and_a_world_it_can_stand_in(tmp_path, vox_models):
    exe = b.build_tools()
    path = vox_models[0][0]
    common = ["--size", "64x48", "--frames", "1", "--out", str(tmp_path / "f.ppm")]
    for args, text in ((["--n", "64", "--pose", f"{tmp_path / 'none.vox'}@1,2,3,0"], "Failed to load VOX"),
                       (["--vox", str(path), "--pose", f"{path}@1,2,3,0"], "over the generated scene or a --terrain"),
                       (["--n", "64", "--pose", f"{path}@1,2,3,0,0.0001"], "SCALE must be at least 1/1024")):
        run = subprocess.run([str(exe)] + common + args, capture_output=True, text=True, timeout=300)
        assert run.returncode == 1 and text in run.stderr, (args, run.stderr)
    # over a terrain the models' palettes are imported; the camera pose number still goes through the same flag
    from blok_amd import terrain as T
    ground = int(T.height(T.default_params(32, 7), [(16, 16)])[0])
    spec = f"{path}@16,{ground + 5},16,45,0.5"                                  # where the terrain's camera looks
    run = subprocess.run([str(exe), "--terrain", "7", "--terrain-size", "32", "--pose", "0", "--pose", spec] + common, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert int(re.search(r"pose: poses won (\d+) of 3072 pixels", run.stdout).group(1)) > 20, run.stdout
