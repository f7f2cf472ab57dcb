"""The headless driver's --paste (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: createModel, stampAffine): the printed count and
the world's voxel count against blok_amd.affine.rotation + stamp_affine_host over the terrain evaluated on the host, for a model of
tests/golden/vox_reference_models.tar.xz; and the flag's error cases.  The driver has no host path: the runs that paste need the device."""
import math
import re
import subprocess
import tarfile
from pathlib import Path

import numpy as np
import pytest

from blok_amd import affine as AF
from blok_amd import build as b
from blok_amd import terrain as T
from blok_amd.vox import VoxFile

GOLDEN = Path(__file__).resolve().parent / "golden"
SEED, SIZE = 7, 96          # the box of test_headless_seal.py
PASTES = [("48,60,48,30,1", (48.0, 60.0, 48.0), 30.0, 1.0), ("40.5,52,30.25,-110,1.5", (40.5, 52.0, 30.25), -110.0, 1.5), ("70,40,70,0,0.5", (70.0, 40.0, 70.0), 0.0, 0.5)]


@pytest.fixture(scope="module")
def knight(tmp_path_factory):
    """(path of the .vox file, its first model's voxels in the driver's local lattice: VOX z is up -> local y)."""
    out = tmp_path_factory.mktemp("paste")
    with tarfile.open(GOLDEN / "vox_reference_models.tar.xz") as tar:
        data = tar.extractfile("chr_knight.vox").read()
    path = out / "chr_knight.vox"
    path.write_bytes(data)
    vox = VoxFile.load_file(str(path))
    voxels = np.array(vox.model(0)[1]).reshape(-1, 4)         # a copy: the file's memory goes with close()
    vox.close()
    return path, np.stack([voxels[:, 0], voxels[:, 2], voxels[:, 1]], axis=1).astype(np.int32)


@pytest.mark.gpu
def test_driver_pastes_a_turned_scaled_model_into_the_terrain(tmp_path, knight):
    exe = b.build_tools()
    path, xyz = knight
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "f.ppm")]
    args = [a for spec, *_ in PASTES for a in ("--paste", f"{path}@{spec}")]
    run = subprocess.run([str(exe)] + common + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    lo, hi = xyz.min(axis=0), xyz.max(axis=0) + 1
    pivot = tuple((int(a) + int(c)) / 2.0 for a, c in zip(lo, hi))
    want = []
    for _, position, yaw_deg, scale in PASTES:
        rec = AF.rotation(yaw=math.radians(yaw_deg), scale=scale, pivot=pivot, position=position)
        want.append(AF.stamp_affine_host(d, m, (0, 0, 0), xyz, np.full(len(xyz), 9, np.uint32), rec))
    got = [int(v) for v in re.findall(r"-> (\d+) voxels written", run.stdout)]
    print(f"host build: {want}; driver: {got}")
    assert got == want and all(n > 0 for n in want), run.stdout
    assert want[1] > 2 * want[0] > 8 * want[2]                 # scale 1.5 and 0.5 against 1: about 3.4 and 1/8 times the cells
    assert int(re.search(r"world: (\d+) voxels", run.stdout).group(1)) == int((d > 0).sum()) > filled


def test_the_flag_refuses_what_it_cannot_read(tmp_path, knight):
    exe = b.build_tools()
    path, _ = knight
    for bad in ("model.vox", "@1,2,3,0,1", f"{path}@1,2,3,0", f"{path}@1,2,3,0,1,5", f"{path}@1,2,3,0,0", f"{path}@1,2,3,0,-2", f"{path}@1,2,x,0,1", f"{path}@1,2,3,nan,1"):
        run = subprocess.run([str(exe), "--terrain", "7", "--paste", bad], capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--paste takes FILE.vox@X,Y,Z,YAW_DEG,SCALE" in run.stderr, (bad, run.stderr)
    run = subprocess.run([str(exe), "--terrain", "7", "--paste"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "missing value" in run.stderr


@pytest.mark.gpu
def test_the_flag_needs_a_terrain_a_file_and_a_scale_it_can_hold(tmp_path, knight):
    exe = b.build_tools()
    path, _ = knight
    common = ["--size", "64x48", "--frames", "1", "--out", str(tmp_path / "f.ppm")]
    for args, text in ((["--n", "64", "--paste", f"{path}@1,2,3,0,1"], "--paste needs a terrain"),
                       (["--terrain", "7", "--terrain-size", "32", "--paste", f"{tmp_path / 'none.vox'}@1,2,3,0,1"], "Failed to load VOX"),
                       (["--terrain", "7", "--terrain-size", "32", "--paste", f"{path}@1,2,3,0,0.01"], "SCALE must be at least 1/64")):
        run = subprocess.run([str(exe)] + common + args, capture_output=True, text=True, timeout=300)
        assert run.returncode == 1 and text in run.stderr, (args, run.stderr)
