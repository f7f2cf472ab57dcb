"""The headless driver's --save-volume and --load-volume (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: encodeBricks,
downloadBricks, decodeBricks; blok_bricks_write_file / blok_bricks_read_file): the saved line against the numpy reference
(tests/bricks_reference.py) over the terrain evaluated on the host, the file against the reference's stream, and the loaded run's frame
against the saving run's."""
import re
import subprocess

import pytest

from blok_amd import bricks as B
from blok_amd import build as b
from blok_amd import terrain as T
from tests import bricks_reference as R

SEED, SIZE = 7, 96          # the box of test_headless_settle.py


@pytest.mark.gpu
def test_driver_saves_a_terrain_and_a_loaded_run_draws_the_same_frame(tmp_path):
    exe = b.build_tools()
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "2"]
    bvol = tmp_path / "world.bvol"
    saved = subprocess.run([str(exe)] + common + ["--save-volume", str(bvol), "--out", str(tmp_path / "saved.ppm")], capture_output=True, text=True, timeout=300)
    assert saved.returncode == 0, saved.stderr
    # the terrain on the host; the driver's palette gives the four materials the ids 1..4 in the order grass, soil, rock, ore
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    want = R.encode(d, m, (0, 0, 0))
    assert int(want[0]["n_voxels"][0]) == filled > 0 and 0 < R.stream_bytes(want) < d.nbytes + m.nbytes
    line = re.search(r"volume saved: (\d+) bricks, (\d+) voxels, (\d+) bytes", saved.stdout)
    assert line, saved.stdout
    assert tuple(int(v) for v in line.groups()) == (len(want[1]), filled, R.stream_bytes(want)), saved.stdout
    assert bvol.stat().st_size == R.stream_bytes(want)
    assert R.same_stream(B.read_file(bvol), want)
    # the loaded run generates nothing: it reads, decodes and rebuilds; --terrain only places the camera where the saving run's stood
    loaded = subprocess.run([str(exe), "--load-volume", str(bvol)] + common + ["--out", str(tmp_path / "loaded.ppm")], capture_output=True, text=True, timeout=300)
    assert loaded.returncode == 0, loaded.stderr
    assert "terrain:" not in loaded.stdout and re.search(rf"volume loaded: {len(want[1])} bricks, {filled} voxels; world: {filled} voxels", loaded.stdout), loaded.stdout
    assert (tmp_path / "loaded.ppm").read_bytes() == (tmp_path / "saved.ppm").read_bytes()
    # a damaged file is refused before anything reaches the device
    (tmp_path / "cut.bvol").write_bytes(bvol.read_bytes()[:-4])
    cut = subprocess.run([str(exe), "--load-volume", str(tmp_path / "cut.bvol"), "--frames", "1", "--out", str(tmp_path / "cut.ppm")], capture_output=True, text=True, timeout=300)
    assert cut.returncode == 1 and "Failed to load volume" in cut.stderr and not (tmp_path / "cut.ppm").exists()
