"""The headless driver's --seal (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: floodField, editByFlood): the printed counts
against the host build (blok_amd/flood.py) over the terrain evaluated on the host — a small terrain with caves, some of which no air from
the box's faces reaches — and the world's voxel count after the rebuild.  The driver has no host path: the test needs the device."""
import re
import subprocess

import pytest

from blok_amd import build as b
from blok_amd import flood as F
from blok_amd import terrain as T

SEED, SIZE = 7, 96          # the box of test_headless_hollow.py


@pytest.mark.gpu
def test_driver_seals_the_caves_air_cannot_reach(tmp_path):
    exe = b.build_tools()
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1"]
    open_ = subprocess.run([str(exe)] + common + ["--out", str(tmp_path / "open.ppm")], capture_output=True, text=True, timeout=300)
    assert open_.returncode == 0, open_.stderr
    sealed = subprocess.run([str(exe)] + common + ["--seal", "--seal-material", "3", "--out", str(tmp_path / "sealed.ppm")], capture_output=True, text=True, timeout=300)
    assert sealed.returncode == 0, sealed.stderr
    # the terrain on the host; the driver's palette gives the four materials the ids 1..4 in the order grass, soil, rock, ore
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    steps, info = F.flood_field_host(d, m, (0, 0, 0), None, None, None, F.MAX_STEPS, F.ALL_FACES)
    farthest = int(info["farthest"][0])
    assert farthest < F.MAX_STEPS, "the flood ended on its own"
    n = F.flood_edit_host(d, m, (0, 0, 0), steps, info, F.FILL_UNREACHED, 0, 1.0, 3)
    assert n == int(info["n_unreached"][0]) > 0, "this terrain has caves that air from the faces does not reach"
    line = re.search(r"seal: (\d+) voxels filled, farthest (\d+)", sealed.stdout)
    assert line and "seal:" not in open_.stdout, sealed.stdout
    print(f"host build: {n} filled, farthest {farthest}; driver: {line.groups()}")
    assert tuple(int(v) for v in line.groups()) == (n, farthest), sealed.stdout
    world = lambda out: int(re.search(r"world: (\d+) voxels", out).group(1))
    assert world(sealed.stdout) == filled + n == int((d > 0).sum()) and world(open_.stdout) == filled
    # no primary ray enters a sealed cell: the camera stands in air the faces reach
    assert (tmp_path / "sealed.ppm").read_bytes() == (tmp_path / "open.ppm").read_bytes()
