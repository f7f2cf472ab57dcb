"""The headless driver's --hollow (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: distanceField, editByDistance): the printed
counts against the host build (blok_amd/distance.py) over the terrain evaluated on the host, the world's voxel count after the rebuild,
and the frames of the hollowed and the solid run, which must not differ.

Why the frames must match: the first filled cell on a primary ray is entered from an empty cell that touches it by a face, an edge or a
corner, so its D <= 3 and HOLLOW at d2 = 3 keeps it; cells on the box's faces are 1 from the empty outside; the camera of --terrain
stands in an empty cell."""
import re
import subprocess

import pytest

from blok_amd import build as b
from blok_amd import distance as D
from blok_amd import terrain as T

SEED, SIZE = 7, 96          # the box of test_headless_settle.py


@pytest.mark.gpu
def test_driver_hollows_a_terrain_and_draws_the_same_frame(tmp_path):
    exe = b.build_tools()
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "2"]
    solid = subprocess.run([str(exe)] + common + ["--out", str(tmp_path / "solid.ppm")], capture_output=True, text=True, timeout=300)
    assert solid.returncode == 0, solid.stderr
    hollow = subprocess.run([str(exe)] + common + ["--hollow", "3", "--out", str(tmp_path / "hollow.ppm")], capture_output=True, text=True, timeout=300)
    assert hollow.returncode == 0, hollow.stderr
    # the terrain on the host; the driver's palette gives the four materials the ids 1..4 in the order grass, soil, rock, ore
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    field = D.distance_field_host(d, (0, 0, 0), None, None, 2, D.TO_EMPTY)
    cleared = D.distance_edit_host(d, m, (0, 0, 0), *field, D.HOLLOW, 3)
    left = int((d > 0).sum())
    assert 0 < cleared and left == filled - cleared
    line = re.search(r"hollow: (\d+) voxels cleared, (\d+) left", hollow.stdout)
    assert line and "hollow:" not in solid.stdout, hollow.stdout
    print(f"host build: {cleared} cleared, {left} left of {filled}; driver: {line.groups()}")
    assert tuple(int(v) for v in line.groups()) == (cleared, left), hollow.stdout
    world = lambda out: int(re.search(r"world: (\d+) voxels", out).group(1))
    assert world(hollow.stdout) == left < world(solid.stdout) == filled
    assert (tmp_path / "hollow.ppm").read_bytes() == (tmp_path / "solid.ppm").read_bytes()
