"""The headless driver's --stroke (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: strokeShapes, applyShapes): the printed count
and the world's voxel count against the Python path (blok_amd/shapes.py: stroke and apply_host over the terrain evaluated on the host),
and the frame against the frame of the same arrays written by the Python path as a .bvol file and loaded by the driver: the hash of
what a dug terrain looks like comes from the host build, not from the kernel under test."""
import hashlib
import re
import subprocess

import numpy as np
import pytest

from blok_amd import bricks as B
from blok_amd import build as b
from blok_amd import shapes as SH
from blok_amd import terrain as T

SEED, SIZE = 7, 96          # the box of test_headless_settle.py
POINTS = ((10.5, 60.5, 12.5), (40.5, 28.5, 30), (60, 34.5, 70.5), (90.5, 20.5, 99.5))      # from above the ground (14 .. 43 high), through it, out of the box's +z face
RADIUS = 5.5


@pytest.mark.gpu
def test_driver_digs_a_stroke_through_a_terrain(tmp_path):
    exe = b.build_tools()
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1"]
    arg = ":".join(",".join(str(c) for c in p) for p in POINTS) + f",{RADIUS},subtract"
    run = subprocess.run([str(exe)] + common + ["--stroke", arg, "--out", str(tmp_path / "stroke.ppm")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    # the terrain on the host; the driver's palette gives the four materials the ids 1..4 in the order grass, soil, rock, ore
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    d, m = np.ascontiguousarray(d), np.ascontiguousarray(m)
    table = SH.stroke(POINTS, RADIUS, SH.SUBTRACT, value=0.0)
    written = SH.apply_host(d, m, (0, 0, 0), table)
    left = int((d > 0).sum())
    assert len(table) == 3 and written > 1000 and 0 < left < filled - 500      # the brush meets the ground
    want = f"stroke: 3 capsules, {written} voxels written"
    line = re.search(r"^stroke: .*$", run.stdout, re.M)
    print(f"host build: {want}; driver: {line and line.group(0)}")
    assert line and line.group(0) == want, run.stdout
    assert int(re.search(r"world: (\d+) voxels", run.stdout).group(1)) == left
    # the frame: the host build's arrays as a .bvol file, loaded by the driver, drawn from where the terrain's camera stands
    bvol = tmp_path / "dug.bvol"
    B.write_file(bvol, *B.encode_host(d, m, (0, 0, 0)))
    loaded = subprocess.run([str(exe), "--load-volume", str(bvol)] + common + ["--out", str(tmp_path / "loaded.ppm")], capture_output=True, text=True, timeout=300)
    assert loaded.returncode == 0, loaded.stderr
    assert re.search(rf"world: {left} voxels", loaded.stdout), loaded.stdout
    frames = [(tmp_path / n).read_bytes() for n in ("stroke.ppm", "loaded.ppm")]
    print("frame sha256:", [hashlib.sha256(f).hexdigest()[:16] for f in frames])
    assert frames[0] == frames[1]
    # a malformed argument is refused before anything is made
    bad = subprocess.run([str(exe)] + common + ["--stroke", "1,2:3,4,5,2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--stroke takes" in bad.stderr
