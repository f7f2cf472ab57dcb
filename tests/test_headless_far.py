"""The headless driver's --far (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: createVolume at each neighbour's place,
generateTerrain, reduceVolume, lodModel, setModelScale; the ring traced as instances of scaled models beside the fine box): the printed
per-neighbour counts against the host build (blok_amd/terrain.py, blok_amd/lod.py), the pixels the ring wins, and the frame against the
plain terrain's.  The driver has no host path: the test needs the device."""
import re
import subprocess

import pytest

from blok_amd import build as b
from blok_amd import lod as L
from blok_amd import terrain as T

SEED, SIZE = 7, 96          # the box of test_headless_lod.py
K, MIN = 2, 3


@pytest.mark.gpu
def test_driver_shows_the_ring_of_coarse_copies_beside_the_fine_box(tmp_path):
    exe = b.build_tools()
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1"]
    plain = subprocess.run([str(exe)] + common + ["--out", str(tmp_path / "plain.ppm")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    far = subprocess.run([str(exe)] + common + ["--far", f"{K},{MIN}", "--out", str(tmp_path / "far.ppm")], capture_output=True, text=True, timeout=300)
    assert far.returncode == 0, far.stderr
    # the same ring on the host; the driver's palette gives the terrain's materials the ids 1..4, grass first
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    want = []
    for dz in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dz == 0:
                continue
            origin = (dx * SIZE, 0, dz * SIZE)
            d, m, _ = T.eval_box(p, origin, (origin[0] + SIZE, SIZE, origin[2] + SIZE))
            levels, _ = L.reduce_host(d, m, origin, None, None, K, L.VOTE_EXPOSED)
            want.append((origin[0], origin[1], origin[2], int((levels[K - 1][0] >= MIN).sum()), K))
    got = [tuple(int(v) for v in g) for g in re.findall(r"far: box \((-?\d+),(-?\d+),(-?\d+)\): (\d+) voxels at level (\d+)", far.stdout)]
    print(f"host build: {want}; driver: {got}")
    assert got == want and "far:" not in plain.stdout, far.stdout
    assert sum(w[3] > 0 for w in want) >= 4
    won = re.search(r"far: instances won (\d+) of (\d+) pixels", far.stdout)
    assert won and int(won.group(2)) == 64 * 48 and int(won.group(1)) > 0, far.stdout
    assert (tmp_path / "far.ppm").read_bytes() != (tmp_path / "plain.ppm").read_bytes()
    assert re.findall(r"world: (\d+) voxels", far.stdout) == re.findall(r"world: (\d+) voxels", plain.stdout)       # the fine box is the world, as it was
    # only with --terrain, K in 1 .. 5, MIN at most 8^K
    for args in (["--n", "64", "--far", "2"], common + ["--far", "6"], common + ["--far", "2,65"]):
        bad = subprocess.run([str(exe)] + args + ["--frames", "1", "--out", str(tmp_path / "bad.ppm")], capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0, args
