"""The headless driver's --far-direct and --far-rings (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: reduceTerrain, lodModel,
setModelScale, with the fine box in place and no volume made for the ring): the same lines and the same image as --far, the rings' counts
against the host build (blok_amd/lod.py: terrain_reduce_host), and the refused arguments.  The driver has no host path: the test needs
the device.  The arguments are those of tests/test_headless_far.py."""
import re
import subprocess

import pytest

from blok_amd import build as b
from blok_amd import lod as L
from blok_amd import terrain as T

SEED, SIZE = 7, 96
K, MIN = 2, 3
LINE = r"far: box \((-?\d+),(-?\d+),(-?\d+)\): (\d+) voxels at level (\d+)"


def far_lines(text):
    return [tuple(int(v) for v in g) for g in re.findall(LINE, text)]


@pytest.mark.gpu
def test_driver_builds_the_same_ring_directly_and_further_rings(tmp_path):
    exe = b.build_tools()
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1"]

    def run(extra, out):
        return subprocess.run([str(exe)] + common + extra + ["--out", str(tmp_path / out)], capture_output=True, text=True, timeout=300)

    far = run(["--far", f"{K},{MIN}"], "far.ppm")
    assert far.returncode == 0, far.stderr
    direct = run(["--far", f"{K},{MIN}", "--far-direct"], "direct.ppm")
    assert direct.returncode == 0, direct.stderr
    print(f"--far: {far_lines(far.stdout)}; --far-direct: {far_lines(direct.stdout)}")
    assert len(far_lines(far.stdout)) == 8 and far_lines(direct.stdout) == far_lines(far.stdout)
    assert (tmp_path / "direct.ppm").read_bytes() == (tmp_path / "far.ppm").read_bytes()
    assert re.findall(r"far: instances won (\d+) of (\d+) pixels", direct.stdout) == re.findall(r"far: instances won (\d+) of (\d+) pixels", far.stdout)
    # the ring is built after the fine box: its lines follow the world's
    assert direct.stdout.index("world:") < direct.stdout.index("far: box") and far.stdout.index("far: box") < far.stdout.index("world:")
    # two rings: 8 + 16 boxes, ring r at level K + r - 1, the counts the host build's
    rings = run(["--far", f"{K},{MIN}", "--far-rings", "2"], "rings.ppm")
    assert rings.returncode == 0, rings.stderr
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    want = []
    for r in (1, 2):
        level = min(K + r - 1, 5)
        for dz in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if max(abs(dx), abs(dz)) != r:
                    continue
                origin = (dx * SIZE, 0, dz * SIZE)
                levels, _ = L.terrain_reduce_host(p, origin, (origin[0] + SIZE, SIZE, origin[2] + SIZE), level, L.VOTE_EXPOSED)
                want.append((origin[0], origin[1], origin[2], int((levels[level - 1][0] >= min(MIN, 8 ** level)).sum()), level))
    got = far_lines(rings.stdout)
    print(f"host build: {want}; driver: {got}")
    assert len(got) == 24 and got == want and got[:8] == far_lines(far.stdout)
    for args in (common + ["--far-direct"], common + ["--far", "2", "--far-rings", "0"], common + ["--far", "2", "--far-rings", "4"]):
        bad = subprocess.run([str(exe)] + args + ["--out", str(tmp_path / "bad.ppm")], capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0, args
