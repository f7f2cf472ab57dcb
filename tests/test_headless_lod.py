"""The headless driver's --lod (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: reduceVolume, downloadLod; then
blok_hip_set_voxel_size + blok_hip_upload_dense): the printed counts against the host build (blok_amd/lod.py) over the terrain evaluated on
the host, and the frame of the coarse world against the plain terrain's.  The driver has no host path: the test needs the device."""
import re
import subprocess

import pytest

from blok_amd import build as b
from blok_amd import lod as L
from blok_amd import terrain as T

SEED, SIZE = 7, 96          # the box of test_headless_seal.py
K, MIN = 2, 3


@pytest.mark.gpu
def test_driver_renders_the_coarse_copy_of_the_terrain(tmp_path):
    exe = b.build_tools()
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1"]
    plain = subprocess.run([str(exe)] + common + ["--out", str(tmp_path / "plain.ppm")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    coarse = subprocess.run([str(exe)] + common + ["--lod", f"{K},{MIN}", "--out", str(tmp_path / "coarse.ppm")], capture_output=True, text=True, timeout=300)
    assert coarse.returncode == 0, coarse.stderr
    # the same reduction on the host; the driver's palette gives the terrain's materials the ids 1..4, grass first
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    levels, info = L.reduce_host(d, m, (0, 0, 0), None, None, K, L.VOTE_EXPOSED)
    top = info["level"][0][K - 1]
    voxels = int((levels[K - 1][0] >= MIN).sum())
    want = [K, int(top["n_filled"]), int(top["n_cells"]), int(top["n_exposed"]), voxels, MIN]
    assert int(top["sum_n"]) == filled and 0 < voxels < int(top["n_filled"]) < int(top["n_cells"]) == (SIZE >> K) ** 3, "MIN drops some cells of this terrain"
    line = re.search(r"lod: level (\d+): (\d+) of (\d+) cells filled, (\d+) exposed, (\d+) voxels at min (\d+)", coarse.stdout)
    assert line and "lod:" not in plain.stdout, coarse.stdout
    print(f"host build: {want}; driver: {line.groups()}")
    assert [int(v) for v in line.groups()] == want, coarse.stdout
    worlds = re.findall(r"world: (\d+) voxels", coarse.stdout)
    assert [int(w) for w in worlds] == [filled, voxels], coarse.stdout      # the terrain's world, then the coarse one in its place
    assert (tmp_path / "coarse.ppm").read_bytes() != (tmp_path / "plain.ppm").read_bytes()
    # only with --terrain, and K in 1 .. 5
    for args in (["--n", "64", "--lod", "2"], common + ["--lod", "6"], common + ["--lod", "2,65"]):
        bad = subprocess.run([str(exe)] + args + ["--frames", "1", "--out", str(tmp_path / "bad.ppm")], capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0, args
