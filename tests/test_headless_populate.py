"""The headless driver's --populate (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: columnField, scatterModels, downloadScatter,
stampModels): the printed counts against the host builds (blok_amd/columns.py) over the terrain evaluated on the host, with two .vox models
written here; with --bake the stamped voxels and the world's voxel count against blok_stamp_voxels.  The driver has no host path: the test
needs the device."""
import re
import subprocess

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import columns as K
from blok_amd import stamp as S
from blok_amd import terrain as T
from tests.test_vox import make_vox

SEED, SIZE = 7, 96          # the box of test_headless_seal.py

# (size, voxels (x, y, z up, colour index)): a small tree and a flat rock
TREE = ((3, 3, 5), [(1, 1, z, 10) for z in range(4)] + [(x, y, z, 20) for x in range(3) for y in range(3) for z in (3, 4) if (x, y, z) != (1, 1, 3)])
ROCK = ((4, 2, 2), [(x, y, z, 30) for x in range(4) for y in range(2) for z in range(2) if (x + y + z) % 4 != 3])


def local(model):
    """(xyz in the model's local lattice, y up; the anchor the driver gives it: the centre of its base)."""
    size, voxels = model
    return np.array([(x, z, y) for x, y, z, _ in voxels], np.int32), (size[0] // 2, 0, size[1] // 2)


@pytest.mark.gpu
def test_driver_scatters_models_over_the_terrain_and_bakes_them(tmp_path):
    exe = b.build_tools()
    paths = []
    for name, model in (("tree", TREE), ("rock", ROCK)):
        paths.append(tmp_path / f"{name}.vox")
        paths[-1].write_bytes(make_vox([model]))
    common = ["--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1"]
    plain = subprocess.run([str(exe)] + common + ["--out", str(tmp_path / "plain.ppm")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    populate = ["--populate", ",".join(str(p) for p in paths)]
    traced = subprocess.run([str(exe)] + common + populate + ["--out", str(tmp_path / "traced.ppm")], capture_output=True, text=True, timeout=300)
    assert traced.returncode == 0, traced.stderr
    baked = subprocess.run([str(exe)] + common + populate + ["--bake", "--out", str(tmp_path / "baked.ppm")], capture_output=True, text=True, timeout=300)
    assert baked.returncode == 0, baked.stderr
    # the same chain on the host; the driver's palette gives the terrain's materials the ids 1..4, grass first
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    top, material, info = K.column_field_host(d, m, (0, 0, 0), None, None, 1, 0)
    models = [local(TREE), local(ROCK)]
    params = K.scatter_params(seed=SEED, flags=K.ROTATE | K.MIRROR, cell_log2=4, probability=40000, surface_material=1, radius=1, max_rise=1, max_drop=1)
    entries = K.scatter_entries([(i, 1, anchor, 0) for i, (_, anchor) in enumerate(models)])
    table, s = K.scatter_host(top, material, info, params, entries)
    s = s[0]
    want = [len(models), int(info["n_hit"][0]), int(info["n_columns"][0]), int(s["n_cells"]), int(s["n_placed"])] + [int(n) for n in s["n_rejected"]]
    assert want[4] > 0 and {int(r["model"]) for r in table} == {0, 1}, "this terrain takes both models"
    pattern = r"populate: (\d+) models over (\d+) of (\d+) columns, (\d+) cells, (\d+) placed, rejected (\d+) (\d+) (\d+) (\d+) (\d+)"
    for run in (traced, baked):
        line = re.search(pattern, run.stdout)
        assert line and "populate:" not in plain.stdout, run.stdout
        print(f"host builds: {want}; driver: {line.groups()}")
        assert [int(v) for v in line.groups()] == want, run.stdout
    # baked: the voxels blok_stamp_voxels writes for the same table, and the world they leave
    written = sum(S.stamp_voxels_host(d, m, (0, 0, 0), models[int(r["model"])][0], np.full(len(models[int(r["model"])][0]), 9, np.uint32), r, S.STAMP_SET, 1.0) for r in table)
    world = lambda out: int(re.search(r"world: (\d+) voxels", out).group(1))
    assert int(re.search(r", baked (\d+) voxels", baked.stdout).group(1)) == written > 0 and "baked" not in traced.stdout
    assert world(baked.stdout) == int((d > 0).sum()) > filled and world(traced.stdout) == world(plain.stdout) == filled
    # the models show, as instances and as stamped voxels: both frames differ from the bare terrain's
    frames = [(tmp_path / f"{n}.ppm").read_bytes() for n in ("plain", "traced", "baked")]
    assert frames[1] != frames[0] and frames[2] != frames[0]
