"""The headless driver's --scroll (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: volumeScroll, generateTerrain into the exposed
boxes): the printed counts against the host builds (blok_amd/scroll.py over the terrain evaluated on the host, blok_amd/terrain.py over
each exposed box), and the world's voxel count after the rebuild against the same terrain evaluated whole where the box now is — the
terrain is a function of the world voxel, so a scrolled and refilled box holds what a box generated there would."""
import re
import subprocess

import pytest

from blok_amd import build as b
from blok_amd import scroll as S
from blok_amd import terrain as T

SEED, SIZE = 7, 96          # the box of test_headless_settle.py
DELTA = (16, 0, -24)


@pytest.mark.gpu
def test_driver_scrolls_a_terrain_and_refills_what_came_into_view(tmp_path):
    exe = b.build_tools()
    run = subprocess.run([str(exe), "--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1", "--scroll", ",".join(map(str, DELTA)),
                          "--out", str(tmp_path / "scrolled.ppm")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    # the terrain on the host; the driver's palette gives the four materials the ids 1..4 in the order grass, soil, rock, ore
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    d, m, filled = T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))
    _, _, info = S.scroll_voxels_host(d, m, (0, 0, 0), DELTA)
    rec = info[0]
    assert int(rec["n_filled_before"]) == filled
    exposed = S.boxes(info, "exposed")
    generated = sum(T.eval_box(p, lo, hi)[2] for lo, hi in exposed)
    lost = filled - int(rec["n_filled_kept"])
    assert len(exposed) == 2 and generated > 0 and lost > 0
    want = f"scroll: origin {DELTA[0]} {DELTA[1]} {DELTA[2]}, kept {int(rec['n_cells_kept'])} cells, lost {lost} filled voxels, exposed 2 boxes, generated {generated} voxels"
    line = re.search(r"^scroll: .*$", run.stdout, re.M)
    print(f"host builds: {want}; driver: {line and line.group(0)}")
    assert line and line.group(0) == want, run.stdout
    whole = T.eval_box(p, DELTA, tuple(c + SIZE for c in DELTA))[2]
    assert whole == int(rec["n_filled_kept"]) + generated
    assert int(re.search(r"world: (\d+) voxels", run.stdout).group(1)) == whole
