"""The headless driver's --smooth and --rule (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: volumeAutomaton): the printed info
line against the host build (blok_amd/automaton.py) over the terrain evaluated on the host, and the world's voxel count after the
rebuild."""
import re
import subprocess

import pytest

from blok_amd import automaton as A
from blok_amd import build as b
from blok_amd import terrain as T

SEED, SIZE = 7, 96          # the box of test_headless_hollow.py


def terrain():
    """The terrain on the host; the driver's palette gives the four materials the ids 1..4 in the order grass, soil, rock, ore."""
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = 1, 2, 3, 4
    return T.eval_box(p, (0, 0, 0), (SIZE, SIZE, SIZE))


@pytest.mark.gpu
@pytest.mark.parametrize("flags,rule", [(["--smooth", "2"], A.smooth(2)),
                                        (["--rule", "18,7FE00,7FC00,3,solid"], A.rule(18, A.at_least(9, 18), A.at_least(10, 18), steps=3, box_is_solid=True))],
                         ids=["smooth", "rule"])
def test_driver_steps_a_rule_over_the_terrain(tmp_path, flags, rule):
    exe = b.build_tools()
    run = subprocess.run([str(exe), "--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "frame.ppm")] + flags,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    d, m, filled = terrain()
    hd, _, info, _ = A.automaton_host(d, m, rule)
    want = tuple(int(info[k][0]) for k in ("steps_run", "n_born", "n_died", "n_filled"))
    assert want[1] > 0 and want[2] > 0 and want[3] == int((hd > 0).sum()) == filled + want[1] - want[2]
    line = re.search(r"rule: (\d+) steps run, (\d+) voxels born, (\d+) died, (\d+) left", run.stdout)
    assert line, run.stdout
    print(f"host build: {want}; driver: {line.groups()}")
    assert tuple(int(v) for v in line.groups()) == want, run.stdout
    assert int(re.search(r"world: (\d+) voxels", run.stdout).group(1)) == want[3]


def test_driver_refuses_a_malformed_rule():
    exe = b.build_tools()
    for flags in (["--rule", "7,0,0,1"], ["--rule", "26,7FFE000,7FFC000"], ["--rule", "6,FF,0,1"], ["--smooth", "0"], ["--smooth", "256"], ["--smooth", "2x"],
                  ["--rule", "26,0,0,1,hollow"]):
        run = subprocess.run([str(exe), "--terrain", "7"] + flags, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--rule takes" in run.stderr, (flags, run.stderr)
