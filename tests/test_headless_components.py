"""The headless driver's --components (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: labelComponents) on a small terrain: the
printed counts against the numpy reference (tests/components_reference.py) on the same terrain, evaluated on the host."""
import re
import subprocess

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import terrain as T
from tests import components_reference as R

SEED, SIZE = 7, 96          # the smallest of the tried boxes whose caves leave more than one component


@pytest.mark.gpu
def test_driver_counts_the_terrains_components(tmp_path):
    exe = b.build_tools()
    proc = subprocess.run([str(exe), "--terrain", str(SEED), "--terrain-size", str(SIZE), "--components", "--size", "64x48", "--frames", "1",
                           "--out", str(tmp_path / "frame.ppm")], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    # the driver's terrain: the default parameters of the box; material ids play no part in what hangs together
    d, _, filled = T.eval_box(T.default_params(SIZE, SEED), (0, 0, 0), (SIZE, SIZE, SIZE))
    _, records = R.label(d)
    assert int(records["n_voxels"].sum()) == filled and len(records) >= 3
    floating = records[records["touches"] & 8 == 0]
    want = (len(records), filled, int(records["n_voxels"].max()), len(floating), int(floating["n_voxels"].sum()))
    got = re.search(r"components: (\d+) over (\d+) voxels, largest (\d+) voxels, (\d+) not touching the floor \((\d+) voxels\)", proc.stdout)
    assert got, proc.stdout
    assert tuple(int(v) for v in got.groups()) == want, proc.stdout

