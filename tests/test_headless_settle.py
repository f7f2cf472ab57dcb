"""The headless driver's --settle (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: labelComponents, captureComponent, sweepModels,
stampModels) on a small terrain: the printed line against the same procedure carried out with the numpy references
(tests/components_reference.py, tests/sweep_reference.py, tests/stamp_reference.py) on the terrain evaluated on the host."""
import re
import subprocess

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import terrain as T
from tests import components_reference as CR
from tests import stamp_reference as SR
from tests import sweep_reference as R

SEED, SIZE = 7, 96          # the box of test_headless_components.py: its caves leave two small floating pieces


def settled(d):
    """--settle on the array: (pieces, voxels, total travel, longest, components after, floating after), and --components' numbers before."""
    m = np.zeros(d.shape, dtype=np.uint32)
    origin = (0, 0, 0)
    pieces = voxels = total = longest = 0
    before = None
    for _ in range(8):
        labels, records = CR.label(d, origin)
        floating = records[records["touches"] & 8 == 0]
        if before is None:
            before = (len(records), int(records["n_voxels"].sum()), int(records["n_voxels"].max()), len(floating), int(floating["n_voxels"].sum()))
        if len(floating) == 0:                                  # (this labelling is also the one after)
            return (pieces, voxels, total, longest, len(records), 0), before
        for rec in sorted(floating, key=lambda r: (int(r["lo"][1]), int(r["label"]))):
            xyz, mm, _ = CR.members(d, m, origin, (labels, None, None), rec)
            CR.clear_members(d, m, origin, (labels, None, None), rec)
            lo = tuple(int(c) for c in rec["lo"])
            _, travel, _ = R.sweep(d, origin, xyz, (lo, (0, 1, 2), 0), 3, SIZE, R.BOX_IS_SOLID)
            assert SR.stamp(d, m, origin, xyz, mm, ((lo[0], lo[1] - travel, lo[2]), (0, 1, 2), 0), SR.SET, 1.0) == len(mm)
            pieces, voxels, total, longest = pieces + 1, voxels + len(mm), total + travel, max(longest, travel)
    _, records = CR.label(d, origin)
    return (pieces, voxels, total, longest, len(records), int((records["touches"] & 8 == 0).sum())), before


@pytest.mark.gpu
def test_driver_settles_the_terrains_floating_pieces(tmp_path):
    exe = b.build_tools()
    proc = subprocess.run([str(exe), "--terrain", str(SEED), "--terrain-size", str(SIZE), "--components", "--settle", "--size", "64x48",
                           "--frames", "1", "--out", str(tmp_path / "frame.ppm")], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    d, _, filled = T.eval_box(T.default_params(SIZE, SEED), (0, 0, 0), (SIZE, SIZE, SIZE))
    d = np.ascontiguousarray(d, dtype=np.float32).copy()
    want, before = settled(d)
    assert int((d > 0).sum()) == filled == before[1]            # nothing is lost on the way down
    assert want[0] >= 2 and want[2] > 0 and want[5] == 0, want  # the case is worth running: pieces fall, and all come to rest
    got = re.search(r"settle: (\d+) pieces, (\d+) voxels, travel (\d+) in total, longest (\d+); (\d+) components after, (\d+) not touching the floor",
                    proc.stdout)
    assert got, proc.stdout
    assert tuple(int(v) for v in got.groups()) == want, proc.stdout
    # --components' own line is what it was
    line = re.search(r"components: (\d+) over (\d+) voxels, largest (\d+) voxels, (\d+) not touching the floor \((\d+) voxels\)", proc.stdout)
    assert line and tuple(int(v) for v in line.groups()) == before, proc.stdout
    assert proc.stdout.index("components:") < proc.stdout.index("settle:")
