"""The headless driver's --lights and --glow (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: lightsFromQuads): a small terrain
whose first four materials (the terrain's own are among them) are made to glow is path-traced with and without the light table; the log line, and an image that differs."""
import re
import subprocess

import pytest

from blok_amd import build as b


@pytest.mark.gpu
def test_driver_builds_the_light_table_and_the_frame_changes(tmp_path):
    exe = b.build_tools()
    base = [str(exe), "--terrain", "7", "--terrain-size", "64", "--size", "64x48", "--frames", "1", "--spp", "2", "--rt", "--glow", "0:0.8,1.5,3.0", "--glow", "1", "--glow", "2", "--glow", "3:0.5,0.5,0.1"]
    images = {}
    for name, extra in (("lit", ["--lights"]), ("unlit", [])):
        out = tmp_path / f"{name}.ppm"
        run = subprocess.run(base + extra + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        assert "path trace" in run.stdout
        line = re.search(r"lights: (\d+) rectangles, (\d+) faces, (\d+) materials", run.stdout)
        assert (line is not None) == (name == "lit"), run.stdout
        if line:
            n, faces, owned = map(int, line.groups())
            assert n >= 1 and faces >= n and owned >= 1
        images[name] = out.read_bytes()
    assert len(images["lit"]) == len(images["unlit"]) and images["lit"] != images["unlit"]


def test_the_flags_refusals(tmp_path):
    exe = b.build_tools()
    run = subprocess.run([str(exe), "--terrain", "7", "--terrain-size", "64", "--lights"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--lights is sampled by the path-traced frames" in run.stderr, run.stderr
    run = subprocess.run([str(exe), "--terrain", "7", "--glow", "x"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--glow takes ID or ID:R,G,B" in run.stderr, run.stderr
