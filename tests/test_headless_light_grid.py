"""The headless driver's --light-grid (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: buildLightGrid): a small terrain whose
grass glows is path-traced with --lights and with --lights --light-grid C,R,SHARE.  The log line's counts go against the Python entry over
the same terrain, material table and light table; the written frame against the Python entry's draw_frame_rt under the same grid at the
camera the driver prints, byte for byte, and different from the frame of --lights alone; and the flag's refusals."""
import re
import subprocess

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import lights as LT
from blok_amd import terrain as T
from blok_amd._ffi import CAMERA
from blok_amd.vox import MaterialLibrary

SEED, SIZE, WD, HT, SPP = 7, 64, 64, 48, 2
C, R, SHARE = 3, 1, 200


def terrain_library():
    """The driver's material library without a model: the terrain's four materials."""
    lib = MaterialLibrary()
    ids = []
    for name, rgb, emission in (("grass", (0.25, 0.62, 0.20), 0.0), ("soil", (0.45, 0.30, 0.16), 0.0), ("rock", (0.50, 0.50, 0.52), 0.0), ("ore", (1.0, 0.55, 0.10), 4.0)):
        d = MaterialLibrary.new_desc()
        d["albedo"][0] = rgb
        if emission > 0.0:
            d["emission"][0], d["emission_power"][0], d["type"][0] = rgb, emission, 3
        d["name"][0] = name.encode()
        ids.append(lib.add_material(d))
    return lib, ids


@pytest.mark.gpu
def test_driver_builds_the_grid_the_python_entry_builds(tmp_path):
    from blok_amd.tracer import HipTracer
    exe = b.build_tools()
    lib, ids = terrain_library()
    glow = ids[0]
    base = [str(exe), "--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", f"{WD}x{HT}", "--frames", "1", "--spp", str(SPP), "--rt", "--glow", str(glow), "--lights"]
    runs = {}
    for name, extra in (("grid", ["--light-grid", f"{C},{R},{SHARE}"]), ("table", [])):
        out = tmp_path / f"{name}.ppm"
        run = subprocess.run(base + extra + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        runs[name] = (run.stdout, out.read_bytes())
    assert "light grid:" not in runs["table"][0]
    table = re.search(r"lights: (\d+) rectangles, (\d+) faces", runs["grid"][0])
    line = re.search(r"light grid: (\d+) cells \((\d+) x (\d+) x (\d+) of (\d+) voxels, reach (\d+), share (\d+)/256\), (\d+) with a list, (\d+) items, the longest list (\d+)\n", runs["grid"][0])
    assert table and line, runs["grid"][0]
    # the same chain through the Python API
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = ids
    tr = HipTracer(WD, HT).init()
    tr.volume_create((0, 0, 0), (SIZE, SIZE, SIZE))
    tr.volume_generate_terrain(p)
    mats = lib.pack_for_gpu()
    mats["emission"][glow] = np.float32(4.0) * mats["albedo"][glow]
    tr.volume_rebuild(mats)
    tr.volume_extract_quads()
    lights = LT.from_quads(tr)
    g = LT.build_grid(tr, C, R, SHARE)
    host = LT.host_build_grid(LT.download(tr), C, R, SHARE)[3]
    cam = np.zeros(1, dtype=CAMERA)
    cam.view(np.float32)[:] = [np.float32(v) for v in re.search(r"light grid: camera (.*)", runs["grid"][0]).group(1).split()]
    rgba = [tr.draw_frame_rt(cam, SPP, 2)[0] for _ in range(2)][-1]
    tr.shutdown()
    assert g.tobytes() == host.tobytes()
    want = [int(g["n_cells"][0]), *[int(d) for d in g["dim"][0]], 1 << C, R, SHARE, int(g["n_nonempty"][0]), int(g["n_items"][0]), int(g["max_items"][0])]
    print(f"python entry: lights {int(lights['n'][0])} / {int(lights['n_faces'][0])}, grid {want}; driver: {table.groups()} {line.groups()}")
    assert [int(v) for v in table.groups()] == [int(lights["n"][0]), int(lights["n_faces"][0])]
    assert [int(v) for v in line.groups()] == want
    assert want[0] > 1 and want[8] >= int(lights["n"][0]) and want[9] >= 1
    head = f"P6\n{WD} {HT}\n255\n".encode()
    assert runs["grid"][1].startswith(head)
    as_rgb = np.stack([rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255], axis=-1).astype(np.uint8).tobytes()
    assert runs["grid"][1][len(head):] == as_rgb, "the driver's frame is the Python entry's under the same grid"
    assert len(runs["grid"][1]) == len(runs["table"][1]) and runs["grid"][1] != runs["table"][1], "the frames sample through the grid"


def test_the_flag_is_refused_without_lights_and_out_of_range():
    exe = b.build_tools()
    run = subprocess.run([str(exe), "--terrain", "7", "--terrain-size", "64", "--rt", "--light-grid", "4"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--light-grid is built over the light table: give --lights" in run.stderr, run.stderr
    for bad in ("1", "13", "4,4", "4,1,0", "4,1,256", "x"):
        run = subprocess.run([str(exe), "--terrain", "7", "--rt", "--lights", "--light-grid", bad], capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--light-grid takes C[,R[,SHARE]]" in run.stderr, (bad, run.stderr)
