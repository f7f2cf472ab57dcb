"""The headless driver's --model-lights (tools/blok_headless.cpp over include/blok/hip_tracer.hpp: modelLights, instanceLightsInfo,
drawFrameRTInstanced): a lantern .vox written here is scattered over a small terrain by --populate, its head's material made to glow by
--glow, and the path-traced frames sample every copy as a light.  The written PPM goes against the Python API — the same material library,
terrain, model, scatter, rebuild, blok_amd.lights.model_lights and draw_frame_rt_instanced at the camera the driver prints, after the same
number of frames — byte for byte; the log line against the Python entry's counts; and the flag's refusals."""
import re
import subprocess

import numpy as np
import pytest

from blok_amd import build as b
from blok_amd import columns as K
from blok_amd import lights as LT
from blok_amd import terrain as T
from blok_amd._ffi import CAMERA
from blok_amd.vox import MaterialLibrary, VoxFile
from tests.test_vox import make_vox

SEED, SIZE, WD, HT, SPP = 7, 96, 64, 48, 2
POST, HEAD = 10, 20                       # colour indices: a grey post two voxels high, a 3 x 3 x 2 head on it
LANTERN = ((3, 3, 4), [(1, 1, z, POST) for z in range(2)] + [(x, y, z, HEAD) for x in range(3) for y in range(3) for z in (2, 3)])


def library_and_model(path):
    """The driver's material library (the terrain's four materials, then the .vox file's palette) and the model as the driver loads it:
    (library, terrain material ids, xyz with VOX z up -> local y, material ids, the anchor at the centre of the base)."""
    lib = MaterialLibrary()
    ids = []
    for name, rgb, emission in (("grass", (0.25, 0.62, 0.20), 0.0), ("soil", (0.45, 0.30, 0.16), 0.0), ("rock", (0.50, 0.50, 0.52), 0.0), ("ore", (1.0, 0.55, 0.10), 4.0)):
        d = MaterialLibrary.new_desc()
        d["albedo"][0] = rgb
        if emission > 0.0:
            d["emission"][0], d["emission_power"][0], d["type"][0] = rgb, emission, 3
        d["name"][0] = name.encode()
        ids.append(lib.add_material(d))
    vox = VoxFile.load_file(path)
    size, v = vox.model(0)
    mapping = vox.import_materials(lib)
    xyz = np.stack([v[:, 0], v[:, 2], v[:, 1]], axis=1).astype(np.int32)
    return lib, ids, xyz, mapping[v[:, 3]].astype(np.uint32), (size[0] // 2, 0, size[1] // 2), int(mapping[HEAD])


@pytest.mark.gpu
def test_driver_lights_the_terrain_with_scattered_lanterns_like_the_python_api(tmp_path):
    from blok_amd.tracer import HipTracer
    exe = b.build_tools()
    path = tmp_path / "lantern.vox"
    path.write_bytes(make_vox([LANTERN]))
    lib, terrain_ids, xyz, ids, anchor, glow = library_and_model(path)
    common = [str(exe), "--terrain", str(SEED), "--terrain-size", str(SIZE), "--size", f"{WD}x{HT}", "--frames", "1", "--spp", str(SPP), "--rt", "--populate", str(path),
              "--glow", str(glow)]
    out = tmp_path / "lit.ppm"
    run = subprocess.run(common + ["--model-lights", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    plain = subprocess.run(common + ["--out", str(tmp_path / "plain.ppm")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "model lights:" not in plain.stdout, plain.stderr
    line = re.search(r"model lights: (\d+) models, (\d+) faces; (\d+) instances, (\d+) lit, (\d+) faces in the world\n", run.stdout)
    assert line, run.stdout
    cam = np.zeros(1, dtype=CAMERA)
    cam.view(np.float32)[:] = [np.float32(v) for v in re.search(r"model lights: camera (.*)", run.stdout).group(1).split()]
    # the same chain through the Python API
    p = T.default_params(SIZE, SEED)
    p.surface_material, p.soil_material, p.rock_material, p.ore_material = terrain_ids
    tr = HipTracer(WD, HT).init()
    tr.volume_create((0, 0, 0), (SIZE, SIZE, SIZE))
    tr.volume_generate_terrain(p)
    model = tr.model_create(xyz, ids)
    tr.volume_column_field(None, None, 1, 0)
    params = K.scatter_params(seed=SEED, flags=K.ROTATE | K.MIRROR, cell_log2=4, probability=40000, surface_material=terrain_ids[0], radius=1, max_rise=1, max_drop=1)
    tr.volume_scatter_models(params, K.scatter_entries([(model, 1, anchor, 0)]))
    inst = tr.volume_scatter_download()
    mats = lib.pack_for_gpu()
    mats["emission"][glow] = np.float32(4.0) * mats["albedo"][glow]
    tr.volume_rebuild(mats)
    plain_py = [tr.draw_frame_rt(cam, SPP, 2)[0] for _ in range(2)][-1]
    tr.post_reset()
    faces = int(LT.model_lights(tr, model)["n"][0])
    header, icum = LT.instance_lights_info(tr, inst)
    want = [1, faces, len(inst), int(header["n_lit"][0]), int(header["a_inst"][0])]
    print(f"python entry: {want}; driver: {line.groups()}")
    assert [int(v) for v in line.groups()] == want
    assert faces == 9 + 12 * 2 + 8 and len(inst) > 0 and want[3] == len(inst) and want[4] == faces * len(inst)      # the head's top, sides and the rim under it
    for _ in range(2):
        rgba, frames = tr.draw_frame_rt_instanced(cam, inst, SPP, 2)
    assert frames == 2
    tr.shutdown()

    def body(data):
        head = f"P6\n{WD} {HT}\n255\n".encode()
        assert data.startswith(head)
        return data[len(head):]

    as_rgb = lambda px: np.stack([px & 255, (px >> 8) & 255, (px >> 16) & 255], axis=-1).astype(np.uint8).tobytes()
    assert body(out.read_bytes()) == as_rgb(rgba)
    # without the flag --rt shows the world alone, as before
    assert body((tmp_path / "plain.ppm").read_bytes()) == as_rgb(plain_py)
    assert as_rgb(rgba) != as_rgb(plain_py)


def test_the_flag_is_refused_when_nothing_is_placed(tmp_path):
    exe = b.build_tools()
    for args in (["--terrain", "7", "--rt", "--model-lights"], ["--terrain", "7", "--populate", "m.vox", "--model-lights"],
                 ["--terrain", "7", "--rt", "--populate", "m.vox", "--bake", "--model-lights"], ["--n", "64", "--rt", "--model-lights"]):
        run = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--model-lights samples the placed models' emissive faces" in run.stderr and "--populate" in run.stderr, (args, run.stderr)
