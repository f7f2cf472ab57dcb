"""CPU: emissive models as lights (include/blok_hip.h, "emissive models as lights"; include/blok_world.h: blok_model_lights,
blok_instance_light_record).  The host build against the numpy model of tests/model_lights_reference.py over tests/model_lights_cases.py;
the record map over all 48 orientations against the world voxels tests/instance_oracle.py maps a cell to; the prefix rule with its
overflow pair; the ABI; and the stand-alone program of tests/host_harness/model_lights_main.cpp under ASan + UBSan."""
from __future__ import annotations

import os
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import lights as LT
from blok_amd._ffi import HIT, INSTANCE, LIGHT
from tests import instance_oracle as IO
from tests import model_lights_cases as MC
from tests import model_lights_reference as MR

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
CASES = MC.table()


def test_abi_symbols_sizes_and_version():
    header = (ROOT / "include" / "blok_hip.h").read_text()
    for name in ("blok_hip_model_lights", "blok_hip_model_lights_info", "blok_hip_model_lights_download", "blok_hip_model_lights_clear",
                 "blok_hip_instance_lights_info"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _ffi.HIP_SYMBOLS
        assert hasattr(_ffi.hip_lib(), name)
    for name in ("blok_model_lights", "blok_instance_light_record"):
        assert name in _ffi.HOST_SYMBOLS and hasattr(_ffi.host_lib(), name)
    assert _ffi.INSTANCE_LIGHTS_INFO.itemsize == 32
    version = _ffi.hip_lib().blok_hip_abi_version()
    assert version >> 16 == 1 and version & 0xFFFF >= 28
    assert "1.28:" in header
    mirror = (ROOT / "include" / "blok" / "hip_tracer.hpp").read_text()
    assert "blok_hip_model_lights" in mirror and "blok_hip_instance_lights_info" in mirror


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_build_equals_the_numpy_model(case):
    got = LT.host_model_lights(case.xyz, case.ids, case.materials)
    faces = MR.model_faces(case.xyz, case.ids, case.materials)
    print(f"{case.name}: {len(case.xyz)} voxels -> {len(got)} faces")
    if case.n_faces is not None:
        assert len(faces) == case.n_faces
    else:
        assert len(faces) > 600
    assert len(got) == len(faces)
    assert (got["du"] == 1).all() and (got["dv"] == 1).all()
    assert got["cum"].tolist() == list(range(len(got)))
    # the set: the voxel is lo with the + faces' plane taken back
    plus = np.stack([got["face"] == 0, got["face"] == 2, got["face"] == 4], axis=1)
    voxel = got["lo"].astype(np.int64) - plus
    assert {(int(v[0]), int(v[1]), int(v[2]), int(f), int(m)) for v, f, m in zip(voxel, got["face"], got["material"])} == faces
    # the order: the material array's (the tree's key of the voxel), then the face
    key = MR.tree_order_key(np.concatenate([voxel, MR.last_wins(case.xyz, case.ids)[0]]))[:len(voxel)]
    order = list(zip(key.tolist(), got["face"].tolist()))
    assert order == sorted(order) and len(set(order)) == len(order)
    assert got.tobytes() == MR.table_of(case.xyz, case.ids, case.materials).tobytes()


def test_host_build_refuses_what_it_cannot_build():
    m = MC.materials()
    for xyz, ids, mats, status in (([(0, 0, 0)], [2], np.zeros(0, dtype=_ffi.MATERIAL), -1), ([(0, 0, 0), (40000, 0, 0)], [2, 2], m, -5)):
        with pytest.raises(_ffi.BlokError) as e:
            LT.host_model_lights(xyz, ids, mats)
        assert e.value.status == status


@pytest.mark.parametrize("e", [0, 1, 3])
def test_record_map_names_the_faces_of_the_world_voxels_the_instance_oracle_reports(e):
    """For every orientation and face: the cell's fine voxels (a model voxel of exponent e is a cube of 2^e voxels of the lattice the oracle's
    map works in) go through instance_oracle.world_records; the record's rectangle must be the outermost layer of those world voxels in the
    direction of the world face the oracle reports, and carry that face number."""
    s = 1 << e
    cell = np.array([-3, 5, 2])
    fine = np.stack(np.meshgrid(*[np.arange(c * s, (c + 1) * s) for c in cell], indexing="ij"), -1).reshape(-1, 3)
    for axis, flip in IO.SIGNED_PERMUTATIONS:
        inst = IO.instance(4, (100, -200, 3000), axis, flip)
        for face in range(6):
            local = np.zeros(len(fine), dtype=HIT)
            local["hit"], local["face"], local["voxel"] = 1, face, fine
            world = IO.world_records(local, inst)
            wf = int(world["face"][0])
            assert (world["face"] == wf).all()
            vox = world["voxel"].astype(np.int64)
            a = wf >> 1
            edge = vox[:, a].max() if wf % 2 == 0 else vox[:, a].min()
            want = {tuple(v) for v in vox[vox[:, a] == edge].tolist()}
            m = np.zeros(1, dtype=LIGHT)[0]
            m["lo"] = cell + (np.arange(3) == (face >> 1)) * (face % 2 == 0)
            m["du"], m["dv"], m["face"], m["material"], m["cum"] = 1, 1, face, 9, 5
            rec = LT.instance_light_record(inst, e, m)
            got, got_face = MR.rectangle_voxels(rec)
            assert got_face == wf and got == want, (axis, flip, face, e)
            assert (int(rec["du"]), int(rec["dv"]), int(rec["material"]), int(rec["cum"])) == (s, s, 9, 0)


def _lantern_models(e):
    return {0: dict(lo=(0, 0, 0), hi=(3, 3, 3), e=e, live=True, n_faces=54)}


def test_prefix_rule_and_its_overflow_pair():
    """A 3^3 all-glowing cube has 54 faces, 54 * 4^8 = 3 538 944 per instance at e = 8: 1213 instances stay below 2^32, 1214 do not.
    This checks the numpy rule of tests/model_lights_reference.py alone, no product code: it is the reference the device's prefix kernel
    (tests/test_model_lights_gpu.py) and the host shim's prefix (tests/test_model_lights_paths_cpu.py, through its header and icum) are
    held to."""
    per = 54 << 16
    assert per == 3_538_944 and 1213 * per < 2 ** 32 <= 1214 * per
    for n, disabled in ((1213, 0), (1214, 1)):
        inst = np.zeros(n, dtype=INSTANCE)
        inst["axis"] = (0, 1, 2)
        icum, h = MR.prefix(inst, _lantern_models(8))
        assert h["disabled"] == disabled and h["n_lit"] == (0 if disabled else n)
        assert h["a_inst"] == (0 if disabled else n * per) and h["a_total"] == h["a_inst"]
        assert icum.tolist() == ([0] * (n + 1) if disabled else [i * per for i in range(n + 1)])
    # a world table counts towards the limit
    inst = np.zeros(1213, dtype=INSTANCE)
    inst["axis"] = (0, 1, 2)
    room = 2 ** 32 - 1213 * per
    assert MR.prefix(inst, _lantern_models(8), a_world=room - 1)[1]["disabled"] == 0
    icum, h = MR.prefix(inst, _lantern_models(8), a_world=room)
    assert h["disabled"] == 1 and h["a_total"] == room and not icum.any()
    # unusable records count nothing, in place
    inst = np.zeros(5, dtype=INSTANCE)
    inst["axis"] = (0, 1, 2)
    inst["model"][1] = 7                                  # no such model
    inst["flip"][2] = 8
    inst["offset"][3] = (32767, 0, 0)                     # the box leaves the lattice
    icum, h = MR.prefix(inst, _lantern_models(1), a_world=10, vs=0.5)
    assert icum.tolist() == [0, 216, 216, 216, 216, 432] and h["n_lit"] == 2 and h["a_total"] == 442
    assert h["area_world"] == np.float32(442 * 0.25)


def test_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "model_lights_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(SRC / "model_lights_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/model_lights.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
    files = []
    for n, case in enumerate(CASES):
        want = MR.table_of(case.xyz, case.ids, case.materials)
        files.append(tmp_path / f"case_{n}.bin")
        files[-1].write_bytes(struct.pack("<QQQ", len(case.xyz), len(case.materials), len(want)) + case.xyz.tobytes() + case.ids.tobytes() +
                              case.materials.tobytes() + want.tobytes())
    run = subprocess.run([os.fspath(exe), *map(os.fspath, files)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "model_lights_main: ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count(" faces\n") == len(files)
