"""CPU: the light table (include/blok_hip.h, "emissive voxels as lights"; include/blok_world.h: blok_lights_from_quads, blok_lights_check).
The host build against the numpy model of tests/lights_reference.py, bit for bit, over tests/lights_cases.py; every rule of the table
check; the pick, exhaustively; and the stand-alone program of tests/host_harness/lights_main.cpp under ASan + UBSan."""
from __future__ import annotations

import ctypes as C
import os
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import lights as LT
from blok_amd._ffi import LIGHT, LIGHTS_INFO, BlokError
from tests import lights_cases as LC
from tests import lights_reference as LR

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
CASES = LC.table()


def test_abi_symbols_sizes_and_version():
    header = (ROOT / "include" / "blok_hip.h").read_text()
    for name in ("blok_hip_lights_from_quads", "blok_hip_set_lights", "blok_hip_lights_info", "blok_hip_lights_download"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _ffi.HIP_SYMBOLS
        assert hasattr(_ffi.hip_lib(), name)
    for name in ("blok_lights_from_quads", "blok_lights_check"):
        assert name in _ffi.HOST_SYMBOLS and hasattr(_ffi.host_lib(), name)
    assert LIGHT.itemsize == 32 and LIGHTS_INFO.itemsize == 32 and LIGHT.itemsize == _ffi.QUAD.itemsize
    assert [LIGHT.fields[k][1] for k in ("lo", "du", "dv", "material", "face", "cum")] == [_ffi.QUAD.fields[k][1] for k in ("lo", "du", "dv", "material", "face", "reserved")]
    version = _ffi.hip_lib().blok_hip_abi_version()
    assert version >> 16 == 1 and version & 0xFFFF >= 26
    mirror = (ROOT / "include" / "blok" / "hip_tracer.hpp").read_text()
    assert "blok_hip_lights_from_quads" in mirror and "blok_hip_set_lights" in mirror


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_build_equals_the_numpy_model(case):
    quads = LC.quads_of(case)
    want, faces, owned = LR.from_quads(quads, case.materials)
    for vs in (1.0, 0.5):
        got, info = LT.host_from_quads(quads, case.materials, vs)
        print(f"{case.name}: {len(quads)} quads -> {len(got)} lights, {faces} faces, owned {owned.tolist()}")
        assert got.tobytes() == want.tobytes()
        assert (int(info["n"][0]), int(info["n_faces"][0]), int(info["n_owned"][0]), int(info["bytes"][0])) == (len(want), faces, len(owned), 32 * len(want))
        assert info["area_world"][0] == np.float32(faces) * np.float32(vs) * np.float32(vs)
    if case.n_lights is not None:
        assert (len(want), faces) == (case.n_lights, case.n_faces)
    else:
        assert len(want) > 4096
    if len(want):
        assert int(LT.check(want)["n_faces"][0]) == faces
        dropped = len(quads) - len(want)
        assert case.name.startswith(("one glowing", "glowing voxels on")) or dropped > 0


def _good(n=3):
    t = np.zeros(n, dtype=LIGHT)
    t["du"], t["dv"] = 2, 3
    t["face"] = np.arange(n) % 6
    t["lo"] = [(i, 2 * i, -i) for i in range(n)]
    t["cum"] = 6 * np.arange(n)
    return t


def test_each_rule_of_the_table_check():
    assert int(LT.check(_good())["n"][0]) == 3
    assert int(LT.check(np.zeros(0, dtype=LIGHT))["n"][0]) == 0
    for field, at, value, status, text in (("face", 1, 6, BLOK_ERR_INVALID_ARG, "light 1: face"), ("du", 2, 0, BLOK_ERR_INVALID_ARG, "light 2: du or dv"),
                                           ("dv", 0, 0, BLOK_ERR_INVALID_ARG, "light 0: du or dv"), ("cum", 1, 5, BLOK_ERR_INVALID_ARG, "light 1: cum"),
                                           ("cum", 0, 1, BLOK_ERR_INVALID_ARG, "light 0: cum")):
        t = _good()
        t[field][at] = value
        with pytest.raises(BlokError) as e:
            LT.check(t)
        assert e.value.status == status and text in str(e.value), str(e.value)
    for lo in ((-32769, 0, 0), (0, 32769, 0), (0, 0, 32767)):       # the last: lo + dv passes 32768 along v of face 0
        t = _good(1)
        t["lo"][0] = lo
        with pytest.raises(BlokError) as e:
            LT.check(t)
        assert e.value.status == BLOK_ERR_INVALID_ARG and "corner" in str(e.value)
    t = _good(1)
    t["lo"][0] = (32768, 32766, 32765)                               # the far corner of the lattice itself is inside
    assert int(LT.check(t)["n_faces"][0]) == 6
    forged = np.zeros(1, dtype=LIGHT)
    forged["lo"], forged["du"], forged["dv"], forged["face"] = (-32768, -32768, -32768), 65536, 65536, 4
    with pytest.raises(BlokError) as e:
        LT.check(forged)
    assert e.value.status == BLOK_ERR_UNSUPPORTED
    # A = 2^32 - 1 passes, one more face does not
    t = np.zeros(3, dtype=LIGHT)
    t["lo"] = (-32768, -32768, 0)
    t["du"], t["dv"], t["face"] = (65535, 65535, 1), (65536, 1, 1), 4
    t["cum"] = (0, 65535 * 65536, 65535 * 65536 + 65535)
    assert t["cum"][2] == 2 ** 32 - 1
    assert int(LT.check(t[:2])["n_faces"][0]) == 2 ** 32 - 1
    with pytest.raises(BlokError) as e:
        LT.check(t)
    assert e.value.status == BLOK_ERR_UNSUPPORTED


def _mixed_table(n, rng):
    t = np.zeros(n, dtype=LIGHT)
    t["du"] = rng.integers(1, 9, n)
    t["dv"] = rng.integers(1, 9, n)
    t["face"] = rng.integers(0, 6, n)
    t["lo"] = rng.integers(-50, 50, (n, 3))
    area = t["du"].astype(np.int64) * t["dv"]
    t["cum"] = np.concatenate([[0], np.cumsum(area)[:-1]])
    return t, int(area.sum())


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_every_pick_lands_in_its_light_and_cell(n, tmp_path):
    """Through the library's own search (find_light, compiled into a small shared object here) and the numpy model."""
    so = tmp_path / "liblights_pick.so"
    src = tmp_path / "pick.cpp"
    src.write_text('#include "lights_core.h"\nextern "C" uint32_t lp_find(const blok_light* t, uint32_t n, uint32_t pick) { return blok::lights::find_light(t, n, pick); }\n'
                   'extern "C" uint32_t lp_pick(uint32_t r, uint32_t a) { return blok::lights::pick_of(r, a); }\n'
                   'extern "C" void lp_point(const blok_light* l, uint32_t off, float u1, float u2, float vs, float* q, float* nl) { blok::lights::sample_point(*l, off, u1, u2, vs, q, nl); }\n')
    subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-ffp-contract=off", "-shared", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/common'}", "-o", os.fspath(so),
                    os.fspath(src)], check=True)
    lib = C.CDLL(os.fspath(so))
    lib.lp_find.restype = C.c_uint32
    lib.lp_find.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.lp_pick.restype = C.c_uint32
    lib.lp_pick.argtypes = [C.c_uint32, C.c_uint32]
    lib.lp_point.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    t, faces = _mixed_table(n, np.random.default_rng(n))
    assert faces <= 4096
    owner = np.repeat(np.arange(n), t["du"].astype(np.int64) * t["dv"])
    q, nl = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    for pick in range(faces):
        i = lib.lp_find(_ffi.ptr(t), n, pick)
        assert i == owner[pick] == LR.find_light(t, pick)
        off = pick - int(t["cum"][i])
        assert 0 <= off < int(t["du"][i]) * int(t["dv"][i])
        if pick % 7 == 0:
            u1, u2 = np.float32(0.25 + 0.5 * (pick % 2)), np.float32(0.8125)
            lib.lp_point(_ffi.ptr(t[i:i + 1]), off, u1, u2, 0.5, _ffi.ptr(q), _ffi.ptr(nl))
            wq, wnl = LR.sample_point(t[i], off, u1, u2, 0.5)
            assert q.tobytes() == wq.tobytes() and nl.tobytes() == wnl.tobytes()
            a = int(t["face"][i]) >> 1
            u_ax, v_ax = (1 if a == 0 else 0), (1 if a == 2 else 2)
            cell = (q / np.float32(0.5))
            assert int(t["lo"][i][u_ax]) + off % int(t["du"][i]) <= cell[u_ax] < int(t["lo"][i][u_ax]) + off % int(t["du"][i]) + 1
            assert int(t["lo"][i][v_ax]) + off // int(t["du"][i]) <= cell[v_ax] < int(t["lo"][i][v_ax]) + off // int(t["du"][i]) + 1
    for r in (0, 1, 2 ** 31, 2 ** 32 - 1):
        for a in (1, 2, 6, faces, 4096, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1):
            p = lib.lp_pick(r, a)
            assert p == LR.pick_of(r, a) and p < a
    # every face is picked by some r, in order: the map r -> pick is onto [0, A) and monotone
    rs = np.linspace(0, 2 ** 32 - 1, 4 * faces + 1).astype(np.uint64)
    picks = [lib.lp_pick(int(r), faces) for r in rs]
    assert picks == sorted(picks) and set(picks) == set(range(faces))


def test_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "lights_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(SRC / "lights_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/lights.cpp")], check=True)
    files = []
    for n, case in enumerate(CASES):
        quads = LC.quads_of(case)
        want, _, _ = LR.from_quads(quads, case.materials)
        vs = 0.5 if n % 2 else 1.0
        files.append(tmp_path / f"case_{n}.bin")
        files[-1].write_bytes(struct.pack("<QQQfI", len(quads), len(case.materials), len(want), vs, 0) + quads.tobytes() + case.materials.tobytes() + want.tobytes())
    run = subprocess.run([os.fspath(exe), *map(os.fspath, files)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "lights_main: ok" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count(" faces\n") == len(files)
