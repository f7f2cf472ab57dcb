"""The fill units of a packed frame's one launch (blok_amd/csrc/hip/fill_units.h; trace_kernels.hip: packed_frame_kernel,
packed_frame_own_kernel), on the host through a shim: the grid follows its formula, every pixel of the rectangle is owned by exactly one
(workgroup, unit, lane), no workgroup meets a unit that is not below U or carries more than k.  No GPU."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "fill_units_shim.cpp"
HDR = ROOT / "blok_amd" / "csrc" / "hip" / "fill_units.h"
LIB = ROOT / "tests" / "host_harness" / "libfill_units_shim.so"

WIDTHS = (1, 7, 8, 63, 64, 65, 77, 200, 3840)
HEIGHTS = (1, 8, 61, 136)
GROUPS = (0, 1, 37, 5000)
CAPS = (1, 4, 1000)


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-Wall", "-Wextra", "-Werror", f"-I{HDR.parent}", "-shared", "-o", os.fspath(LIB), os.fspath(SRC)], check=True)
    L = C.CDLL(os.fspath(LIB))
    L.fill_units_walk.restype = C.c_uint32
    L.fill_units_walk.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)] * 4 + [C.c_void_p, C.POINTER(C.c_uint64)]
    return L


def walk(L, w, h, n_groups, k):
    owners = np.zeros((h, w), dtype=np.uint32)
    units, units_x, most, beyond, outside = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    grid = L.fill_units_walk(w, h, n_groups, k, C.byref(units), C.byref(units_x), C.byref(most), C.byref(beyond), C.c_void_p(owners.ctypes.data), C.byref(outside))
    return int(grid), int(units.value), int(units_x.value), int(most.value), int(beyond.value), owners, int(outside.value)


@pytest.mark.parametrize("w", WIDTHS)
def test_every_pixel_has_one_owner_and_the_grid_follows_its_formula(lib, w):
    for h in HEIGHTS:
        for n_groups in GROUPS:
            for k in CAPS:
                grid, units, units_x, most, beyond, owners, outside = walk(lib, w, h, n_groups, k)
                where = f"{w} x {h}, {n_groups} groups, k = {k}"
                assert units_x == -(-w // 64) and units == h * units_x, where
                assert grid == max(n_groups, -(-units // k)), where
                assert beyond == 0, f"{where}: {beyond} units that are not below U"
                assert most <= k, f"{where}: a workgroup with {most} units"
                assert (owners == 1).all(), f"{where}: {int((owners != 1).sum())} pixels without exactly one owner"
                assert outside == units * 64 - w * h, where


def test_the_headline_frame(lib):
    """3840 x 2160 with pose A's 38 000 groups: 129 600 units; k = 4 leaves the grid at the walk's, k = 2 adds a tail, k = 1 more of it."""
    for k, want in ((1, 129600), (2, 64800), (4, 38000), (8, 38000)):
        grid, units, _, most, _, owners, _ = walk(lib, 3840, 2160, 38000, k)
        assert (units, grid) == (129600, want) and most <= k and (owners == 1).all()


def test_the_walk_runs_clean_under_the_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main), built with the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "fill_units_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFILL_UNITS_SHIM_MAIN",
                    f"-I{HDR.parent}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    r = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
