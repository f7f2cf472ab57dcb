"""CPU: the host build of the pyramid of coarser levels (blok_lod_reduce, blok_amd/lod.py) against the numpy model of the contract
(tests/lod_reference.py), planes and infos byte for byte on every case table of the GPU tests; the properties of the rule asserted from the
model alone; and the long boxes' closed form pinned to the model at LENGTH_PINNED cells."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import lod as HL
from blok_amd._ffi import BlokError
from tests import limit_cases as LC
from tests import lod_reference as R

ROOT = Path(__file__).resolve().parent.parent
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
X = R.VOTE_EXPOSED


def same(got, want, tag=""):
    """(levels, info) pairs equal byte for byte."""
    assert got[1].tobytes() == want[1].tobytes(), f"{tag}: info {got[1]} != {want[1]}"
    assert len(got[0]) == len(want[0])
    for j, (g, w) in enumerate(zip(got[0], want[0]), start=1):
        for plane, (a, b) in enumerate(zip(g, w)):
            assert a.dtype == b.dtype and a.shape == b.shape, f"{tag}: level {j} plane {plane}: {a.dtype} {a.shape} != {b.dtype} {b.shape}"
            assert a.tobytes() == b.tobytes(), f"{tag}: level {j} plane {plane}: {int((a != b).sum())} of {a.size} cells differ"


def host_of(c):
    return HL.reduce_host(c["d"], c["m"], c["origin"], c["lo"], c["hi"], c["levels"], c["flags"])


def test_abi_is_at_least_1_16_and_the_info_has_its_size():
    assert _ffi.hip_lib().blok_hip_abi_version() >= (1 << 16) | 16
    assert _ffi.LOD_INFO.itemsize == 360 and _ffi.LOD_LEVEL.itemsize == 64 and _ffi.LOD_INFO.fields["level"][1] == 40


@pytest.mark.parametrize("table", ["noise", "seams"])
def test_host_build_matches_the_model(table):
    cases = R.noise_cases() if table == "noise" else R.seam_cases()
    assert len(cases) >= 6
    for c in cases:
        same(host_of(c), R.model_of(c), c["name"])


@pytest.mark.parametrize("which", LC.LIMITS)
def test_host_build_matches_the_model_in_the_limit_boxes(which):
    c = R.limit_case(which)
    same(host_of(c), R.model_of(c), c["name"])


@pytest.mark.parametrize("box", LC.LONG_BOXES, ids=LC.LONG_IDS)
def test_long_box_closed_form_is_pinned_to_the_model(box):
    """At LENGTH_PINNED cells the closed form equals the model, and the host build both; the box still crosses waves, and holds filled cells
    of id 0 and of id 0xFFFFFFFF."""
    short = box.shortened()
    d, m = R.long_fill(short)
    want = R.reduce(d, m, short.origin, None, None, R.LONG_LEVELS, 0)
    closed = R.long_expected(short, d, m)
    for j in range(R.LONG_LEVELS):
        for plane in range(3):
            assert closed[j][plane].tobytes() == want[0][j][plane].tobytes(), (j, plane)
    same(HL.reduce_host(d, m, short.origin, None, None, R.LONG_LEVELS, 0), want, box.name)
    ids = m[d > 0]
    assert (ids == 0).any() and (ids == 0xFFFFFFFF).any() and int((d > 0).sum()) > 100


def test_host_build_errors():
    d, m = R.noise(0.5)
    o = R.NOISE_ORIGIN
    for kw, rc in ((dict(levels=0), BLOK_ERR_INVALID_ARG), (dict(levels=6), BLOK_ERR_INVALID_ARG), (dict(flags=2), BLOK_ERR_INVALID_ARG),
                   (dict(lo=(0, 0, 0)), BLOK_ERR_INVALID_ARG), (dict(lo=(1, 0, 0), hi=(0, 1, 1)), BLOK_ERR_INVALID_ARG),
                   (dict(lo=(-6, 0, 0), hi=(0, 1, 1)), BLOK_ERR_UNSUPPORTED), (dict(lo=(0, 0, 0), hi=(9, 1, 1)), BLOK_ERR_UNSUPPORTED)):
        with pytest.raises(BlokError) as e:
            HL.reduce_host(d, m, o, **kw)
        assert e.value.status == rc, kw


def _checksum(raw: bytes) -> int:
    w = np.frombuffer(raw, dtype=np.uint32).astype(np.uint64)
    return int((w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_host_build_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/lod_main.cpp) over case files: every noise and seam case and three refusals, the planes in an
    array of exactly the planned size; nothing loaded into Python is sanitized."""
    exe = tmp_path / "lod_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/lod_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/lod.cpp")], check=True)
    jobs = [(c, 0) for c in R.noise_cases() + R.seam_cases()]
    first = jobs[0][0]
    jobs += [(dict(first, levels=6), BLOK_ERR_INVALID_ARG), (dict(first, flags=4), BLOK_ERR_INVALID_ARG), (dict(first, lo=(-9, 0, 0), hi=(0, 1, 1)), BLOK_ERR_UNSUPPORTED)]
    files, want = [], []
    for i, (c, status) in enumerate(jobs):
        path = tmp_path / f"case{i}.bin"
        region = [1] + list(c["lo"]) + list(c["hi"]) if c["lo"] is not None else [0] * 7
        header = np.array(list(c["shape"]) + list(c["origin"]) + region + [c["levels"], c["flags"]], dtype=np.int32)
        path.write_bytes(header.tobytes() + c["d"].tobytes() + c["m"].tobytes())
        files.append(os.fspath(path))
        if status:
            want.append(f"{status} {status} 0 0 0")
        else:
            levels, info = R.model_of(c)
            raw = b"".join(plane.tobytes() for level in levels for plane in level)
            want.append(f"0 0 {len(raw)} {_checksum(raw)} {_checksum(info.tobytes())}")
    run = subprocess.run([os.fspath(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.splitlines() == want


# ---- the rule, from the model alone ----------------------------------------------------------------------------------------------------------
def box(shape, fill=0.0, ident=0):
    nx, ny, nz = shape
    return np.full((nz, ny, nx), fill, np.float32), np.full((nz, ny, nx), ident, np.uint32)


def test_a_tie_goes_to_the_smallest_id():
    assert R.vote([1, 1], [9, 4]) == 4 and R.vote([2, 1, 1], [7, 3, 3]) == 3 and R.vote([0, 0], [5, 6]) == 0 and R.vote([0, 3], [1, 0xFFFFFFFF]) == 0xFFFFFFFF
    d, m = box((2, 2, 2))
    d[0, 0, 0] = d[1, 1, 1] = 1.0
    m[0, 0, 0], m[1, 1, 1] = 9, 4
    (level,), info = R.reduce(d, m, (0, 0, 0))
    assert level[0].tolist() == [[[2]]] and level[2].tolist() == [[[4]]]
    same(HL.reduce_host(d, m, (0, 0, 0)), ((level,), info))


def test_the_weighted_vote_beats_the_unweighted_one():
    """At level 2: one child with n = 8 of id 5 against three children with n = 1 of id 2 gives 5."""
    d, m = box((4, 4, 4))
    d[0:2, 0:2, 0:2], m[0:2, 0:2, 0:2] = 1.0, 5
    for z, y, x in ((0, 0, 2), (0, 2, 0), (2, 0, 0)):
        d[z, y, x], m[z, y, x] = 1.0, 2
    levels, _ = R.reduce(d, m, (0, 0, 0), levels=2)
    assert sorted(levels[0][0].reshape(-1).tolist()) == [0, 0, 0, 0, 1, 1, 1, 8]
    assert levels[1][0].tolist() == [[[11]]] and levels[1][2].tolist() == [[[5]]]
    same(HL.reduce_host(d, m, (0, 0, 0), levels=2), R.reduce(d, m, (0, 0, 0), levels=2))


def test_vote_exposed_keeps_the_skin_and_falls_back_without_one():
    """A slab of id 2 under a one-cell layer of id 1 gives 2 without VOTE_EXPOSED and 1 with it; a cell with e = 0 falls back to the n-vote."""
    d, m = box((8, 8, 8))
    d[:, 0:7, :], m[:, 0:6, :], m[:, 6, :] = 1.0, 2, 1          # y 0..5 id 2, y 6 id 1, y 7 empty
    plain, _ = R.reduce(d, m, (0, 0, 0), levels=3)
    skin, info = R.reduce(d, m, (0, 0, 0), levels=3, flags=X)
    assert plain[2][2].tolist() == [[[2]]] and skin[2][2].tolist() == [[[1]]]
    assert int(skin[2][0][0, 0, 0]) == 7 * 64 and int(skin[2][1][0, 0, 0]) == 64
    # level 1: the cells of y 0..5 are buried (the box's faces expose nothing): e = 0, and their id is the n-vote's
    assert (skin[0][1][:, 0:3, :] == 0).all() and (skin[0][2][:, 0:3, :] == 2).all() and (skin[0][1][:, 3, :] == 4).all() and (skin[0][2][:, 3, :] == 1).all()
    assert (plain[0][2][:, 3, :] == 1).all()                    # (a tie of 4 and 4: the smallest id)
    same(HL.reduce_host(d, m, (0, 0, 0), levels=3, flags=X), (skin, info))


def test_the_faces_of_the_box_expose_nothing_and_a_regions_own_faces_see_the_real_neighbours():
    d, m = box((6, 6, 6), 1.0, 3)
    (level,), info = R.reduce(d, m, (-3, 5, 1))
    assert int(info["level"][0][0]["sum_n"]) == 216 and int(info["level"][0][0]["sum_e"]) == 0
    # a region inside the full box: its faces cut filled cells whose neighbours are filled -> still nothing exposed
    (inner,), inner_info = R.reduce(d, m, (-3, 5, 1), (-2, 6, 2), (2, 10, 6))
    assert int(inner_info["level"][0][0]["sum_n"]) == 64 and int(inner_info["level"][0][0]["sum_e"]) == 0
    # ... and with an empty cell just outside the region, the cell inside that touches it is exposed
    d[2, 2, 0] = 0.0                                              # box-local (0, 2, 2): world (-3, 7, 3), outside the region, next to (-2, 7, 3)
    (inner,), inner_info = R.reduce(d, m, (-3, 5, 1), (-2, 6, 2), (2, 10, 6))
    assert int(inner_info["level"][0][0]["sum_n"]) == 64 and int(inner_info["level"][0][0]["sum_e"]) == 1
    same(HL.reduce_host(d, m, (-3, 5, 1), (-2, 6, 2), (2, 10, 6)), ((inner,), inner_info))


def test_a_full_aligned_box_has_a_level_5_cell_of_32768():
    d, m = box((64, 32, 32), 1.0, 6)
    got = R.reduce(d, m, (-64, 32, 0), levels=5)
    same(HL.reduce_host(d, m, (-64, 32, 0), levels=5), got)
    assert got[0][4][0].dtype == np.uint16 and got[0][4][0].tolist() == [[[32768, 32768]]] and got[0][4][2].tolist() == [[[6, 6]]]
    assert [int(c) for c in got[1]["level"][0][4]["clo"]] == [-2, 1, 0] and int(got[1]["level"][0][4]["sum_e"]) == 0


def test_levels_nest_and_regions_restrict_and_boxes_translate():
    d, m = R.noise(0.5)
    o = R.NOISE_ORIGIN
    full, _ = R.reduce(d, m, o, levels=3, flags=X)
    # level j of a K-level call equals level j of a j-level call
    for j in (1, 2):
        part, _ = R.reduce(d, m, o, levels=j, flags=X)
        for plane in range(3):
            assert part[j - 1][plane].tobytes() == full[j - 1][plane].tobytes()
    # the whole-box result restricted to a 2^K-aligned sub-region equals that sub-region's own result (K = 2: world [-4, 4) x [0, 4) x [0, 4))
    K = 2
    whole, winfo = R.reduce(d, m, o, levels=K, flags=X)
    sub, sinfo = R.reduce(d, m, o, (-4, 0, 0), (4, 4, 4), levels=K, flags=X)
    for j in range(1, K + 1):
        wl, sl = winfo["level"][0][j - 1], sinfo["level"][0][j - 1]
        off = [int(sl["clo"][a]) - int(wl["clo"][a]) for a in range(3)]
        ext = [int(c) for c in sl["cext"]]
        for plane in range(3):
            cut = whole[j - 1][plane][off[2]:off[2] + ext[2], off[1]:off[1] + ext[1], off[0]:off[0] + ext[0]]
            assert cut.tobytes() == sub[j - 1][plane].tobytes(), (j, plane)
    # translating the box and the region by multiples of 2^K translates the planes
    shift = (8, -16, 24)
    moved, minfo = R.reduce(d, m, tuple(a + s for a, s in zip(o, shift)), levels=3, flags=X)
    finfo = R.reduce(d, m, o, levels=3, flags=X)[1]
    for j in range(3):
        for plane in range(3):
            assert moved[j][plane].tobytes() == full[j][plane].tobytes()
        assert [int(c) for c in minfo["level"][0][j]["clo"]] == [int(c) + (s >> (j + 1)) for c, s in zip(finfo["level"][0][j]["clo"], shift)]
    same(HL.reduce_host(d, m, tuple(a + s for a, s in zip(o, shift)), levels=3, flags=X), (moved, minfo))
