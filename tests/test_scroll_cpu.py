"""CPU: the scroll of the resident volume on the host (blok_scroll_plan, blok_scroll_voxels) against the numpy model
(tests/scroll_reference.py) on every case the GPU tests run, and — from the model alone — what makes those cases hard.  Every comparison
is exact."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import scroll as S
from blok_amd._ffi import BlokError
from tests import scroll_reference as R

ROOT = Path(__file__).resolve().parent.parent
BOXES = (R.SMALL, R.MID)
CASES = [(box, delta) for box in BOXES for delta in R.deltas(box)]
CASE_IDS = [f"{'x'.join(map(str, box[0]))}-by-{'_'.join(map(str, delta))}" for box, delta in CASES]


def is_main(box, delta):
    """A case that keeps something and moves."""
    return any(delta) and R.plan(box[1], box[0], delta)["n_cells_kept"] > 0


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
def test_record_sizes():
    assert _ffi.SCROLL_BOX.itemsize == 24 and _ffi.SCROLL_INFO.itemsize == 200
    text = (ROOT / "include" / "blok_hip.h").read_text()
    for record, size in (("blok_scroll_box", 24), ("blok_scroll_info", 200)):
        assert f"}} {record};" in text and f"{size} bytes */" in text.split(f"}} {record};")[1].splitlines()[0]
    src = "#include \"blok_hip.h\"\n_Static_assert(sizeof(blok_scroll_box) == 24 && sizeof(blok_scroll_info) == 200, \"sizes\");\nint main(void) { return 0; }\n"
    r = subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", "-fsyntax-only", "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def test_model_plan_by_hand():
    """The box [-5, 8) x [-3, 7) x [-2, 5) moved by (-8, 0, 4): C = [-5, 0) x [-3, 7) x [2, 5)."""
    p = R.plan((-5, -3, -2), (13, 10, 7), (-8, 0, 4))
    assert p["origin"] == (-13, -3, 2) and p["n_cells_kept"] == 5 * 10 * 3
    assert p["exposed"] == [((-13, -3, 5), (0, 7, 9)), ((-13, -3, 2), (-5, 7, 5))]      # the z slab over new x and y, then the x slab cut to C's z
    assert p["leaving"] == [((-5, -3, -2), (8, 7, 2)), ((0, -3, 2), (8, 7, 5))]
    gone = R.plan((-5, -3, -2), (13, 10, 7), (0, 12, 0))
    assert gone["n_cells_kept"] == 0 and gone["exposed"] == [((-5, 9, -2), (8, 19, 5))] and gone["leaving"] == [((-5, -3, -2), (8, 7, 5))]
    still = R.plan((-5, -3, -2), (13, 10, 7), (0, 0, 0))
    assert still["exposed"] == [] and still["leaving"] == [] and still["n_cells_kept"] == 13 * 10 * 7 and still["origin"] == (-5, -3, -2)


@pytest.mark.parametrize("box,delta", CASES, ids=CASE_IDS)
def test_host_plan_equals_the_model_and_the_boxes_tile(box, delta):
    dims, origin = box
    got = S.scroll_plan_host(origin, dims, delta)
    zeros = np.zeros(dims[::-1], np.float32)
    assert got.tobytes() == R.info(zeros, zeros.view(np.uint32), origin, delta).tobytes()
    new_origin = tuple(int(c) for c in got["origin"][0])
    assert new_origin == tuple(o + d for o, d in zip(origin, delta))
    # painted: every cell of new \ old, and of old \ new, is covered once, every other cell never
    assert np.array_equal(R.paint(S.boxes(got, "exposed"), new_origin, dims), (~R.inside(new_origin, dims, origin)).astype(np.int32))
    assert np.array_equal(R.paint(S.boxes(got, "leaving"), origin, dims), (~R.inside(origin, dims, new_origin)).astype(np.int32))
    assert int(got["n_cells_kept"][0]) == int(R.inside(origin, dims, new_origin).sum())


# ---- the move -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box,delta", CASES, ids=CASE_IDS)
def test_host_move_equals_the_model(box, delta):
    dims, origin = box
    d, m = R.noise(dims)
    keep_d, keep_m = d.copy(), m.copy()
    got_d, got_m, info = S.scroll_voxels_host(d, m, origin, delta)
    want_d, want_m = R.scroll(d, m, delta)
    assert got_d.tobytes() == want_d.tobytes() and got_m.tobytes() == want_m.tobytes()
    assert info.tobytes() == R.info(d, m, origin, delta).tobytes()
    assert d.tobytes() == keep_d.tobytes() and m.tobytes() == keep_m.tobytes()


def test_model_moves_world_cells():
    """The model itself, cell by cell on the small box: a world voxel in both boxes keeps its words, every other cell is (+0.0f, 0)."""
    dims, origin = R.SMALL
    d, m = R.noise(dims)
    for delta in R.deltas(R.SMALL):
        out_d, out_m = R.scroll(d, m, delta)
        for z in range(dims[2]):
            for y in range(dims[1]):
                for x in range(dims[0]):
                    sx, sy, sz = x + delta[0], y + delta[1], z + delta[2]
                    if 0 <= sx < dims[0] and 0 <= sy < dims[1] and 0 <= sz < dims[2]:
                        assert out_d.view(np.uint32)[z, y, x] == d.view(np.uint32)[sz, sy, sx] and out_m[z, y, x] == m[sz, sy, sx]
                    else:
                        assert out_d.view(np.uint32)[z, y, x] == 0 and out_m[z, y, x] == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _ffi.host_lib()
    for dims, origin in BOXES + (((96, 80, 64), (R.LATTICE_LO,) * 3), ((96, 80, 64), tuple(R.LATTICE_HI - n for n in (96, 80, 64)))):
        d, m = R.noise(dims)
        for delta, flags, status in R.refusals(origin, dims):
            if flags:
                continue                                           # (the host builds take no flags)
            with pytest.raises(BlokError) as e:
                S.scroll_plan_host(origin, dims, delta)
            assert e.value.status == status, (origin, delta)
            out_d, out_m = np.full_like(d, 7.0), np.full_like(m, 7)
            info = np.full(1, 0, dtype=_ffi.SCROLL_INFO)
            rc = lib.blok_scroll_voxels(_ffi.ptr(d), _ffi.ptr(m), S._vec(origin), *dims, S._vec(delta), _ffi.ptr(out_d), _ffi.ptr(out_m), _ffi.ptr(info))
            assert rc == status and (out_d == 7.0).all() and (out_m == 7).all() and not info.tobytes().strip(b"\0")      # nothing written
    info = np.zeros(1, dtype=_ffi.SCROLL_INFO)
    delta = S._vec((4, 0, 0))
    assert lib.blok_scroll_plan(None, 0, 4, 4, delta, _ffi.ptr(info)) == R.INVALID_ARG
    assert lib.blok_scroll_plan(None, 4, 4, 4, delta, None) == R.INVALID_ARG
    assert lib.blok_scroll_plan(None, 4, 4, 4, delta, _ffi.ptr(info)) == 0 and tuple(info["origin"][0]) == (4, 0, 0)      # a null origin is (0, 0, 0)
    d = np.zeros((4, 4, 4), np.float32)
    assert lib.blok_scroll_voxels(None, _ffi.ptr(d), None, 4, 4, 4, delta, _ffi.ptr(d), _ffi.ptr(d), None) == R.INVALID_ARG
    # ending exactly on the lattice's end is fine, on either side
    assert S.scroll_plan_host((R.LATTICE_HI - 16, 0, 0), (8, 8, 8), (8, 0, 0))["origin"][0, 0] == R.LATTICE_HI - 8
    assert S.scroll_plan_host((R.LATTICE_LO + 8, 0, 0), (8, 8, 8), (-8, 0, 0))["origin"][0, 0] == R.LATTICE_LO


# ---- the host builds under the sanitizers ---------------------------------------------------------------------------------------------------
def _checksum(a) -> int:
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_host_builds_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/scroll_main.cpp) over case files: every case of the table and every refusal; nothing loaded
    into Python is sanitized."""
    exe = tmp_path / "scroll_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/scroll_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/scroll.cpp")], check=True)
    jobs = [(box, delta, 0) for box, delta in CASES]
    jobs += [(R.SMALL, delta, status) for delta, flags, status in R.refusals(R.SMALL[1], R.SMALL[0]) if not flags]
    files, want = [], []
    for i, ((dims, origin), delta, status) in enumerate(jobs):
        d, m = R.noise(dims, seed=i)
        path = tmp_path / f"case{i}.bin"
        header = np.array(list(dims) + list(origin) + list(delta or (0, 0, 0)) + [delta is not None], dtype=np.int32)
        path.write_bytes(header.tobytes() + d.tobytes() + m.tobytes())
        files.append(os.fspath(path))
        if status:
            want.append(f"{status} {status} 0 0 0 0")
        else:
            out_d, out_m = R.scroll(d, m, delta)
            zeros = np.zeros_like(d)
            want.append(f"0 0 {_checksum(out_d)} {_checksum(out_m)} {_checksum(R.info(zeros, zeros, origin, delta))} {_checksum(R.info(d, m, origin, delta))}")
    run = subprocess.run([os.fspath(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.splitlines() == want


# ---- what makes the cases hard, from the model alone ----------------------------------------------------------------------------------------
def test_the_cases_are_hard():
    counts = set()
    for box, delta in CASES:
        dims, origin = box
        d, m = R.noise(dims)
        rec = R.info(d, m, origin, delta)[0]
        counts.add(int(rec["n_exposed"]))
        assert int(rec["n_exposed"]) == int(rec["n_leaving"])
        if not is_main(box, delta):
            continue
        assert int(rec["n_filled_before"]) > int(rec["n_filled_kept"]) > 0, (box, delta)      # filled voxels are lost, and some stay
        dst, src = R.kept_slices(dims, delta)
        kept_d, kept_m = d[src], m[src]
        words = kept_d.view(np.uint32)
        assert (words == 0x80000000).any(), "-0.0f among the kept cells"
        assert np.isnan(kept_d).any() and (kept_d < 0).any()
        assert ((kept_m != 0) & ~R.filled(kept_d)).any(), "an id under density 0"
    assert counts == {0, 1, 2, 3}
    assert any(R.plan(box[1], box[0], delta)["n_cells_kept"] == 0 for box, delta in CASES), "some case keeps nothing"
    assert sum(is_main(box, delta) for box, delta in CASES) >= 14
    # a ragged case in which a brick that is full in the old box lands on the new box's ragged last brick: the moved mask must be cut
    dims, origin = R.SMALL
    d, m = R.noise(dims)
    bx, by, bz = R.FULL_BRICK
    assert R.brick_mask(d, bx, by, bz) == (1 << 64) - 1
    delta = (-4, 0, 0)
    assert delta in R.deltas(R.SMALL) and bx + 1 == (dims[0] + 3) // 4 - 1 and dims[0] % 4 != 0
    after = R.brick_mask(R.scroll(d, m, delta)[0], bx + 1, by, bz)
    assert after != 0 and after != (1 << 64) - 1 and bin(after).count("1") == 16 * (dims[0] % 4)
