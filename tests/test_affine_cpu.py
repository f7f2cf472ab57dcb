"""CPU: the host build of the affine stamp (blok_affine_stamp_voxels) and its helpers (blok_affine_from_instance, blok_affine_from_matrix)
against the numpy model of the contract (tests/affine_reference.py) and against the stamp's own model (tests/stamp_reference.py); the core
header at its limits against unbounded Python integers, and under ASan + UBSan in a program of its own (tests/host_harness/affine_main.cpp)."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import affine as AF
from blok_amd import stamp as ST
from blok_amd._ffi import BlokError
from tests import affine_reference as R
from tests import stamp_reference as SR
from tests.terrain_cases import prior

ROOT = Path(__file__).resolve().parent.parent
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
MODES = (R.SET, R.KEEP, R.ERASE)


def prior_with_empties(shape_xyz):
    """terrain_cases.prior plus negative and NaN densities (test_stamp_gpu.py's recipe)."""
    d0, m0 = prior(tuple(shape_xyz)[::-1])
    d0[::3, ::2, ::5] = -0.5
    d0[1::7, ::3, ::2] = np.nan
    return np.ascontiguousarray(d0), np.ascontiguousarray(m0)


def to_affine(spec, model=0):
    """A CASES entry's ("matrix", F) or ("record", r) as one AFFINE record."""
    kind, what = spec
    if kind == "matrix":
        return AF.from_matrix(what, model)
    rec = np.zeros(1, dtype=_ffi.AFFINE)
    rec["model"], rec["anchor"], rec["m"], rec["t"] = model, what["anchor"], what["m"], what["t"]
    return rec


def clip_region(region, origin, shape):
    if region is None:
        return None, None
    lo = tuple(max(a, o) for a, o in zip(region[0], origin))
    hi = tuple(min(b, o + s) for b, o, s in zip(region[1], origin, shape))
    return lo, hi


def both(d, m, origin, model, rec, lo, hi, mode, value, tag):
    """The host build and the numpy model on copies of (d, m): equal arrays and counts; returns them."""
    gd, gm, wd, wm = d.copy(), m.copy(), d.copy(), m.copy()
    got = AF.stamp_affine_host(gd, gm, origin, *model, rec, lo, hi, mode, value)
    want = R.stamp(wd, wm, origin, *model, rec, lo, hi, mode, value)
    assert got == want, (tag, got, want)
    assert gd.tobytes() == wd.tobytes(), (tag, "density")
    assert gm.tobytes() == wm.tobytes(), (tag, "ids")
    return wd, wm, want


def test_every_orientation_equals_the_stamp_at_exponent_zero():
    d0, m0 = prior_with_empties(R.SHAPE)
    rng = np.random.default_rng(5)
    for name, model in (("small", R.MODELS["small"]), ("large", R.MODELS["large"])):
        for axis, flip in SR.ORIENTATIONS:
            offset = tuple(int(v) for v in rng.integers((-34, -38, -18), (50, 30, 34)))
            mode = MODES[(flip + axis[0]) % 3]
            rec = AF.from_instance(ST.placement(offset, axis, flip, 7))
            assert int(rec["model"][0]) == 7
            gd, gm, wd, wm = d0.copy(), m0.copy(), d0.copy(), m0.copy()
            got = AF.stamp_affine_host(gd, gm, R.ORIGIN, *model, rec, mode=mode, value=1.25)
            want = SR.stamp(wd, wm, R.ORIGIN, *model, (offset, axis, flip), mode, 1.25)
            assert got == want and (want > 0 or mode == R.KEEP), (name, axis, flip, got, want)
            assert gd.tobytes() == wd.tobytes() and gm.tobytes() == wm.tobytes(), (name, axis, flip)


@pytest.mark.parametrize("origin,shape", [(R.ORIGIN, R.SHAPE), (R.ODD_ORIGIN, R.ODD_SHAPE)], ids=["box", "odd box"])
def test_the_matrix_table_equals_the_numpy_model(origin, shape):
    d0, m0 = prior_with_empties(shape)
    written = {mode: 0 for mode in MODES}
    for k, (name, (model, spec, region)) in enumerate(R.CASES.items()):
        rec = to_affine(spec)
        lo, hi = clip_region(region, origin, shape)
        for mode in MODES:
            _, _, n = both(d0, m0, origin, R.MODELS[model], rec, lo, hi, mode, 0.5 + k, (name, mode))
            written[mode] += n
            if mode == R.SET:
                assert (n == 0) == (name == "rank 0, on a hole"), (name, n)
        if name == "rank 0, on a voxel":                       # the whole region gets voxel (1, 0, 0)'s material
            wd, wm, n = both(d0, m0, origin, R.MODELS[model], rec, lo, hi, R.SET, 2.0, name)
            assert n == int(np.prod(np.asarray(hi) - np.asarray(lo)))
            mat = int(R.MODELS["small"][1][[tuple(v) for v in R.MODELS["small"][0]].index((1, 0, 0))])
            assert int((wm == mat).sum()) >= n
    assert all(n > 10000 for n in written.values()), written


def test_regions_that_end_off_the_tile_grid():
    d0, m0 = prior_with_empties(R.SHAPE)
    rec = to_affine(R.CASES["compound rotation, scale 1.5"][1])
    model = R.MODELS["large"]
    for lo, hi in (((-40, -44, -24), (-39, -43, -23)), ((-37, -41, -21), (26, 21, 17)), ((-40, -44, -24), (24, 20, 40)), ((-39, -43, -23), (26, -38, -18)),
                   ((1, 2, 3), (1, 30, 30)), ((-40, -44, -24), (56, 36, 40))):
        for mode in MODES:
            both(d0, m0, R.ORIGIN, model, rec, lo, hi, mode, 1.5, (lo, hi, mode))


# ---- the limits ---------------------------------------------------------------------------------------------------------------------

LIMIT_BOXES = [((-32768, -32768, -32768), (12, 7, 5)), ((32768 - 12, 32768 - 7, 32768 - 5), (12, 7, 5))]      # either end of the int16 lattice


def limit_records(origin, shape):
    """Records at |m| = 2^22, |t| = 2^40 and an anchor 2^20 - 1 from the box's far cell, with both signs."""
    far = [o + s - 1 for o, s in zip(origin, shape)]
    reach = (1 << 20) - 1
    out = []
    for sign in (1, -1):
        anchor_lo = [f - reach for f in far]                   # the far cell lies 2^20 - 1 above the anchor
        anchor_hi = [o + reach for o in origin]                # the first cell 2^20 - 1 below it
        for anchor in (anchor_lo, anchor_hi):
            m = [[sign * (1 << 22), -(1 << 22), (1 << 22)], [(1 << 22), sign * (1 << 22), -(1 << 22)], [-(1 << 22), (1 << 22), sign * (1 << 22)]]
            out.append(R.record(anchor, m, [sign * (1 << 40), -sign * (1 << 40), (1 << 40)]))
            out.append(R.record(anchor, [[sign * (1 << 22)] * 3] * 3, [sign * (1 << 40)] * 3))      # every term of one sign: the largest |P|
    return out


@pytest.mark.parametrize("origin,shape", LIMIT_BOXES, ids=["low end", "high end"])
def test_at_the_limits_the_host_build_samples_what_python_integers_give(origin, shape):
    """The model is one voxel placed where a chosen cell samples; the host build must write exactly the cells whose exact v is that voxel."""
    corners = [tuple(o + c * (s - 1) for o, c, s in zip(origin, bits, shape)) for bits in itertools.product((0, 1), repeat=3)]
    largest = 0
    for rec in limit_records(origin, shape):
        for w in corners + [tuple(o + s // 2 for o, s in zip(origin, shape))]:
            P, v = R.sample_exact(rec, w)
            largest = max(largest, max(abs(p) for p in P))
            assert max(abs(p) for p in P) < 1 << 44
            if max(abs(c) for c in v) >= 1 << 31:
                continue                                       # no model voxel can lie there
            d = np.zeros(tuple(shape)[::-1], dtype=np.float32)
            m = np.zeros(tuple(shape)[::-1], dtype=np.uint32)
            n = AF.stamp_affine_host(d, m, origin, np.array([v], dtype=np.int32), np.array([77], dtype=np.uint32), to_affine(("record", rec)), value=1.0)
            want = np.zeros(tuple(shape)[::-1], dtype=bool)
            for z, y, x in itertools.product(range(shape[2]), range(shape[1]), range(shape[0])):      # (other cells may sample the same voxel: a singular m)
                want[z, y, x] = R.sample_exact(rec, (x + origin[0], y + origin[1], z + origin[2]))[1] == v
            assert want[w[2] - origin[2], w[1] - origin[1], w[0] - origin[0]]
            assert n == int(want.sum()) and ((m == 77) == want).all(), (rec, w)
    assert largest > 13 << 39                                  # the cases come within a factor of two of the header's bound, 13 * 2^40


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_change_nothing():
    origin, shape = (-9, -7, -5), (24, 20, 16)
    d0, m0 = prior_with_empties(shape)
    xyz, mm = R.MODELS["small"]
    good = AF.from_instance(ST.placement((2, 3, 1)))

    def refused(status, rec=good, lo=None, hi=None, mode=R.SET, value=1.0, tag=None):
        d, m = d0.copy(), m0.copy()
        with pytest.raises(BlokError) as e:
            AF.stamp_affine_host(d, m, origin, xyz, mm, rec, lo, hi, mode, value)
        assert e.value.status == status, (tag, e.value.status)
        assert d.tobytes() == d0.tobytes() and m.tobytes() == m0.tobytes(), tag

    def changed(field, value):
        rec = good.copy()
        rec[field] = value
        return rec

    refused(BLOK_ERR_INVALID_ARG, mode=3, tag="mode")
    refused(BLOK_ERR_INVALID_ARG, mode=-1, tag="mode")
    for value in (0.0, -1.0, float("nan"), float("inf")):
        refused(BLOK_ERR_INVALID_ARG, value=value, tag="density")
        refused(BLOK_ERR_INVALID_ARG, value=value, mode=R.KEEP, tag="density")
    refused(BLOK_ERR_INVALID_ARG, rec=changed("reserved", (0, 0, 1, 0, 0)), tag="reserved")
    for bad in ((1 << 22) + 1, -(1 << 22) - 1):
        m = good["m"].copy()
        m[0, 1, 2] = bad
        refused(BLOK_ERR_INVALID_ARG, rec=changed("m", m), tag="m")
        refused(BLOK_ERR_INVALID_ARG, rec=changed("t", (0, bad << 18, 0)), tag="t")
    refused(BLOK_ERR_INVALID_ARG, rec=changed("anchor", (14 - (1 << 20), 0, 0)), tag="anchor below")      # the last cell x = 14 lies 2^20 above
    refused(BLOK_ERR_INVALID_ARG, rec=changed("anchor", (0, 0, -5 + (1 << 20))), tag="anchor above")      # the first cell z = -5 lies 2^20 below
    refused(BLOK_ERR_INVALID_ARG, lo=(0, 0, 0), tag="lo alone")
    refused(BLOK_ERR_INVALID_ARG, hi=(1, 1, 1), tag="hi alone")
    refused(BLOK_ERR_INVALID_ARG, lo=(2, 2, 2), hi=(3, 1, 3), tag="lo above hi")
    refused(BLOK_ERR_UNSUPPORTED, lo=(-10, 0, 0), hi=(3, 3, 3), tag="leaves below")
    refused(BLOK_ERR_UNSUPPORTED, lo=(0, 0, 0), hi=(3, 3, 12), tag="leaves above")
    lib = _ffi.host_lib()
    d, m = d0.copy(), m0.copy()
    n = C.c_uint64(5)
    o = (C.c_int32 * 3)(*origin)
    assert lib.blok_affine_stamp_voxels(_ffi.ptr(d), _ffi.ptr(m), o, 24, 20, 16, _ffi.ptr(xyz), _ffi.ptr(mm), len(xyz), None, None, None, 0, 1.0, C.byref(n)) == BLOK_ERR_INVALID_ARG
    assert n.value == 0
    assert lib.blok_affine_stamp_voxels(_ffi.ptr(d), _ffi.ptr(m), o, 24, 20, 16, None, None, 3, _ffi.ptr(good), None, None, 0, 1.0, C.byref(n)) == BLOK_ERR_INVALID_ARG
    assert d.tobytes() == d0.tobytes() and m.tobytes() == m0.tobytes()
    # legal: the anchor limits met exactly, an empty list, an empty region, ERASE with any density
    assert AF.stamp_affine_host(d, m, origin, xyz, mm, changed("anchor", (14 - (1 << 20) + 1, 0, -5 + (1 << 20) - 1))) >= 0
    d, m = d0.copy(), m0.copy()
    assert AF.stamp_affine_host(d, m, origin, np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.uint32), good) == 0
    assert AF.stamp_affine_host(d, m, origin, xyz, mm, good, (1, 1, 1), (1, 5, 5)) == 0
    assert d.tobytes() == d0.tobytes()
    assert AF.stamp_affine_host(d, m, origin, xyz, mm, good, mode=R.ERASE, value=float("nan")) == len(mm)


# ---- the helpers --------------------------------------------------------------------------------------------------------------------

def permutation_forward(offset, axis, flip):
    """The forward map of a placement: the voxel cube [v, v + 1) of local axis k lands on [o + v, o + v + 1), or [o - 1 - v, o - v) flipped."""
    f = np.zeros((3, 4))
    for k in range(3):
        f[axis[k], k] = -1.0 if (flip >> k) & 1 else 1.0
    f[:, 3] = offset
    return f


def test_from_matrix_gives_from_instances_records():
    rng = np.random.default_rng(9)
    proper = 0
    for axis, flip in SR.ORIENTATIONS:
        offset = tuple(int(v) for v in rng.integers(-30000, 30000, size=3))
        f = permutation_forward(offset, axis, flip)
        proper += int(round(np.linalg.det(f[:, :3]))) == 1
        a, b = AF.from_matrix(f, 3), AF.from_instance(ST.placement(offset, axis, flip, 3))
        assert a.tobytes() == b.tobytes(), (axis, flip, a, b)
    assert proper == 24
    for e in range(9):
        f = R.forward(float(1 << e) * np.eye(3), (11, -7, 5))
        assert AF.from_matrix(f).tobytes() == AF.from_instance(ST.placement((11, -7, 5)), e).tobytes(), e
    # the exponent's cells are the tracer's: floor((w - o) / 2^e), or floor((o - 1 - w) / 2^e) flipped
    for e, (axis, flip) in itertools.product((0, 1, 3, 8), (((0, 1, 2), 0), ((2, 0, 1), 5), ((1, 0, 2), 7))):
        offset = (5, -3, 2)
        rec = AF.from_instance(ST.placement(offset, axis, flip), e)
        for w in itertools.product((-700, -1, 0, 1, 2, 255, 256, 300), repeat=3):
            want = [((offset[axis[k]] - 1 - w[axis[k]]) if (flip >> k) & 1 else (w[axis[k]] - offset[axis[k]])) >> e for k in range(3)]
            assert R.sample_exact(rec, w)[1] == want, (e, axis, flip, w)


def test_from_matrix_and_from_instance_refuse_what_they_must():
    def refused(fn, *args):
        with pytest.raises(BlokError) as e:
            fn(*args)
        assert e.value.status == BLOK_ERR_INVALID_ARG

    eye = R.forward(np.eye(3), (0, 0, 0))
    refused(AF.from_matrix, R.forward(np.zeros((3, 3)), (0, 0, 0)))
    refused(AF.from_matrix, R.forward([[1, 2, 3], [2, 4, 6], [0, 0, 1]], (0, 0, 0)))        # rank 2
    refused(AF.from_matrix, R.forward(np.eye(3) / 65.0, (0, 0, 0)))                         # |m| = 65 * 2^16 > 2^22
    refused(AF.from_matrix, R.forward(np.eye(3), (3e9, 0, 0)))                              # an anchor outside int32
    refused(AF.from_matrix, R.forward(np.eye(3) * np.nan, (0, 0, 0)))
    refused(AF.from_matrix, R.forward(np.eye(3), (np.inf, 0, 0)))
    AF.from_matrix(R.forward(np.eye(3) / 64.0, (0, 0, 0)))                                  # |m| = 2^22 is legal
    assert AF.from_matrix(eye)["anchor"].tolist() == [[0, 0, 0]]
    assert AF.from_matrix(R.forward(np.eye(3), (-0.25, 2.75, -3.0)))["anchor"].tolist() == [[-1, 2, -3]]      # the floor
    refused(AF.from_instance, ST.placement((0, 0, 0)), 9)
    refused(AF.from_instance, ST.placement((0, 0, 0), (0, 0, 2)))
    refused(AF.from_instance, ST.placement((0, 0, 0), flip=8))
    lib = _ffi.host_lib()
    out = np.zeros(1, dtype=_ffi.AFFINE)
    assert lib.blok_affine_from_instance(None, 0, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG
    assert lib.blok_affine_from_instance(_ffi.ptr(ST.placement((0, 0, 0))), 0, None) == BLOK_ERR_INVALID_ARG
    assert lib.blok_affine_from_matrix(None, _ffi.ptr(out)) == BLOK_ERR_INVALID_ARG


def test_rotation_turns_about_the_pivot():
    """rotation() puts the pivot at the position whatever the angles and scale: the cell that holds the position samples the pivot's voxel."""
    for yaw, pitch, roll, scale in ((0.5, 0.0, 0.0, 1.0), (1.0, -0.4, 2.0, 1.5), (-2.0, 0.3, 0.1, 0.5), (0.0, 0.0, 0.0, 2.75)):
        rec = AF.rotation(yaw, pitch, roll, scale, pivot=(3.5, -2.5, 7.5), position=(10.5, 20.5, -30.5), model=4)
        assert R.sample_exact(rec, (10, 20, -31))[1] == [3, -3, 7] and int(rec["model"][0]) == 4
    # a quarter turn about +y: model +x goes to world -z
    rec = AF.rotation(np.pi / 2, pivot=(0.0, 0.0, 0.0), position=(0.0, 0.0, 0.0))
    assert R.sample_exact(rec, (0, 0, -6))[1][0] == 5


# ---- the core header and the host build under sanitizers, in a program of their own -------------------------------------------------

def test_affine_core_at_the_limits_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "affine_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/affine_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/affine.cpp")], check=True)
    run = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split() == ["affine", "ok", "64"], run.stdout
