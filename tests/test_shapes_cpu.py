"""CPU: the shape table on the host (blok_shapes_check, blok_shape_bounds, blok_shapes_voxels) against the numpy model
(tests/shapes_reference.py).  Every comparison is exact: integers, or floats copied or selected, never computed."""
from __future__ import annotations

import itertools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import shapes as SH
from blok_amd._ffi import BlokError
from tests import shapes_cases as K
from tests import shapes_reference as R

ROOT = Path(__file__).resolve().parent.parent
ORIGIN, DIMS = K.CPU_ORIGIN, K.CPU_SHAPE


def both(shapes, origin=ORIGIN, dims=DIMS, seed=5):
    """The table on the model and on the host build, from the same pre-state: the arrays and the count agree.  Returns (count, d, m, d0, m0)."""
    d0, m0 = R.noise(dims, seed)
    d, m = d0.copy(), m0.copy()
    want = R.apply(d, m, origin, shapes)
    hd, hm = d0.copy(), m0.copy()
    got = SH.apply_host(hd, hm, origin, R.record(shapes))
    assert got == want, (got, want)
    assert R.same(hd, d), int((hd.view(np.uint32) != d.view(np.uint32)).sum())
    assert R.same(hm, m), int((hm != m).sum())
    return want, d, m, d0, m0


# ---- the record -------------------------------------------------------------------------------------------------------------------------
def test_record_size_and_constants():
    assert _ffi.SHAPE.itemsize == 64
    text = (ROOT / "include" / "blok_hip.h").read_text()
    src = ("#include \"blok_hip.h\"\n#include <stddef.h>\n_Static_assert(sizeof(blok_shape) == 64 && offsetof(blok_shape, a) == 8 && offsetof(blok_shape, r) == 32 && "
           "offsetof(blok_shape, value) == 52 && BLOK_SHAPE_CYLINDER == 3 && BLOK_SHAPE_SUBTRACT == 6 && BLOK_SHAPES_MAX == 65536, \"layout\");\nint main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", "-fsyntax-only", "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "} blok_shape;" in text and "64 bytes */" in text.split("} blok_shape;")[1].splitlines()[0]
    assert _ffi.SHAPE.fields["a"][1] == 8 and _ffi.SHAPE.fields["r"][1] == 32 and _ffi.SHAPE.fields["value"][1] == 52
    assert (R.BOX, R.CYLINDER, R.SET, R.SUBTRACT, R.SHAPES_MAX) == (_ffi.SHAPE_BOX, _ffi.SHAPE_CYLINDER, _ffi.SHAPE_SET, _ffi.SHAPE_SUBTRACT, _ffi.SHAPES_MAX)
    assert _ffi.hip_lib().blok_hip_abi_version() >= (1 << 16) | 15      # the ABI that brought the entry


def test_builders_make_the_records_the_model_builds():
    want = R.record([R.vbox((-3, 2, 1), (4, 5, 6), R.KEEP, material=3, value=0.5),
                     R.shape(R.ELLIPSOID, R.ADD, a=(5, -3, 8), r=(4, 6, 9), value=0.25),
                     R.shape(R.ELLIPSOID, R.PAINT, a=(4, 4, 4), r=(7, 7, 7), material=2),
                     R.shape(R.CAPSULE, R.REPLACE, a=(1, 3, 5), b=(9, -3, 6), r=(5, 0, 0), material=6, match=2),
                     R.shape(R.CYLINDER, R.ERASE, a=(1, 3, 5), b=(9, -3, 6), r=(4, 0, 0)),
                     R.shape(R.CAPSULE, R.SUBTRACT, a=(1, 1, 1), b=(3, 3, 3), r=(3, 0, 0), value=0.0),
                     R.shape(R.CAPSULE, R.SUBTRACT, a=(3, 3, 3), b=(5, 3, 4), r=(3, 0, 0), value=0.0)])
    got = np.concatenate([SH.box((-3, 2, 1), (4, 5, 6), SH.KEEP, 3, 0.5), SH.ellipsoid((2.5, -1.5, 4), (2, 3, 4.5), SH.ADD, value=0.25),
                          SH.sphere((2, 2, 2), 3.5, SH.PAINT, 2), SH.capsule((0.5, 1.5, 2.5), (4.5, -1.5, 3), 2.5, SH.REPLACE, 6, match=2),
                          SH.cylinder((0.5, 1.5, 2.5), (4.5, -1.5, 3), 2, SH.ERASE),
                          SH.stroke([(0.5, 0.5, 0.5), (1.5, 1.5, 1.5), (2.5, 1.5, 2)], 1.5, SH.SUBTRACT, value=0.0)])
    assert got.tobytes() == want.tobytes()
    assert SH.stroke([(1, 2, 3)], 2).tobytes() == R.record([R.shape(R.CAPSULE, R.ADD, a=(2, 4, 6), b=(2, 4, 6), r=(4, 0, 0))]).tobytes()


# ---- the host build against the model -------------------------------------------------------------------------------------------------------
def test_the_pre_state_holds_what_the_operations_tell_apart():
    d, m = R.noise(DIMS)
    w = d.view(np.uint32)
    assert (w == 0x80000000).any() and (w == 0).any() and np.isnan(d).any() and (d < 0).any()
    assert ((d > 0) & (m == 0)).any() and (~R.filled(d) & (m != 0)).any() and ((d > 0) & (m == 3)).any()


@pytest.mark.parametrize("tag,shapes", K.kinds_by_ops(ORIGIN, DIMS), ids=lambda v: v if isinstance(v, str) else "")
def test_every_kind_and_op(tag, shapes):
    n, d, m, d0, m0 = both(shapes)
    op = shapes[0]["op"]
    assert n > 200, (tag, n)
    changed_d, changed_m = not R.same(d, d0), not R.same(m, m0)
    assert changed_d == (op not in (R.PAINT, R.REPLACE)) and changed_m == (op not in (R.ADD, R.SUBTRACT)), tag      # every op does its own thing


@pytest.mark.parametrize("tag,shapes", K.placements(ORIGIN, DIMS) + K.zero_radii(ORIGIN, DIMS), ids=lambda v: v if isinstance(v, str) else "")
def test_centres_on_voxel_centres_faces_and_corners_and_zero_radii(tag, shapes):
    n, *_ = both(shapes)
    assert (n == 0) == (tag == "point off every centre"), (tag, n)
    expected = {"ellipsoid r (0, 0, 0)": 1, "ellipsoid r (0, 0, 10)": 11, "ellipsoid r (14, 0, 0)": 15, "ellipsoid r (0, 12, 0)": 13, "capsule r 0": 9, "cylinder r 0": 9}
    if tag in expected:                                            # a point, the three segments (2 (r / 2) + 1 centres), a segment of 16 half-voxels
        assert n == expected[tag], (tag, n)


def test_a_capsule_with_equal_ends_is_the_sphere():
    for a, radius in itertools.product(((21, 43, -9), (22, 43, -9), (22, 42, -10)), (0, 5, 8, 11)):
        capsule = [R.shape(R.CAPSULE, R.SET, a=a, b=a, r=(radius, 0, 0), material=4, value=1.0)]
        sphere = [R.shape(R.ELLIPSOID, R.SET, a=a, r=(radius,) * 3, material=4, value=1.0)]
        n1, d1, m1, *_ = both(capsule)
        n2, d2, m2, *_ = both(sphere)
        assert n1 == n2 and R.same(d1, d2) and R.same(m1, m2), (a, radius)


def test_clipping_at_each_face_and_wholly_outside():
    for op in (R.SET, R.ERASE, R.ADD, R.PAINT):
        for tag, shapes in K.clipped(ORIGIN, DIMS, op):
            n, *_ = both(shapes)
            full = sum(int(np.prod([hi - lo for lo, hi in zip(*SH.bounds_host(R.record([s])))])) for s in shapes)
            assert 0 < n < full, (tag, op, n, full)                # some of it lands inside, and not all of it
    outside = K.outside(ORIGIN, DIMS)
    for s in outside:
        n, d, m, d0, m0 = both([s])
        assert n == 0 and R.same(d, d0) and R.same(m, m0)
    assert both(outside)[0] == 0
    assert both([])[0] == 0


def test_order_matters_and_is_kept():
    pair = K.order_pair(ORIGIN, DIMS)
    d0, m0 = R.noise(DIMS)
    d1, m1, d2, m2 = d0.copy(), m0.copy(), d0.copy(), m0.copy()
    R.apply(d1, m1, ORIGIN, pair)
    R.apply(d2, m2, ORIGIN, pair[::-1])
    assert not R.same(m1, m2), "the reversed table gives the same arrays: the case shows nothing"
    both(pair)
    both(pair[::-1])


def test_a_table_of_many_overlapping_shapes():
    shapes = K.stroke(ORIGIN, DIMS, R.ADD, value=0.75) + K.stroke(ORIGIN, DIMS, R.KEEP, radius=9, material=8) + K.stroke(ORIGIN, DIMS, R.PAINT, material=77)
    assert both(shapes)[0] > 10000


# ---- shape_bounds ---------------------------------------------------------------------------------------------------------------------------
def bound_shapes():
    out = []
    for a in ((-41, -23, -5), (-40, -23, -6), (-40, -22, -6), (-39, -24, -7)):
        out.append(R.shape(R.BOX, R.SET, a=a, b=(a[0] + 9, a[1] + 4, a[2] + 1)))
        out.append(R.shape(R.BOX, R.SET, a=a, b=a))
        for r in ((0, 0, 0), (1, 2, 3), (4, 4, 4), (6, 3, 8), (7, 7, 7)):
            out.append(R.shape(R.ELLIPSOID, R.SET, a=a, r=r))
        for r in (0, 1, 2, 5, 6):
            out.append(R.shape(R.CAPSULE, R.SET, a=a, b=(a[0] + 6, a[1] - 10, a[2] + 4), r=(r, 0, 0)))
            out.append(R.shape(R.CYLINDER, R.SET, a=a, b=(a[0] - 8, a[1] + 2, a[2] + 4), r=(r, 0, 0)))
    return out


def test_shape_bounds_hold_every_inside_voxel_and_are_tight():
    """Brute force over a margin of 4 voxels around the rule's extent, at negative coordinates.  The box holds every inside voxel; per axis it
    is exactly the voxels whose centre lies in the rule's extent (the smallest w with 2 w + 1 >= lo, the largest with 2 w + 1 <= hi, found here
    by search, not by division); and where the extent's ends can be reached — a BOX, or a shape on voxel centres with an even radius, whose
    extreme points c = a +- r are centres — every face of the box holds an inside voxel."""
    reached = 0
    for s in bound_shapes():
        lo, hi = SH.bounds_host(R.record([s]))
        ext = [R.extent(s, k) for k in range(3)]
        want_lo = [min((w for w in range(-60, 40) if 2 * w + 1 >= ext[k][0]), default=None) for k in range(3)]
        want_hi = [max((w for w in range(-60, 40) if 2 * w + 1 <= ext[k][1]), default=None) for k in range(3)]
        empty = any(want_lo[k] > want_hi[k] for k in range(3))
        if not empty:
            assert (list(lo), list(hi)) == (want_lo, [w + 1 for w in want_hi]), s
        else:
            assert any(lo[k] >= hi[k] for k in range(3)), s
        g_lo = [ext[k][0] // 2 - 4 for k in range(3)]
        dims = [ext[k][1] // 2 + 5 - g_lo[k] for k in range(3)]
        sel = np.broadcast_to(R.inside(s, R.centres(g_lo, dims)), dims[::-1])
        z, y, x = np.nonzero(sel)
        w = np.stack([x + g_lo[0], y + g_lo[1], z + g_lo[2]], axis=1)
        if len(w):
            assert (w >= np.array(lo)).all() and (w < np.array(hi)).all(), s
        on_centres = all(c % 2 for c in s["a"]) and (s["kind"] == R.ELLIPSOID or all(c % 2 for c in s["b"])) and all(r % 2 == 0 for r in s["r"])
        if (s["kind"] == R.BOX and not empty) or (s["kind"] in (R.ELLIPSOID, R.CAPSULE) and on_centres):
            assert len(w) and (w.min(axis=0) == np.array(lo)).all() and (w.max(axis=0) + 1 == np.array(hi)).all(), s
            reached += 1
    assert reached >= 8


# ---- the arithmetic at every limit -----------------------------------------------------------------------------------------------------------
def limit_probes():
    """[(shape, [world voxel corners of 4^3 probe boxes])]: radius 1024, segments of 4096 per axis, coordinates at +-2^17; probes at the corners
    of the extent (the largest products), on the surface and at the centre."""
    top = R.COORD_MAX
    out = []
    for a in ((top - 1, -top + 1, top - 1), (-top + 1, top - 1, -top + 1)):
        s = R.shape(R.ELLIPSOID, R.SET, a=a, r=(1024, 1024, 1024), material=1)
        c = [v // 2 for v in a]
        out.append((s, [tuple(c[k] + o[k] for k in range(3)) for o in ((510, 510, 510), (-514, -514, -514), (294, 294, 294), (-297, -297, -297), (510, -2, -2), (-2, -2, -2),
                                                                        (360, 360, -2), (-364, -2, 360))]))
    for sign in (1, -1):
        a = (-sign * top, sign * top, -sign * top)
        b = (a[0] + sign * 4096, a[1] - sign * 4096, a[2] + sign * 4096)
        for kind in (R.CAPSULE, R.CYLINDER):
            s = R.shape(kind, R.SET, a=a, b=b, r=(1024, 0, 0), material=1)
            ca, cb = [v // 2 for v in a], [v // 2 for v in b]
            mid = [(ca[k] + cb[k]) // 2 for k in range(3)]
            probes = [tuple(cb[k] + sg * (o if k != 1 else -o) - 2 for k in range(3)) for sg in (sign,) for o in (512, 294, 0)]
            probes += [tuple(ca[k] - sign * (o if k != 1 else -o) - 2 for k in range(3)) for o in (512, 294, 0)]
            probes += [(mid[0] + 360 - 2, mid[1] - 2, mid[2] - 360 - 2), (mid[0] - 2, mid[1] + 362 - 2, mid[2] + 362 - 2), (mid[0] + 209 - 2, mid[1] + 418 - 2, mid[2] + 209 - 2)]
            out.append((s, probes))
    return out


def test_the_int64_core_equals_python_integers_at_every_limit():
    seen = {True: 0, False: 0}
    largest = 0
    for s, probes in limit_probes():
        assert SH.check_host(R.record([s])) is None
        for corner in probes:
            d, m = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.uint32)
            SH.apply_host(d, m, corner, R.record([s]))
            for z, y, x in itertools.product(range(4), repeat=3):
                c = tuple(2 * (corner[k] + v) + 1 for k, v in enumerate((x, y, z)))
                want = bool(R.inside(s, c))                           # Python integers: exact
                assert bool(m[z, y, x]) == want, (s, corner, (x, y, z))
                seen[want] += 1
                if all(R.extent(s, k)[0] <= c[k] <= R.extent(s, k)[1] for k in range(3)):
                    if s["kind"] == R.ELLIPSOID:
                        largest = max(largest, sum((c[k] - s["a"][k]) ** 2 for k in range(3)) * 1024 ** 4)
                    else:
                        dd = sum((s["b"][k] - s["a"][k]) ** 2 for k in range(3))
                        largest = max(largest, sum((c[k] - s["a"][k]) ** 2 for k in range(3)) * dd)
    assert seen[True] > 300 and seen[False] > 300, seen
    assert 2 ** 61 < largest < 3 * 2 ** 60 + 1, largest              # the probes reach the corner of the ellipsoid's extent: the contract's bound


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def test_limits_are_inclusive():
    top = R.COORD_MAX
    for s in (R.shape(R.BOX, R.SET, a=(-top,) * 3, b=(top,) * 3), R.shape(R.ELLIPSOID, R.SUBTRACT, a=(top, -top, 0), r=(1024, 0, 1024), value=-3.0),
              R.shape(R.CAPSULE, R.ADD, a=(0, 0, 0), b=(4096, -4096, 4096), r=(1024, 0, 0), value=0.0), R.shape(R.CYLINDER, R.ERASE, a=(0, 0, 0), b=(0, 0, 1))):
        assert SH.check_host(R.record([s])) is None, s


def test_each_error_names_the_index_and_writes_nothing():
    good = R.vbox((-5, 5, -18), (20, 30, 5), R.SET, material=2, value=1.0)
    lib = _ffi.host_lib()
    d0, m0 = R.noise(DIMS)
    for text, bad in K.bad_shapes():
        for at in (0, 2):
            table = [good, good, good]
            table[at] = bad
            found = SH.check_host(R.record(table))
            assert found is not None and found[0] == at and f"shape {at}: " in found[1] and text in found[1], (text, found)
            d, m = d0.copy(), m0.copy()
            with pytest.raises(BlokError) as e:
                SH.apply_host(d, m, ORIGIN, R.record(table))
            assert e.value.status == R.INVALID_ARG and f"shape {at}" in str(e.value)
            assert R.same(d, d0) and R.same(m, m0), text
        with pytest.raises(BlokError):
            SH.bounds_host(R.record([bad]))
    d, m = d0.copy(), m0.copy()
    n = np.zeros(1, np.uint64)
    import ctypes as C
    origin = (C.c_int32 * 3)(*ORIGIN)
    count = C.c_uint64(9)
    assert lib.blok_shapes_voxels(_ffi.ptr(d), _ffi.ptr(m), origin, *DIMS, None, 2, C.byref(count)) == R.INVALID_ARG and count.value == 0      # a null table
    assert SH.check_host(np.zeros(0, _ffi.SHAPE)) is None and lib.blok_shapes_check(None, 1, None, None, 0) == R.INVALID_ARG
    many = np.repeat(R.record([good]), R.SHAPES_MAX + 1)
    assert SH.check_host(many[:R.SHAPES_MAX]) is None
    assert SH.check_host(many) is not None and "BLOK_SHAPES_MAX" in SH.check_host(many)[1]
    assert lib.blok_shapes_voxels(_ffi.ptr(d), _ffi.ptr(m), origin, *DIMS, _ffi.ptr(many), len(many), None) == R.INVALID_ARG
    assert lib.blok_shapes_voxels(None, _ffi.ptr(m), origin, *DIMS, _ffi.ptr(many), 1, None) == R.INVALID_ARG
    assert lib.blok_shapes_voxels(_ffi.ptr(d), _ffi.ptr(m), origin, 0, 4, 4, _ffi.ptr(many), 1, None) == R.INVALID_ARG
    assert R.same(d, d0) and R.same(m, m0) and not n.any()


# ---- the host build under the sanitizers -----------------------------------------------------------------------------------------------------
def _checksum(a) -> int:
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_host_build_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/shapes_main.cpp) over case files: small tables of every kind, clipped and outside, at the
    limits, and every refusal; nothing loaded into Python is sanitized."""
    exe = tmp_path / "shapes_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/shapes_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/shapes.cpp")], check=True)
    small_origin, small = (-9, 2, -13), (21, 18, 17)
    jobs = [(small_origin, small, shapes) for _, shapes in K.kinds_by_ops(small_origin, small)[::3]]
    jobs += [(small_origin, small, shapes) for _, shapes in K.clipped(small_origin, small)]
    jobs.append((small_origin, small, K.outside(small_origin, small)))
    jobs.append((small_origin, small, K.stroke(small_origin, small, R.ADD, n=12, radius=5, value=0.75) + K.stroke(small_origin, small, R.PAINT, n=9, radius=6, material=7)))
    jobs += [(corner, (4, 4, 4), [s]) for s, probes in limit_probes() for corner in probes[:2]]
    jobs += [(small_origin, small, [bad]) for _, bad in K.bad_shapes()]
    files, want = [], []
    for i, (origin, dims, shapes) in enumerate(jobs):
        d, m = R.noise(dims, seed=i)
        table = R.record(shapes)
        path = tmp_path / f"case{i}.bin"
        path.write_bytes(np.array(list(dims) + list(origin) + [len(table)], dtype=np.int32).tobytes() + table.tobytes() + d.tobytes() + m.tobytes())
        files.append(os.fspath(path))
        if SH.check_host(table) is not None:
            want.append(f"{R.INVALID_ARG} {R.INVALID_ARG} 0 {_checksum(d)} {_checksum(m)}")
        else:
            n = R.apply(d, m, origin, shapes)
            want.append(f"0 0 {n} {_checksum(d)} {_checksum(m)}")
    run = subprocess.run([os.fspath(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.splitlines() == want
