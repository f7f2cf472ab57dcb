"""GPU: blok_hip_volume_extract_quads against the host build of the same contract (blok_quads_extract) over volume_download(): whole
record arrays bit-equal, after every kind of edit and in both brick layouts; the snapshot's life; the round trip through the voxelizer."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import mesh as M
from blok_amd import terrain as T
from blok_amd._ffi import BlokError
from tests.terrain_cases import params, prior

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5


def _tracer():
    from blok_amd.tracer import HipTracer
    return HipTracer(64, 64).init()


def _same(a, b):
    return np.ascontiguousarray(a, dtype=_ffi.QUAD).tobytes() == np.ascontiguousarray(b, dtype=_ffi.QUAD).tobytes()


def _check(t, origin, lo=None, hi=None, ignore=False, volume=None):
    """The device's records for the region equal the host's over the downloaded volume; returns them."""
    d, m = t.volume_download() if volume is None else volume
    want = M.extract_quads_host(d, m, origin, lo, hi, ignore)
    n_quads, n_faces = M.extract_quads_host.totals
    got = t.volume_extract_quads(lo, hi, ignore)
    print(f"region {lo}..{hi} ignore={ignore}: host {n_quads} quads / {n_faces} faces, device {len(got)} / {t.last_quad_faces}")
    assert (len(got), t.last_quad_faces) == (n_quads, n_faces)
    assert _same(got, want)
    assert t.volume_extract_quads(lo, hi, ignore, count_only=True) == (n_quads, n_faces)
    return got


@pytest.mark.parametrize("keyed", [True, False])
def test_whole_box_and_ragged_regions_over_prior_content(keyed):
    t = _tracer()
    t.set_volume_layout(keyed)
    origin, shape = (-40, -44, -24), (96, 80, 64)
    t.volume_create(origin, shape)
    d0, m0 = prior(shape[::-1])
    d0[::3, ::2, ::5] = -0.5
    d0[1::7, ::3, ::2] = np.nan
    t.volume_upload(d0, m0)
    vol = t.volume_download()
    for ignore in (False, True):
        _check(t, origin, ignore=ignore, volume=vol)
        _check(t, origin, (-31, -39, -13), (38, 21, 30), ignore, vol)         # ragged, unaligned in every axis
        _check(t, origin, (-8, -20, 0), (24, 4, 1), ignore, vol)              # one voxel thick in z
        _check(t, origin, (-40, 3, -24), (56, 4, 40), ignore, vol)            # ... in y
        _check(t, origin, (17, -44, -20), (18, 36, 33), ignore, vol)          # ... in x
    # a denser field whose runs and stacks do merge: terrain over the prior content
    p, _ = params(flags=4)
    t.volume_generate_terrain(p)
    vol = t.volume_download()
    for ignore in (False, True):
        _check(t, origin, ignore=ignore, volume=vol)
        _check(t, origin, (-31, -39, -13), (38, 21, 30), ignore, vol)
    t.shutdown()


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
def test_regions_off_the_brick_grid_of_a_24_13_9_volume(keyed):
    """6 x 4 x 3 bricks, ragged last bricks in y and z, three tree levels: a keyed brick's index is far from its row-major one.  No corner
    of the regions is a multiple of 4."""
    t = _tracer()
    t.set_volume_layout(keyed)
    origin, shape = (-7, 3, -2), (24, 13, 9)
    t.volume_create(origin, shape)
    rng = np.random.default_rng(29)
    d0 = np.where(rng.random(shape[::-1]) < 0.45, rng.uniform(0.1, 2.0, shape[::-1]), 0.0).astype(np.float32)
    d0[::3, ::2, ::5] = -0.5
    m0 = np.where(d0 > 0, rng.integers(5, 8, shape[::-1]), 0).astype(np.uint32)
    t.volume_upload(d0, m0)
    vol = t.volume_download()
    for ignore in (False, True):
        _check(t, origin, ignore=ignore, volume=vol)
        for lo, hi in (((1, 1, 1), (22, 11, 7)), ((5, 2, 3), (19, 10, 6)), ((17, 1, 5), (23, 13, 9)), ((2, 6, 1), (3, 7, 2))):      # box-local
            assert all(c % 4 for c in lo + hi)
            _check(t, origin, tuple(o + c for o, c in zip(origin, lo)), tuple(o + c for o, c in zip(origin, hi)), ignore, vol)
    t.shutdown()


def test_terrain_with_caves_in_256_cubed():
    t = _tracer()
    origin, shape = (-128, -100, -128), (256, 256, 256)
    t.volume_create(origin, shape)
    p = T.default_params(256, 7)
    p.base_height -= 100
    assert p.cave_octaves > 0
    assert t.volume_generate_terrain(p) > 0
    q = _check(t, origin)
    assert int((q["du"].astype(np.int64) * q["dv"]).sum()) == t.last_quad_faces
    _check(t, origin, ignore=True)
    t.shutdown()


def test_after_voxelize_brushes_and_set_voxels():
    from tests import voxelize_meshes as VM
    t = _tracer()
    origin, shape = (-64, -64, -64), (160, 128, 128)
    t.volume_create(origin, shape, chunk_size=64)
    pos, tri = VM.icosphere([3.3, 1.7, -2.2], 40.0, 3)
    assert t.volume_voxelize_mesh(pos, tri, material=5, solid=True) > 0
    _check(t, origin)
    pos, tri = VM.icosphere([60.0, 20.0, 30.0], 25.5, 3)
    mats = (np.arange(len(tri)) % 3 + 7).astype(np.uint32)
    assert t.volume_voxelize_mesh(pos, tri, mats, solid=False) > 0
    _check(t, origin)
    # brushes across brick and chunk borders (chunk edge 64: world 0 and 64 are borders)
    t.volume_apply_brush((0.5, 0.5, 0.5), 13.0, -1.0, 1)          # SUBTRACT through the solid sphere's centre
    _check(t, origin)
    t.volume_apply_brush((63.5, 0.0, 1.5), 9.5, 0.8, 0)           # ADD across x = 64
    _check(t, origin)
    t.volume_apply_brush((30.0, 38.0, -20.0), 7.0, 0.0, 1)        # SUBTRACT to exactly 0: empty
    _check(t, origin)
    rng = np.random.default_rng(5)
    xyz = (rng.integers(-45, 45, (4000, 3))).astype(np.int32)
    dens = rng.choice(np.array([1.0, 0.0, -1.0, -0.0, np.nan], np.float32), 4000)
    t.volume_set_voxels(xyz, rng.integers(1, 4, 4000).astype(np.uint32), dens)
    _check(t, origin)
    _check(t, origin, (-50, -47, -33), (51, 40, 48), True)
    t.shutdown()


def test_checkerboard_is_the_worst_case():
    t = _tracer()
    t.volume_create((0, 0, 0), (64, 64, 64))
    z, y, x = np.indices((64, 64, 64))
    d = ((x + y + z) % 2 == 0).astype(np.float32)
    t.volume_upload(d, np.ones((64, 64, 64), np.uint32))
    assert t.volume_extract_quads(count_only=True) == (786432, 786432)
    _check(t, (0, 0, 0), volume=(d, np.ones((64, 64, 64), np.uint32)))
    t.shutdown()


def test_full_256_box_is_six_quads():
    t = _tracer()
    origin = (-256, 0, 100)
    t.volume_create(origin, (256, 256, 256))
    t.volume_upload(np.ones((256, 256, 256), np.float32), np.full((256, 256, 256), 9, np.uint32))
    q = t.volume_extract_quads()
    assert len(q) == 6 and t.last_quad_faces == 6 * 256 * 256
    assert (q["du"] == 256).all() and (q["dv"] == 256).all() and (q["material"] == 9).all() and q["face"].tolist() == list(range(6))
    assert q["lo"].tolist() == [[0, 0, 100], [-256, 0, 100], [-256, 256, 100], [-256, 0, 100], [-256, 0, 356], [-256, 0, 100]]
    t.shutdown()


def test_snapshot_life_paging_and_determinism():
    t = _tracer()
    origin, shape = (-32, -40, -32), (64, 64, 64)
    t.volume_create(origin, shape)
    p, _ = params()
    t.volume_generate_terrain(p)
    a = t.volume_extract_quads()
    assert len(a) == 12996 and t.last_quad_faces == 39470          # the contract's quoted case
    b = t.volume_extract_quads()
    assert a.tobytes() == b.tobytes()                                # two runs give identical bytes
    # COUNT_ONLY leaves the previous snapshot downloadable
    assert t.volume_extract_quads((-20, -30, -20), (20, 20, 20), count_only=True) == (5237, 10932)
    assert t.volume_quads_download(0, len(a)).tobytes() == a.tobytes()
    # paged download equals one download
    assert t.volume_quads_download(0, len(a), page=1000).tobytes() == a.tobytes()
    assert t.volume_quads_download(5000, 77).tobytes() == a[5000:5077].tobytes()
    assert len(t.volume_quads_download(len(a), 0)) == 0
    # the snapshot is unchanged by a later edit
    t.volume_apply_brush((0.0, 0.0, 0.0), 12.0, -1.0, 1)
    t.volume_generate_terrain(T.default_params(64, 3), (-32, -40, -32), (0, 24, 32))
    assert t.volume_quads_download(0, len(a)).tobytes() == a.tobytes()
    c = _check(t, origin)
    assert c.tobytes() != a.tobytes()
    # an empty region: OK, zero counts, an empty snapshot
    assert len(t.volume_extract_quads((0, 0, 0), (0, 10, 10))) == 0
    with pytest.raises(BlokError):
        t.volume_quads_download(0, 1)
    t.shutdown()


def _raw(t, lo, hi, flags):
    arr = lambda v: None if v is None else (C.c_int32 * 3)(*v)
    nq, nf = C.c_uint64(99), C.c_uint64(99)
    rc = t._lib.blok_hip_volume_extract_quads(t._ctx, arr(lo), arr(hi), flags, C.byref(nq), C.byref(nf))
    return rc, int(nq.value), int(nf.value)


def test_error_table_leaves_the_snapshot():
    t = _tracer()
    out = np.zeros(4, dtype=_ffi.QUAD)
    assert _raw(t, None, None, 0)[0] == BLOK_ERR_NO_WORLD
    assert t._lib.blok_hip_volume_quads_download(t._ctx, _ffi.ptr(out), 0, 1) == BLOK_ERR_INVALID_ARG      # no snapshot
    origin, shape = (10, 20, 30), (24, 20, 16)
    t.volume_create(origin, shape)
    t.volume_upload(np.ones(shape[::-1], np.float32), np.ones(shape[::-1], np.uint32))
    a = t.volume_extract_quads()
    assert len(a) == 6
    for lo, hi, flags, want in [(None, None, 4, BLOK_ERR_INVALID_ARG), (None, None, 0x80000001, BLOK_ERR_INVALID_ARG),
                                ((10, 20, 30), None, 0, BLOK_ERR_INVALID_ARG), (None, (34, 40, 46), 0, BLOK_ERR_INVALID_ARG),
                                ((12, 20, 30), (11, 40, 46), 0, BLOK_ERR_INVALID_ARG), ((9, 20, 30), (34, 40, 46), 0, BLOK_ERR_UNSUPPORTED),
                                ((10, 20, 30), (34, 40, 47), 0, BLOK_ERR_UNSUPPORTED)]:
        assert _raw(t, lo, hi, flags) == (want, 0, 0), (lo, hi, flags)
        assert t.volume_quads_download(0, 6).tobytes() == a.tobytes()                                      # nothing replaced
    assert t._lib.blok_hip_volume_quads_download(t._ctx, _ffi.ptr(out), 3, 4) == BLOK_ERR_INVALID_ARG      # past the end
    assert t._lib.blok_hip_volume_quads_download(t._ctx, _ffi.ptr(out), 7, 0) == BLOK_ERR_INVALID_ARG
    assert t._lib.blok_hip_volume_quads_download(t._ctx, None, 0, 2) == BLOK_ERR_INVALID_ARG
    assert t._lib.blok_hip_volume_quads_download(t._ctx, _ffi.ptr(out), 2, 4) == 0 and out.tobytes() == a[2:6].tobytes()
    t.volume_destroy()                                                                                       # frees the snapshot
    assert t._lib.blok_hip_volume_quads_download(t._ctx, _ffi.ptr(out), 0, 1) == BLOK_ERR_INVALID_ARG
    t.shutdown()


def _dilate26(v):
    p = np.pad(v, 1)
    out = np.zeros_like(v)
    n = v.shape
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= p[dz:dz + n[0], dy:dy + n[1], dx:dx + n[2]]
    return out


def test_round_trip_through_the_voxelizer():
    """quads_to_triangles(extract(V)) voxelized into an emptied volume of the same box: SOLID gives exactly the 26-neighbourhood dilation
    of V, SURFACE that dilation minus the voxels of V whose 26 neighbours are all in V (column centres never lie on lattice planes, so
    the interior is V; the surface set is every voxel whose closed cube touches the boundary of V)."""
    t = _tracer()
    origin, n = (-20, 5, -31), 48
    t.volume_create(origin, (n, n, n))
    rng = np.random.default_rng(12)
    v = np.zeros((n, n, n), bool)
    v[1:-1, 1:-1, 1:-1] = rng.random((n - 2, n - 2, n - 2)) < 0.15
    z, y, x = np.indices((n, n, n))
    v |= (x - 24) ** 2 + (y - 22) ** 2 + (z - 25) ** 2 < 15 ** 2          # a body with a real interior
    v[[0, -1]] = False; v[:, [0, -1]] = False; v[:, :, [0, -1]] = False    # V stays one voxel inside the box
    t.volume_upload(v.astype(np.float32), np.where(v, 3, 0).astype(np.uint32))
    q = t.volume_extract_quads()
    pos, tri, mats = M.quads_to_triangles(q)
    assert len(tri) == 2 * len(q) and (mats == 3).all()
    dil = _dilate26(v)
    inner = ~_dilate26(~v) & v                                              # all 26 neighbours in V
    assert inner.any()
    for solid, want in ((True, dil), (False, dil & ~inner)):
        t.volume_upload(None, None)
        written = t.volume_voxelize_mesh(pos, tri, mats, density=1.0, solid=solid)
        d, _ = t.volume_download()
        print(f"round trip solid={solid}: V {int(v.sum())}, quads {len(q)}, written {written}, expected {int(want.sum())}")
        assert np.array_equal(d > 0, want)
    t.shutdown()


def test_headless_driver_exports_the_terrain_as_obj(tmp_path):
    import re
    import subprocess
    from blok_amd import build as b
    from blok_amd.mesh import ObjMesh
    from blok_amd.vox import MaterialLibrary
    exe = b.build_tools()
    out = tmp_path / "terrain.obj"
    proc = subprocess.run([str(exe), "--terrain", "0xB10C0001", "--terrain-size", "64", "--size", "160x100", "--frames", "1", "--out", str(tmp_path / "f.ppm"),
                           "--export-obj", str(out)], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    found = re.search(r"surface: (\d+) exposed faces -> (\d+) quads", proc.stdout)
    assert found, proc.stdout
    n_quads = int(found.group(2))
    assert n_quads > 0 and (tmp_path / "terrain.mtl").exists()
    lib = MaterialLibrary()
    mesh = ObjMesh.load_file(out, lib)
    assert len(mesh.triangles) == 2 * n_quads
    # the same world made here gives the same count
    t = _tracer()
    t.volume_create((0, 0, 0), (64, 64, 64))
    t.volume_generate_terrain(T.default_params(64, 0xB10C0001))
    assert t.volume_extract_quads(count_only=True)[0] == n_quads
    t.shutdown()
    proc = subprocess.run([str(exe), "--n", "64", "--frames", "1", "--export-obj", str(out)], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 1 and "--export-obj needs a resident volume" in proc.stderr
