"""GPU: blok_hip_volume_voxelize_mesh against the CPU shim of its exact tests (tests/host_harness/voxelize_shim.cpp), bit for bit on the
volume's arrays, and the bookkeeping it leaves for the rebuild."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd._ffi import BlokError
from tests import voxelize_meshes as M
from tests.test_voxelize_cpu import shim, shim_voxelize      # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD = -1, -4


def _tracer():
    from blok_amd.tracer import HipTracer
    return HipTracer(64, 64).init()


def _bumpy(v):
    return 0.08 * np.sin(5.0 * v[:, 0]) * np.cos(4.0 * v[:, 1]) + 0.05 * np.sin(7.0 * v[:, 2])


def _prior(shape, seed=1):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    d = np.where(rng.random((nz, ny, nx)) < 0.05, rng.uniform(0.1, 2.0, (nz, ny, nx)), 0.0).astype(np.float32)
    m = np.where(d > 0, rng.integers(1, 9, (nz, ny, nx)), 0).astype(np.uint32)
    return d, m


def _compare(shim, t, pos, tri, origin, shape, materials=None, solid=False, prior=True, material=3, density=1.5):
    d0, m0 = _prior(shape) if prior else (np.zeros(shape[::-1], np.float32), np.zeros(shape[::-1], np.uint32))
    t.volume_create(origin, shape)
    t.volume_upload(d0, m0)
    n = t.volume_voxelize_mesh(pos, tri, materials=materials, material=material, density=density, solid=solid)
    d, m = t.volume_download()
    rc, dr, mr, nr = shim_voxelize(shim, pos, tri, origin, shape, materials=materials, material=material, density=density, solid=solid,
                                   dens=d0, ids=m0)
    assert rc == 0
    assert np.array_equal(d.view(np.uint32), dr.view(np.uint32))
    assert np.array_equal(m, mr)
    assert n == nr
    return d, m


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("solid", [False, True])
@pytest.mark.parametrize("per_triangle", [False, True])
def test_arrays_equal_the_shim(shim, keyed, solid, per_triangle):
    t = _tracer()
    t.set_volume_layout(keyed)
    pos, tri = M.merge(M.icosphere([30.3, 28.7, 33.1], 21.0, 4, _bumpy), M.torus([30.0, 31.0, 30.0], 14.0, 4.0, 40, 16))
    mats = (np.arange(len(tri)) % 13 + 2).astype(np.uint32) if per_triangle else None
    _compare(shim, t, pos, tri, (0, 0, 0), (64, 64, 64), materials=mats, solid=solid)
    t.shutdown()


@pytest.mark.parametrize("solid", [False, True])
def test_large_displaced_icosphere(shim, solid):
    t = _tracer()
    pos, tri = M.icosphere([128.2, 127.6, 128.9], 110.0, 7, _bumpy)                 # 327 680 triangles
    assert len(tri) > 300_000
    mats = (np.arange(len(tri)) % 256).astype(np.uint32)
    _compare(shim, t, pos, tri, (0, 0, 0), (256, 256, 256), materials=mats, solid=solid, prior=False)
    t.shutdown()


def test_mesh_partly_outside_a_ragged_box(shim):
    t = _tracer()
    pos, tri = M.merge(M.icosphere([-10.0, 20.0, 5.0], 30.0, 4), M.torus([30.0, 40.0, 40.0], 20.0, 6.0, 48, 16))
    for solid in (False, True):
        _compare(shim, t, pos, tri, (-37, 3, -11), (83, 61, 67), solid=solid)
    t.shutdown()


def test_single_triangle_across_the_box_diagonally(shim):
    t = _tracer()
    pos = np.array([[0.3, 0.2, 0.4], [255.7, 255.1, 10.0], [20.0, 240.0, 255.6]], np.float32)
    _compare(shim, t, pos, np.array([[0, 1, 2]], np.uint32), (0, 0, 0), (256, 256, 256), prior=False)
    t.shutdown()


def test_pair_list_spans_several_batches(shim):
    t = _tracer()
    rng = np.random.default_rng(11)
    n = 4_600_000                                             # > 2^22 candidate pairs
    c = rng.uniform(1.0, 127.0, (n, 1, 3))
    pos = (c + rng.uniform(-0.8, 0.8, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    tri = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    mats = (np.arange(n) % 97 + 1).astype(np.uint32)
    _compare(shim, t, pos, tri, (0, 0, 0), (128, 128, 128), materials=mats, prior=False)
    t.shutdown()


def test_rebuild_equals_a_fresh_upload():
    """Masks, occupancy words and dirty flags as an upload of the same arrays leaves them: the same tree, also after a brush on top."""
    a, b = _tracer(), _tracer()
    origin, shape = (-5, 2, -9), (90, 70, 80)
    pos, tri = M.icosphere([35.0, 40.0, 30.0], 28.0, 4, _bumpy)
    d0, m0 = _prior(shape, 4)
    for t in (a, b):
        t.volume_create(origin, shape)
        t.volume_upload(d0, m0)
        t.volume_rebuild()
    a.volume_voxelize_mesh(pos, tri, materials=(np.arange(len(tri)) % 5 + 1).astype(np.uint32), solid=True)
    d, m = a.volume_download()
    b.volume_upload(d, m)
    for step in range(2):
        sa, sb = a.volume_rebuild(), b.volume_rebuild()
        assert (sa.n_voxels, sa.n_tree_nodes) == (sb.n_voxels, sb.n_tree_nodes)
        na, ma = a.download_tree()
        nb, mb = b.download_tree()
        assert np.array_equal(na, nb) and np.array_equal(ma, mb)
        for t in (a, b):
            t.volume_apply_brush((20.0, 30.0, 10.0), 9.0, 1.0, 0 if step == 0 else 1)
    a.shutdown()
    b.shutdown()


def test_runs_are_bit_identical():
    t = _tracer()
    pos, tri = M.icosphere([64.3, 63.7, 64.1], 50.0, 5, _bumpy)
    mats = (np.arange(len(tri)) * 31 % 200).astype(np.uint32)
    out = []
    for _ in range(2):
        t.volume_create((0, 0, 0), (128, 128, 128))
        t.volume_voxelize_mesh(pos, tri, materials=mats, solid=True)
        out.append(t.volume_download())
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)) and np.array_equal(out[0][1], out[1][1])
    t.shutdown()


def test_errors_write_nothing():
    t = _tracer()
    good = np.array([[1, 1, 1], [5, 1, 1], [1, 5, 2]], np.float32)
    tri = np.array([[0, 1, 2]], np.uint32)
    with pytest.raises(BlokError) as e:
        t.volume_voxelize_mesh(good, tri)
    assert e.value.status == BLOK_ERR_NO_WORLD
    t.volume_create((0, 0, 0), (16, 16, 16))
    d0, m0 = _prior((16, 16, 16), 9)
    t.volume_upload(d0, m0)
    bad = []
    for v in (np.nan, np.inf, -8388609.0):
        p = good.copy()
        p[2, 1] = v
        bad.append(dict(positions=p, triangles=tri))
    # every coordinate just beyond 2^23, a small extent: refused for the coordinate alone
    beyond = np.array([[8388610.0, 1, 1], [8388611.0, 1, 1], [8388612.0, 2, 1]], np.float32)
    bad += [dict(positions=beyond, triangles=tri), dict(positions=-beyond, triangles=tri)]
    bad.append(dict(positions=good, triangles=np.array([[0, 1, 3]], np.uint32)))
    bad.append(dict(positions=np.array([[0, 0, 0], [2049, 0, 0], [0, 1, 0]], np.float32), triangles=tri))
    bad.append(dict(positions=good, triangles=tri, density=0.0))
    bad.append(dict(positions=good, triangles=tri, density=float("nan")))
    for kw in bad:
        with pytest.raises(BlokError) as e:
            t.volume_voxelize_mesh(**kw)
        assert e.value.status == BLOK_ERR_INVALID_ARG
    rc = t._lib.blok_hip_volume_voxelize_mesh(t._ctx, None, 3, None, 1, None, 1, 1.0, 0, None)
    assert rc == BLOK_ERR_INVALID_ARG
    from blok_amd import _ffi
    rc = t._lib.blok_hip_volume_voxelize_mesh(t._ctx, _ffi.ptr(good), 3, _ffi.ptr(tri), 1, None, 1, 1.0, 2, None)
    assert rc == BLOK_ERR_INVALID_ARG
    d, m = t.volume_download()
    assert np.array_equal(d.view(np.uint32), d0.view(np.uint32)) and np.array_equal(m, m0)
    # an unreferenced non-finite vertex is not looked at
    assert t.volume_voxelize_mesh(np.concatenate([good, [[np.nan] * 3]]).astype(np.float32), tri) > 0
    t.shutdown()


def test_values_at_the_limits_are_accepted(shim):
    t = _tracer()
    at_limit = np.array([[8388608.0, 1, 1], [8388607.0, 2, 1], [8388608.0, 1, 2]], np.float32)      # |x| = 2^23: accepted, outside the box
    t.volume_create((0, 0, 0), (16, 16, 16))
    assert t.volume_voxelize_mesh(at_limit, np.array([[0, 1, 2]], np.uint32)) == 0
    assert t.volume_voxelize_mesh(-at_limit, np.array([[0, 1, 2]], np.uint32)) == 0
    # a snapped extent of exactly 2048 voxels: accepted and exact
    lim = np.array([[-1000.5, 3.5, 2.25], [1047.5, 9.0, 20.0], [3.0, 30.5, 4.0]], np.float32)
    _compare(shim, t, lim, np.array([[0, 1, 2]], np.uint32), (-20, 0, 0), (64, 40, 32), materials=np.array([7], np.uint32))
    t.shutdown()


def test_degenerate_triangles_across_the_box(shim):
    """Segments and points after snapping: voxelized as what they are, and enumerated by a plane through them (not their brick box)."""
    t = _tracer()
    pos = np.array([[0.5, 1.0, 1.5], [254.5, 253.0, 251.5], [127.5, 127.0, 126.5],           # collinear across the diagonal
                    [3.5, 200.25, 9.0], [3.5, 200.25, 9.0], [3.5, 200.25, 9.0],              # a point on a lattice plane
                    [10.0, 10.0, 200.0], [250.0, 10.0, 200.0], [10.0, 10.0, 200.0]],         # a repeated vertex along x
                   np.float32)
    tri = np.arange(9, dtype=np.uint32).reshape(-1, 3)
    d, _ = _compare(shim, t, pos, tri, (0, 0, 0), (256, 256, 256), prior=False)
    assert (d > 0).sum() > 256
    t.shutdown()


def _world_voxels(d, m, origin):
    z, y, x = np.nonzero(d > 0)
    return np.stack([x + origin[0], y + origin[1], z + origin[2]], 1).astype(np.int32), m[z, y, x]


def test_traced_frames_equal_the_oracle_world():
    """The primary frame after voxelize + rebuild equals the oracle's frame of the same voxels (OracleWorld.set_voxels / pack)."""
    from blok_amd import world as W
    from tests import oracle_ffi as O
    from tests.conftest import records_equal
    w, h = 160, 120
    t = _tracer()
    t.resize(w, h)
    origin, shape = (-8, 0, 4), (120, 90, 100)
    pos, tri = M.merge(M.icosphere([40.0, 40.0, 50.0], 30.0, 4, _bumpy), M.torus([70.0, 60.0, 60.0], 25.0, 6.0, 48, 16))
    mats = (np.arange(len(tri)) % 9 + 1).astype(np.uint32)
    t.volume_create(origin, shape)
    t.volume_voxelize_mesh(pos, tri, materials=mats, solid=True, material=4)
    t.volume_rebuild(W.scene_materials())
    d, m = t.volume_download()
    xyz, ids = _world_voxels(d, m, origin)
    ow = O.OracleWorld(128, 1.0)
    ow.set_voxels(xyz, ids)
    ow.rebuild()
    lat = O.Lattice(*ow.pack())
    for eye, at in [((140.0, 120.0, -40.0), (50.0, 45.0, 50.0)), ((-60.0, 30.0, 160.0), (60.0, 50.0, 40.0))]:
        cam = W.camera_look_at(eye, at, 60.0, w, h)
        got = t.draw_frame(cam).reshape(-1)
        ref, ctr = lat.trace(O.primary_rays(cam, w, h), threads=8)
        assert ctr["hits"] > 1000 and records_equal(got, ref).all()
    t.shutdown()


def test_path_traced_frames_with_and_without_the_sun_map_after_voxelizing():
    """The edited box and the fill bit the voxelizer commits (gpu_build.h: gpu_volume_commit) reach the shadow rays' last-occluder map: frames stay bit-identical."""
    from blok_amd import world as W
    w, h = 160, 120
    mats = W.scene_materials()
    t = _tracer()
    t.resize(w, h)
    t.volume_create((0, 0, 0), (64, 96, 64), 128, 1.0)
    ids = W.scene_dense(64)
    z, y, x = np.nonzero(ids)
    t.volume_set_voxels(np.stack([x, y, z], 1).astype(np.int32), ids[z, y, x], np.ones(len(x), dtype=np.float32))
    t.volume_rebuild(mats)
    cams = [W.scene_camera(64, 0, w, h), W.camera_look_at((5.0, 60.0, 5.0), (40.0, 30.0, 40.0), 70.0, w, h)]

    def same(tag):
        for cam in cams:
            t.set_sun_map(False)
            plain = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            t.set_sun_map(True)
            got = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            for k in plain:
                assert got[k].tobytes() == plain[k].tobytes(), (tag, k)

    same("scene")
    for k, (c, r, solid) in enumerate([((30.0, 70.0, 30.0), 12.0, True), ((15.0, 85.0, 45.0), 6.0, False), ((45.0, 60.0, 12.0), 8.0, True)]):
        pos, tri = M.icosphere(c, r, 3)                                        # floating above the terrain: new shadows
        assert t.volume_voxelize_mesh(pos, tri, material=5 + k, solid=solid) > 0
        t.volume_rebuild(mats)
        same(k)
    t.shutdown()


def test_headless_driver_renders_an_obj(tmp_path):
    import subprocess
    from blok_amd import build as b
    exe = b.build_tools()
    pos, tri = M.merge(M.icosphere([0.0, 0.0, 0.0], 1.0, 3), M.torus([0.0, 0.0, 0.0], 1.6, 0.3, 32, 12))
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 0.9 0.2 0.1\nnewmtl b\nKd 0.1 0.3 0.9\nPm 1\n")
    n_sphere = len(M.icosphere([0.0, 0.0, 0.0], 1.0, 3)[1])
    lines = ["mtllib m.mtl"] + [f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in pos.tolist()] + ["usemtl a"]
    lines += [f"f {a + 1} {b_ + 1} {c + 1}" + ("\nusemtl b" if i == n_sphere - 1 else "") for i, (a, b_, c) in enumerate(tri.tolist())]
    (tmp_path / "m.obj").write_text("\n".join(lines) + "\n")
    for extra in ([], ["--solid", "--rt", "--spp", "2"]):
        out = tmp_path / "frame.ppm"
        proc = subprocess.run([str(exe), "--obj", str(tmp_path / "m.obj"), "--obj-size", "96", "--size", "320x200", "--frames", "2",
                               "--out", str(out), *extra], capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr
        assert "voxels written" in proc.stdout and "frame 1:" in proc.stdout
        data = out.read_bytes()
        head = b"P6\n320 200\n255\n"
        assert data.startswith(head) and len(data) == len(head) + 320 * 200 * 3
        body = np.frombuffer(data[len(head):], np.uint8).reshape(-1, 3)
        colours, counts = np.unique(body, axis=0, return_counts=True)
        sky = colours[counts.argmax()]
        surface = body[(body != sky).any(axis=1)].astype(int)
        assert len(surface) > 0.05 * len(body)                                   # surface pixels, not a flat background
        assert (surface[:, 0] > surface[:, 2] + 30).any() and (surface[:, 2] > surface[:, 0] + 30).any()     # both MTL materials
