"""CPU: the voxelizer's exact tests (blok_amd/csrc/hip/voxelize_core.h, compiled for the host through
tests/host_harness/voxelize_shim.cpp) against the independent reference (tests/voxelize_reference.py) and analytic expectations."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from collections import deque
from pathlib import Path

import numpy as np
import pytest

from tests import voxelize_meshes as M
from tests import voxelize_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("voxelize_shim") / "libvoxelize_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'blok_amd/csrc/hip'}", "-shared", "-o", os.fspath(out), os.fspath(SRC / "voxelize_shim.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    L.vs_voxelize.restype = C.c_int
    L.vs_voxelize.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                              C.c_size_t, C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.POINTER(C.c_uint64)]
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def shim_voxelize(shim, positions, triangles, origin, shape, materials=None, material=1, density=1.0, solid=False, dens=None, ids=None):
    nx, ny, nz = shape
    d = np.zeros((nz, ny, nx), np.float32) if dens is None else dens.copy()
    m = np.zeros((nz, ny, nx), np.uint32) if ids is None else ids.copy()
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    mats = None if materials is None else np.ascontiguousarray(materials, dtype=np.uint32)
    o = np.ascontiguousarray(origin, dtype=np.int32)
    n = C.c_uint64(0)
    rc = shim.vs_voxelize(_p(o), nx, ny, nz, _p(d), _p(m), _p(pos), len(pos), _p(tri), len(tri), _p(mats), material, density, 1 if solid else 0,
                          C.byref(n))
    return rc, d, m, int(n.value)


def random_triangles(seed=7, n=2000, box=48):
    rng = np.random.default_rng(seed)
    tris = []
    for i in range(n):
        size = float(np.exp(rng.uniform(np.log(0.01), np.log(40.0))))
        c = rng.uniform(-4, box + 4, 3)
        kind = i % 6
        if kind == 0:                                  # vertices on lattice points
            p = np.round(c + rng.uniform(-size, size, (3, 3)))
        elif kind == 1:                                # on half-voxels
            p = np.round((c + rng.uniform(-size, size, (3, 3))) * 2) / 2
        elif kind == 2:                                # collinear
            a, b = c, c + rng.uniform(-size, size, 3)
            p = np.array([a, b, a + (b - a) * rng.uniform(-1, 2)])
        elif kind == 3:                                # repeated vertex / all equal
            a = c + rng.uniform(-size, size, 3)
            p = np.array([c, a, a]) if i % 12 == 3 else np.array([c, c, c])
        else:                                          # off-lattice
            p = c + rng.uniform(-size, size, (3, 3))
        tris.append(p)
    tris.append(np.array([[1.0, 1.0, 1.0], [2049.0, 3.0, 2.0], [5.0, 2049.0, 4.0]]))      # extent exactly 2048 voxels: accepted
    pos = np.array(tris, dtype=np.float32).reshape(-1, 3)
    return pos, np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)


def test_random_triangles_surface_and_materials_match_the_reference(shim):
    pos, tri = random_triangles()
    origin, shape = (0, 0, 0), (48, 48, 48)
    mats = (np.arange(len(tri), dtype=np.uint32) * 7919 % 251 + 1).astype(np.uint32)
    rc, d, m, n = shim_voxelize(shim, pos, tri, origin, shape, materials=mats)
    assert rc == 0
    filled, ids = R.voxelize(pos, tri, origin, shape, materials=mats)
    assert np.array_equal(d > 0, filled)
    assert np.array_equal(m, ids)
    assert n == int(filled.sum())


def closed_meshes():
    return {
        "box": (M.box([2.3, 3.1, 4.7], [17.6, 15.2, 19.9]), (0, 0, 0), (24, 24, 24)),
        "icosphere": (M.icosphere([11.7, 12.2, 11.4], 8.3, 2), (0, 0, 0), (24, 24, 24)),
        "torus": (M.torus([12.0, 12.0, 12.0], 7.0, 3.0), (0, 0, 0), (24, 24, 24)),
        "nested": (M.merge(M.icosphere([12.0, 12.0, 12.0], 9.5, 2), M.icosphere([12.0, 12.0, 12.0], 5.5, 1)), (0, 0, 0), (24, 24, 24)),
        "octahedron_on_centres": (M.octahedron([10.5, 10.5, 10.5], 6.0), (0, 0, 0), (22, 22, 22)),
        "sphere_half_outside": (M.icosphere([3.0, 12.0, 12.0], 8.0, 2), (0, 0, 0), (20, 24, 24)),
    }


@pytest.mark.parametrize("name", list(closed_meshes()))
def test_solid_closed_meshes_match_the_reference(shim, name):
    (pos, tri), origin, shape = closed_meshes()[name]
    rc, d, m, n = shim_voxelize(shim, pos, tri, origin, shape, material=5, solid=True)
    assert rc == 0
    filled, ids = R.voxelize(pos, tri, origin, shape, material=5, solid=True)
    assert np.array_equal(d > 0, filled)
    assert np.array_equal(m, ids)
    surface, _ = R.voxelize(pos, tri, origin, shape, material=5)
    assert filled.sum() > surface.sum()                    # something interior


def test_nested_spheres_fill_only_the_shell(shim):
    (pos, tri), origin, shape = closed_meshes()["nested"]
    _, d, _, _ = shim_voxelize(shim, pos, tri, origin, shape, solid=True)
    assert d[12, 12, 12] == 0                              # the centre lies inside both spheres: even parity
    assert d[12, 12, 12 + 7] > 0                           # between the spheres


def test_box_gives_the_cube_and_its_shell(shim):
    pos, tri = M.box([0.25] * 3, [9.75] * 3)
    shape = (12, 12, 12)
    _, d, _, n = shim_voxelize(shim, pos, tri, (0, 0, 0), shape, solid=True)
    cube = np.zeros((12, 12, 12), bool)
    cube[:10, :10, :10] = True
    assert np.array_equal(d > 0, cube) and n == 1000
    _, d, _, n = shim_voxelize(shim, pos, tri, (0, 0, 0), shape)
    shell = cube.copy()
    shell[1:9, 1:9, 1:9] = False
    assert np.array_equal(d > 0, shell) and n == 1000 - 512


def test_sphere_interior_and_bounds(shim):
    c, r = np.array([16.3, 15.8, 16.1]), 11.0
    pos, tri = M.icosphere(c, r, 3)
    _, d, _, _ = shim_voxelize(shim, pos, tri, (0, 0, 0), (32, 32, 32), solid=True)
    z, y, x = np.meshgrid(*[np.arange(32) + 0.5] * 3, indexing="ij")
    dist = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    assert (d[dist < r - 1] > 0).all()
    assert not (d[dist > r + 1] > 0).any()


def _outside_reachable(written):
    """Unwritten voxels 6-connected to the box's border."""
    nz, ny, nx = written.shape
    seen = np.zeros_like(written)
    q = deque()
    for idx in zip(*np.nonzero(~written)):
        z, y, x = idx
        if z in (0, nz - 1) or y in (0, ny - 1) or x in (0, nx - 1):
            seen[idx] = True
            q.append(idx)
    while q:
        z, y, x = q.popleft()
        for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            a = (z + dz, y + dy, x + dx)
            if 0 <= a[0] < nz and 0 <= a[1] < ny and 0 <= a[2] < nx and not written[a] and not seen[a]:
                seen[a] = True
                q.append(a)
    return seen


@pytest.mark.parametrize("name", ["box", "icosphere", "torus", "nested", "octahedron_on_centres"])
def test_surfaces_are_watertight(shim, name):
    (pos, tri), origin, shape = closed_meshes()[name]
    _, d, _, _ = shim_voxelize(shim, pos, tri, origin, shape)
    _, solid, _, _ = shim_voxelize(shim, pos, tri, origin, shape, solid=True)
    inside = (solid > 0) & ~(d > 0)                        # centres with odd parity that are not on the surface
    reach = _outside_reachable(d > 0)
    assert not (reach & inside).any()


def test_order_and_winding_do_not_change_the_sets(shim):
    (pos, tri), origin, shape = closed_meshes()["torus"]
    rng = np.random.default_rng(3)
    base = [shim_voxelize(shim, pos, tri, origin, shape, solid=s)[1] for s in (False, True)]
    for t2 in (tri[rng.permutation(len(tri))], np.roll(tri, 1, axis=1), tri[:, ::-1].copy()):
        for s, ref in zip((False, True), base):
            assert np.array_equal(shim_voxelize(shim, pos, np.ascontiguousarray(t2), origin, shape, solid=s)[1], ref)


def test_refusals_and_limits(shim):
    shape, o = (8, 8, 8), (0, 0, 0)
    good = np.array([[1, 1, 1], [3, 1, 1], [1, 3, 1]], np.float32)
    t = np.array([[0, 1, 2]], np.uint32)
    for bad in (np.nan, np.inf, 8388608.5):
        p = good.copy()
        p[1, 0] = bad
        assert shim_voxelize(shim, p, t, o, shape)[0] == -1
    # all three coordinates just beyond 2^23 with a small extent: refused for the coordinate alone
    beyond = np.array([[8388610.0, 1, 1], [8388611.0, 1, 1], [8388612.0, 2, 1]], np.float32)
    assert shim_voxelize(shim, beyond, t, o, shape)[0] == -1
    assert shim_voxelize(shim, -beyond, t, o, shape)[0] == -1
    assert shim_voxelize(shim, good, np.array([[0, 1, 3]], np.uint32), o, shape)[0] == -1
    assert shim_voxelize(shim, np.array([[1, 1, 1], [2050, 1, 1], [1, 2, 1]], np.float32), t, o, shape)[0] == -1
    for dens in (0.0, -1.0, np.nan, np.inf):
        assert shim_voxelize(shim, good, t, o, shape, density=dens)[0] == -1
    # unreferenced vertices are not checked; values at the limits are accepted
    p = np.concatenate([good, [[np.nan, 0, 0]]]).astype(np.float32)
    assert shim_voxelize(shim, p, t, o, shape)[0] == 0
    far = np.array([[8388608.0, 1, 1], [8388608.0, 2, 1], [8388608.0, 1, 2]], np.float32)
    rc, d, _, n = shim_voxelize(shim, far, t, o, shape)
    assert rc == 0 and n == 0
    lim = np.array([[0.5, 0.5, 0.5], [2048.5, 0.5, 0.5], [0.5, 2.5, 0.5]], np.float32)
    rc, d, _, n = shim_voxelize(shim, lim, t, o, shape)
    assert rc == 0
    filled, _ = R.voxelize(lim, t, o, shape)
    assert np.array_equal(d > 0, filled) and n == int(filled.sum())


def test_snapping_rounds_half_to_even(shim):
    # 1/512 is exactly half a snapping step: 0.5 * 1/256 rounds to 0, 1.5 * 1/256 to 2/256
    assert R.snap([1 / 512, 3 / 512, -1 / 512]).tolist() == [0, 2, 0]
    # a triangle in the plane x = 4 + 1/512 snaps onto the lattice plane x = 4 and marks both layers
    p = np.array([[4 + 1 / 512, 1.5, 1.5], [4 + 1 / 512, 2.5, 1.5], [4 + 1 / 512, 1.5, 2.5]], np.float32)
    _, d, _, _ = shim_voxelize(shim, p, np.array([[0, 1, 2]], np.uint32), (0, 0, 0), (8, 8, 8))
    assert d[1, 1, 3] > 0 and d[1, 1, 4] > 0
