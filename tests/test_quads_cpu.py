"""CPU: blok_quads_extract / blok_quads_write_obj (blok_amd/csrc/host/quads.cpp through blok_amd/mesh.py) against the independent numpy
reference (tests/quads_reference.py), the contract's quoted values, and laws computed from the records alone."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import mesh as M
from blok_amd._ffi import BlokError
from blok_amd.mesh import ObjMesh
from blok_amd.vox import MaterialLibrary
from tests import quads_reference as R
from tests import terrain_reference as TR
from tests.terrain_cases import ISSUE, prior

BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5


def _terrain(origin, n):
    lo = list(origin)
    d, m = TR.eval_box(dict(ISSUE), lo, [o + n for o in origin])
    return d, m


def _same(a, b):
    return np.ascontiguousarray(a, dtype=_ffi.QUAD).tobytes() == np.ascontiguousarray(b, dtype=_ffi.QUAD).tobytes()


@pytest.fixture(scope="module")
def terrain64():
    origin = (-32, -40, -32)
    d, m = _terrain(origin, 64)
    return origin, d, m


def test_record_layout():
    assert _ffi.QUAD.itemsize == 32 and R.DTYPE == _ffi.QUAD
    assert [_ffi.QUAD.fields[n][1] for n in ("lo", "du", "dv", "material", "face", "reserved")] == [0, 12, 16, 20, 24, 28]


def test_terrain_64_whole_box_quoted_values(terrain64):
    origin, d, m = terrain64
    assert int((d > 0).sum()) == 165076
    q = M.extract_quads_host(d, m, origin)
    assert M.extract_quads_host.totals == (12996, 39470)
    assert len(q) == 12996
    assert R.digest(q) == "fdddf8120b52c66e84052421a598766fc813c5c34ec43a6baaf51ded943830e1"
    assert np.bincount(q["face"], minlength=6).tolist() == [2108, 2258, 2618, 1713, 2181, 2118]
    first, last = q[0], q[-1]
    assert (int(first["face"]), first["lo"].tolist(), int(first["du"]), int(first["dv"]), int(first["material"])) == (0, [-31, -5, -28], 1, 1, 2)
    assert (int(last["face"]), last["lo"].tolist(), int(last["du"]), int(last["dv"]), int(last["material"])) == (5, [-20, 6, 31], 2, 1, 1)
    # the two identities: area = faces, signed volume = filled (the mesh of a whole box is closed)
    assert int((q["du"].astype(np.int64) * q["dv"]).sum()) == 39470
    assert R.signed_volume6(q) == 6 * 165076
    ref, ref_faces = R.extract(d, m, origin)
    assert ref_faces == 39470 and _same(q, ref)


def test_terrain_64_ignore_material_and_region(terrain64):
    origin, d, m = terrain64
    q = M.extract_quads_host(d, m, origin, ignore_material=True)
    assert M.extract_quads_host.totals == (12121, 39470)
    assert R.digest(q) == "b619be665b55e40455739ce650f7b6612e390602d0148577b002dd1230071b37"
    assert (q["material"] == 0).all()
    q = M.extract_quads_host(d, m, origin, (-20, -30, -20), (20, 20, 20))
    assert M.extract_quads_host.totals == (5237, 10932)
    assert R.digest(q) == "d88722b158d3ea724d75a567185c1dfbb944f7eee65d3725dc2c1763dfd1dcde"


def test_terrain_96_counts():
    origin = (-48, -56, -48)
    d, m = _terrain(origin, 96)
    assert int((d > 0).sum()) == 481231
    assert M.extract_quads_host(d, m, origin, count_only=True) == (31063, 94738)
    assert M.extract_quads_host(d, m, origin, ignore_material=True, count_only=True) == (29312, 94738)
    q = M.extract_quads_host(d, m, origin)
    assert R.signed_volume6(q) == 6 * 481231


def test_prior_content_with_negative_densities():
    d, m = prior((20, 24, 28))
    d[::3, ::2, ::5] = -0.5
    origin = (-7, 3, -11)
    assert int((d > 0).sum()) == 1386
    q = M.extract_quads_host(d, m, origin)
    assert M.extract_quads_host.totals == (7145, 7488)
    assert R.digest(q) == "ba99a3c9ea5a72fba69178b91835d543da6a78b64b2481d976137ccbeae7f439"


def _tuples(q):
    return [(int(r["face"]), tuple(r["lo"].tolist()), int(r["du"]), int(r["dv"])) for r in q]


def test_slab_full_box_and_checkerboard():
    d = np.zeros((8, 8, 8), np.float32)
    d[:, 2:4, :] = 1.0
    m = np.ones((8, 8, 8), np.uint32)
    q = M.extract_quads_host(d, m)
    assert M.extract_quads_host.totals == (6, 192)
    assert _tuples(q) == [(0, (8, 2, 0), 2, 8), (1, (0, 2, 0), 2, 8), (2, (0, 4, 0), 8, 8), (3, (0, 2, 0), 8, 8), (4, (0, 2, 8), 8, 2), (5, (0, 2, 0), 8, 2)]
    m2 = m.copy()
    m2[:, :, 4:] = 2
    assert M.extract_quads_host(d, m2, count_only=True) == (10, 192)
    assert M.extract_quads_host(d, m2, ignore_material=True, count_only=True) == (6, 192)
    full = np.ones((8, 8, 8), np.float32)
    q = M.extract_quads_host(full, m)
    assert M.extract_quads_host.totals == (6, 384) and (q["du"] == 8).all() and (q["dv"] == 8).all()
    z, y, x = np.indices((8, 8, 8))
    checker = ((x + y + z) % 2 == 0).astype(np.float32)
    assert M.extract_quads_host(checker, m, count_only=True) == (1536, 1536)      # the worst case: 3 per cell


def _random_volume(rng, shape_zyx, fill):
    d = np.where(rng.random(shape_zyx) < fill, rng.uniform(0.1, 2.0, shape_zyx), 0.0).astype(np.float32)
    d[rng.random(shape_zyx) < 0.05] = -1.0
    d[rng.random(shape_zyx) < 0.05] = np.nan
    d[rng.random(shape_zyx) < 0.05] = -0.0
    # few materials in blobs, so that runs and stacks both merge and break on the key
    m = (rng.integers(1, 4, shape_zyx) if fill < 0.5 else np.broadcast_to(rng.integers(1, 3, (shape_zyx[0], 1, shape_zyx[2])), shape_zyx)).astype(np.uint32)
    return d, np.ascontiguousarray(m)


@pytest.mark.parametrize("seed", range(6))
def test_seeded_random_volumes_equal_the_reference(seed):
    rng = np.random.default_rng(100 + seed)
    shape = tuple(int(v) for v in rng.integers(3, 23, 3))      # [z][y][x], ragged
    if seed == 0:
        shape = (5, 7, 70)                                       # a row longer than one 64-bit word
    origin = tuple(int(v) for v in rng.integers(-40, 10, 3))
    d, m = _random_volume(rng, shape, (0.15, 0.5, 0.85)[seed % 3])
    dims = shape[::-1]
    regions = [(None, None)]
    for k in range(4):
        a = [int(rng.integers(0, dims[c])) for c in range(3)]
        b = [int(rng.integers(a[c] + 1, dims[c] + 1)) for c in range(3)]
        if k == 3:
            b[k % 3] = a[k % 3] + 1                             # one voxel thick
        regions.append((tuple(origin[c] + a[c] for c in range(3)), tuple(origin[c] + b[c] for c in range(3))))
    for lo, hi in regions:
        for ignore in (False, True):
            ref, ref_faces = R.extract(d, m, origin, lo, hi, ignore)
            q = M.extract_quads_host(d, m, origin, lo, hi, ignore)
            assert M.extract_quads_host.totals == (len(ref), ref_faces), (lo, hi, ignore)
            assert _same(q, ref), (lo, hi, ignore)


def _exposed_unit_faces(d, m, ignore=False):
    return np.stack([R.exposure(d, f) for f in range(6)])


def test_laws_from_the_records_alone():
    rng = np.random.default_rng(7)
    shape, origin = (13, 17, 21), (-5, 4, -9)
    d, m = _random_volume(rng, shape, 0.6)
    q = M.extract_quads_host(d, m, origin)
    assert (q["reserved"] == 0).all() and (q["du"] >= 1).all() and (q["dv"] >= 1).all() and (q["face"] <= 5).all()
    keys = [R.canonical_key(r) for r in q]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)                 # the order is total
    cover, key = R.rasterise(q, shape, origin)
    exposed = _exposed_unit_faces(d, m)
    assert np.array_equal(cover, exposed.astype(np.int32))                       # every exposed unit face exactly once, nothing else
    assert np.array_equal(key[exposed], np.broadcast_to(m, exposed.shape)[exposed])
    assert R.signed_volume6(q) == 6 * int(R.filled(d).sum())
    # regions that tile the box give the unit faces of the whole box
    hi = tuple(o + s for o, s in zip(origin, shape[::-1]))
    cut = (origin[0] + 9, origin[1] + 5, origin[2] + 6)
    total = np.zeros_like(cover)
    n_faces = 0
    for ix in range(2):
        for iy in range(2):
            for iz in range(2):
                lo = tuple((origin, cut)[i][c] for c, i in enumerate((ix, iy, iz)))
                h = tuple((cut, hi)[i][c] for c, i in enumerate((ix, iy, iz)))
                part = M.extract_quads_host(d, m, origin, lo, h)
                n_faces += M.extract_quads_host.totals[1]
                total += R.rasterise(part, shape, origin)[0]
    assert np.array_equal(total, cover) and n_faces == int(exposed.sum())


def test_capacity_gives_a_prefix_and_the_totals(terrain64):
    origin, d, m = terrain64
    whole = M.extract_quads_host(d, m, origin)
    part = M.extract_quads_host(d, m, origin, capacity=1000)
    assert M.extract_quads_host.totals == (12996, 39470)
    assert len(part) == 1000 and _same(part, whole[:1000])


def _raw(d, m, origin, dims, lo, hi, flags, out=None, capacity=0):
    lib = _ffi.host_lib()
    arr = lambda v: None if v is None else (C.c_int32 * 3)(*v)
    nq, nf = C.c_uint64(99), C.c_uint64(99)
    rc = lib.blok_quads_extract(None if d is None else _ffi.ptr(d), None if m is None else _ffi.ptr(m), arr(origin), dims[0], dims[1], dims[2],
                                arr(lo), arr(hi), flags, None if out is None else _ffi.ptr(out), capacity, C.byref(nq), C.byref(nf))
    return rc, int(nq.value), int(nf.value)


def test_error_table():
    d = np.ones((4, 5, 6), np.float32)
    m = np.ones((4, 5, 6), np.uint32)
    dims, origin = (6, 5, 4), (10, 20, 30)
    assert _raw(d, m, origin, dims, None, None, 0) == (0, 6, 2 * (30 + 24 + 20))
    assert _raw(d, m, origin, dims, None, None, 4)[0] == BLOK_ERR_INVALID_ARG                       # unknown flag bits
    assert _raw(d, m, origin, dims, (10, 20, 30), None, 0)[0] == BLOK_ERR_INVALID_ARG                # exactly one region pointer
    assert _raw(d, m, origin, dims, None, (16, 25, 34), 0)[0] == BLOK_ERR_INVALID_ARG
    assert _raw(d, m, origin, dims, (12, 20, 30), (11, 25, 34), 0)[0] == BLOK_ERR_INVALID_ARG        # lo > hi
    assert _raw(d, m, origin, dims, (9, 20, 30), (16, 25, 34), 0)[0] == BLOK_ERR_UNSUPPORTED         # leaves the box
    assert _raw(d, m, origin, dims, (10, 20, 30), (16, 25, 35), 0)[0] == BLOK_ERR_UNSUPPORTED
    assert _raw(d, m, origin, dims, (12, 22, 31), (12, 25, 34), 0) == (0, 0, 0)                      # an empty region
    assert _raw(None, None, origin, (2048, 2048, 2048), None, None, 0)[0] == BLOK_ERR_UNSUPPORTED    # above 2^32 cells
    assert _raw(None, m, origin, dims, None, None, 0)[0] == BLOK_ERR_INVALID_ARG
    assert _raw(d, m, origin, dims, None, None, 0, None, 5)[0] == BLOK_ERR_INVALID_ARG               # a capacity without an array
    assert _raw(d, m, None, dims, (0, 0, 0), (6, 5, 4), 0) == (0, 6, 148)                            # origin NULL = (0, 0, 0)
    for rc_case in (_raw(d, m, origin, dims, None, None, 4), _raw(d, m, origin, dims, (9, 20, 30), (16, 25, 34), 0)):
        assert rc_case[1:] == (0, 0)


def _library():
    lib = MaterialLibrary()
    ids = []
    for k, rgb in enumerate([(0.8, 0.1, 0.1), (0.1, 0.7, 0.2), (0.25, 0.25, 0.9)]):
        desc = MaterialLibrary.new_desc()
        desc["albedo"] = rgb
        desc["name"] = f"user{k}".encode()
        ids.append(lib.add_material(desc))
    return lib, ids


def test_obj_round_trip(tmp_path):
    lib, ids = _library()
    rng = np.random.default_rng(11)
    shape, origin = (9, 8, 10), (-4, 2, -3)
    d, m = _random_volume(rng, shape, 0.6)
    m = np.asarray(ids, dtype=np.uint32)[m % 3]
    q = M.extract_quads_host(d, m, origin)
    path = tmp_path / "surface.obj"
    M.write_obj(path, q, lib)
    assert (tmp_path / "surface.mtl").exists()
    back_lib = MaterialLibrary()
    mesh = ObjMesh.load_file(path, back_lib)
    assert len(mesh.triangles) == 2 * len(q)
    pos = mesh.positions[mesh.triangles.reshape(-1)].reshape(-1, 2, 3, 3)         # [quad][triangle][corner][xyz]
    pos_ref, tri_ref, mat_ref = M.quads_to_triangles(q)
    assert np.array_equal(pos, pos_ref[tri_ref.reshape(-1)].reshape(-1, 2, 3, 3))   # the same corner positions, (c0 c1 c2), (c0 c2 c3)
    assert np.array_equal(np.stack([R.corners(r) for r in q]).astype(np.float32).reshape(-1, 3), pos_ref)
    # outward winding: the triangle normal points along the face normal
    normal = np.cross(pos[:, :, 1] - pos[:, :, 0], pos[:, :, 2] - pos[:, :, 0])
    n_f = np.zeros((len(q), 3))
    n_f[np.arange(len(q)), np.array(R.NORMAL_AXIS)[q["face"]]] = np.where(q["face"] % 2 == 0, 1.0, -1.0)
    assert ((normal * n_f[:, None, :]).sum(axis=2) > 0).all()
    # each triangle's material has the albedo of the quad's material
    for k in range(0, len(q), 7):
        want = lib.get_material(int(q["material"][k]))["albedo"]
        for t in (2 * k, 2 * k + 1):
            assert np.array_equal(back_lib.get_material(int(mesh.materials[t]))["albedo"], want)
    # vertices are shared and numbered by first use
    corners = pos_ref.reshape(-1, 3)
    seen = {}
    for c in map(tuple, corners.tolist()):
        seen.setdefault(c, len(seen))
    assert len(mesh.positions) == len(seen)
    assert [tuple(p) for p in mesh.positions.tolist()] == list(seen.keys())
    text = path.read_text().splitlines()
    assert text[0] == "mtllib surface.mtl"
    assert sum(line.startswith("f ") for line in text) == len(q) and all(len(line.split()) == 5 for line in text if line.startswith("f "))
    changes = 1 + int(np.count_nonzero(np.diff(q["material"].astype(np.int64))))
    assert sum(line.startswith("usemtl m") for line in text) == changes
    assert all(float(v) == int(float(v)) and "." not in v for line in text if line.startswith("v ") for v in line.split()[1:])


def test_obj_of_the_slab_shares_its_eight_vertices(tmp_path):
    d = np.zeros((8, 8, 8), np.float32)
    d[:, 2:4, :] = 1.0
    q = M.extract_quads_host(d, np.ones((8, 8, 8), np.uint32))
    M.write_obj(tmp_path / "slab.obj", q)                                        # no library: no mtllib, no .mtl
    assert not (tmp_path / "slab.mtl").exists()
    mesh = ObjMesh.load_file(tmp_path / "slab.obj")
    assert len(mesh.positions) == 8 and len(mesh.triangles) == 12 and (mesh.materials == 0).all()
    assert "mtllib" not in (tmp_path / "slab.obj").read_text()


def test_write_obj_refuses_what_is_no_quad(tmp_path):
    q = np.zeros(1, dtype=_ffi.QUAD)
    q["du"], q["dv"], q["face"] = 1, 1, 6
    with pytest.raises(BlokError):
        M.write_obj(tmp_path / "bad.obj", q)
    q["face"], q["dv"] = 0, 0
    with pytest.raises(BlokError):
        M.write_obj(tmp_path / "bad.obj", q)
    with pytest.raises(BlokError):
        M.write_obj(tmp_path / "no_such_dir" / "x.obj", np.zeros(0, dtype=_ffi.QUAD))
