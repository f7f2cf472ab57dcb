"""CPU: Wavefront OBJ / MTL import (blok_amd/csrc/host/obj.cpp through blok_amd/mesh.py)."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd._ffi import BlokError
from blok_amd.mesh import ObjMesh, fit_to_box
from blok_amd.vox import MaterialLibrary
from tests import voxelize_meshes as M


def test_statement_forms_negative_indices_and_polygons():
    obj = ("# a comment\nmtllib none.mtl\no thing\ng group\ns 1\n"
           "v 0 0 0\nv 1 0 0 1.0\nv 1 1 0\nv 0 1 0\nv 0 0 1\n"
           "vt 0.5 0.5\nvn 0 0 1\nl 1 2\np 3\nfoo bar\n"
           "f 1 2 3\nf 1/1 3/1 4/1\nf 1//1 2//1 5//1\nf 2/1/1 3/1/1 5/1/1\n"
           "f -5 -4 -3 -2\n"                            # a quad, relative indices: 1 2 3 4
           "f 1 2 3 4 5")                               # a pentagon, no final newline
    m = ObjMesh.load_memory(obj)
    assert m.positions.dtype == np.float32 and m.positions.shape == (5, 3)
    assert m.triangles.dtype == np.uint32 and m.materials.dtype == np.uint32
    assert m.triangles.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    assert (m.materials == 0).all()


def test_crlf_is_accepted():
    a = ObjMesh.load_memory("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    b = ObjMesh.load_memory("v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 3\r\n")
    assert np.array_equal(a.positions, b.positions) and np.array_equal(a.triangles, b.triangles)


MTL = ("newmtl red\nKd 0.8 0.1 0.1\nPr 0.25\nPm 0.75\n"
       "newmtl lamp\nKd 1 1 1\nKe 2 1.5 0.5\n"
       "newmtl dark\nKd 0.1 0.1 0.1\nKe 0 0 0\n")
OBJ = ("mtllib scene.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\n"
       "f 1 2 3\nusemtl red\nf 1 2 4\nusemtl lamp\nf 1 3 4\nusemtl missing\nf 2 3 4\nusemtl dark\nf 1 2 3\n")


def test_mtl_fields_go_into_the_library():
    lib = MaterialLibrary()
    n0 = len(lib)
    m = ObjMesh.load_memory(OBJ, MTL, lib)
    assert len(lib) == n0 + 3
    red, lamp, dark = (lib.get_material_id_by_name(s) for s in ("red", "lamp", "dark"))
    assert m.materials.tolist() == [0, red, lamp, 0, dark]
    r = lib.get_material(red)[0]
    assert np.allclose(r["albedo"], [0.8, 0.1, 0.1]) and r["roughness"] == 0.25 and r["metallic"] == 0.75 and r["type"] == 0
    l_ = lib.get_material(lamp)[0]
    assert np.allclose(l_["emission"], [2, 1.5, 0.5]) and l_["type"] == 3 and l_["emission_power"] == 1.0
    d = lib.get_material(dark)[0]
    assert d["type"] == 0 and d["emission_power"] == 0.0
    assert (ObjMesh.load_memory(OBJ, MTL, None).materials == 0).all()         # no library: all zeros


def test_load_file_resolves_mtllib_next_to_the_obj(tmp_path):
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "scene.mtl").write_text(MTL)
    (tmp_path / "sub" / "model.obj").write_text(OBJ)
    lib = MaterialLibrary()
    m = ObjMesh.load_file(tmp_path / "sub" / "model.obj", lib)
    assert m.materials.tolist()[1] == lib.get_material_id_by_name("red") != 0
    (tmp_path / "sub" / "scene.mtl").unlink()
    with pytest.raises(BlokError, match="line 1") as e:
        ObjMesh.load_file(tmp_path / "sub" / "model.obj", lib)
    assert e.value.status == -1
    with pytest.raises(BlokError):
        ObjMesh.load_file(tmp_path / "nothing.obj")


@pytest.mark.parametrize("text,line", [
    ("v 0 0 0\nv 1 x 0\n", 2),                       # malformed number
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", 4),     # index 0
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4),     # beyond the vertices so far
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\n\nf 1 2 -4\n", 5),  # relative, before the first vertex
    ("v 0 0 0\nv 1 0 0\nf 1 2\n", 3),                # fewer than three vertices
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3a\n", 4),    # malformed index
    ("v 0 0\n", 1),                                  # a vertex needs three coordinates
])
def test_errors_name_the_line(text, line):
    with pytest.raises(BlokError, match=f"line {line}:"):
        ObjMesh.load_memory(text)


def test_mtl_errors_name_the_line():
    with pytest.raises(BlokError, match="mtl line 2:"):
        ObjMesh.load_memory(OBJ, "newmtl a\nKd 1 nope 1\n", MaterialLibrary())


def test_procedural_mesh_round_trips_through_obj(tmp_path):
    pos, tri = M.merge(M.icosphere([1.5, -2.25, 3.0], 4.0, 2), M.torus([0.0, 0.0, 0.0], 3.0, 1.0, 12, 6))
    lines = [f"v {x!r} {y!r} {z!r}" for x, y, z in pos.astype(float).tolist()]
    lines += [f"f {a + 1} {b + 1} {c + 1}" for a, b, c in tri.tolist()]
    path = tmp_path / "mesh.obj"
    path.write_text("\n".join(lines) + "\n")
    m = ObjMesh.load_file(path)
    assert np.array_equal(m.positions, pos) and np.array_equal(m.triangles, tri)


def test_fit_to_box():
    pos, _ = M.torus([10.0, -4.0, 7.0], 3.0, 1.0)
    out = fit_to_box(pos, (5, 5, 5), 64)
    assert out.dtype == np.float32
    assert out.min() >= 5.5 - 1e-4 and out.max() <= 5 + 64 - 0.5 + 1e-4
    ext = out.max(axis=0) - out.min(axis=0)
    assert abs(float(ext.max()) - 63.0) < 1e-3
    src = pos.max(axis=0) - pos.min(axis=0)
    assert np.allclose(ext / src, ext.max() / src.max(), rtol=1e-4)              # uniform scale
