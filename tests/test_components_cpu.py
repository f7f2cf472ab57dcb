"""CPU: the numpy reference of the connected-components contract (tests/components_reference.py) against hand-written cases whose labels
are spelled out here, and blok_components_label (blok_amd/csrc/host/components.cpp through blok_amd/components.py) against the reference
byte for byte, on the cases the GPU tests use and on the error and capacity table.  Where scipy imports, component count and sizes are
checked against scipy.ndimage.label as well."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd.components import label_components_host
from tests import components_reference as R

E = R.EMPTY
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5


def grid(shape_xyz, voxels, value=1.0):
    nx, ny, nz = shape_xyz
    d = np.zeros((nz, ny, nx), dtype=np.float32)
    for x, y, z in voxels:
        d[z, y, x] = value
    return d


def both(d, origin=(0, 0, 0), lo=None, hi=None):
    """The reference's result, after the host build has given the same bytes."""
    labels, records = R.label(d, origin, lo, hi)
    got_labels, got_records = label_components_host(d, origin, lo, hi)
    assert got_labels.tobytes() == labels.tobytes()
    assert got_records.tobytes() == records.tobytes()
    assert label_components_host.totals == (len(records), int(records["n_voxels"].sum()))
    return labels, records


def record(rec):
    return (int(rec["label"]), int(rec["touches"]), int(rec["n_voxels"]), tuple(rec["lo"].tolist()), tuple(rec["hi"].tolist()))


# ---- hand-written cases -------------------------------------------------------------------------------------------------------------

def test_face_edge_and_corner_contacts():
    # a 4 x 3 x 2 box: index = x + 4 y + 12 z
    labels, records = both(grid((4, 3, 2), [(1, 1, 0), (2, 1, 0)]))                  # a shared face
    assert labels.tolist() == [E, E, E, E, E, 5, 5, E, E, E, E, E] + [E] * 12
    assert [record(r) for r in records] == [(5, 32, 2, (1, 1, 0), (3, 2, 1))]                           # in the -Z layer only (bit 5)
    labels, records = both(grid((4, 3, 2), [(1, 1, 0), (2, 2, 0)]))                  # a shared edge: two components
    assert labels.tolist() == [E, E, E, E, E, 5, E, E, E, E, 10, E] + [E] * 12
    assert [record(r)[:3] for r in records] == [(5, 32, 1), (10, 32 | 4, 1)]         # the second also lies in the +Y layer (bit 2)
    labels, records = both(grid((4, 3, 2), [(1, 1, 0), (2, 2, 1)]))                  # a shared corner: two components
    assert labels.tolist() == [E, E, E, E, E, 5, E, E, E, E, E, E] + [E] * 10 + [22, E]
    assert [record(r) for r in records] == [(5, 32, 1, (1, 1, 0), (2, 2, 1)), (22, 16 | 4, 1, (2, 2, 1), (3, 3, 2))]


def test_an_l_and_a_ring():
    # 5 x 5 x 1, index = x + 5 y.  An L: down a column, then along a row
    labels, records = both(grid((5, 5, 1), [(1, 0, 0), (1, 1, 0), (1, 2, 0), (2, 2, 0), (3, 2, 0)]))
    want = [E] * 25
    for i in (1, 6, 11, 12, 13):
        want[i] = 1
    assert labels.tolist() == want
    assert [record(r) for r in records] == [(1, 8 | 16 | 32, 5, (1, 0, 0), (4, 3, 1))]     # -Y layer, and both z layers of a one-thick region
    # a ring around (2, 2) with a separate voxel in its hole: the ring is one component although its two arms meet far from its minimum
    ring = [(x, y, 0) for x in (1, 2, 3) for y in (1, 2, 3) if (x, y) != (2, 2)]
    labels, records = both(grid((5, 5, 3), shifted_z(ring, 1) + [(2, 2, 0)]))
    assert [record(r)[:3] for r in records] == [(12, 32, 1), (31, 0, 8)]
    assert sorted(np.nonzero(labels == 31)[0].tolist()) == [31, 32, 33, 36, 38, 41, 42, 43]


def shifted_z(voxels, dz):
    return [(x, y, z + dz) for x, y, z in voxels]


def test_a_region_cuts_a_bar_in_two_and_voxels_outside_join_nothing():
    # a bar along x at y = 1 bending out of the region through y = 0 and back: inside the region y in [1, 3) it is two pieces
    bar = [(0, 1, 0), (1, 1, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (3, 1, 0), (4, 1, 0)]
    d = grid((5, 3, 1), bar)
    labels, records = both(d)
    assert len(records) == 1 and int(records[0]["n_voxels"]) == 7
    labels, records = both(d, (0, 0, 0), (0, 1, 0), (5, 3, 1))        # rows y = 1, 2: index = x + 5 (y - 1)
    assert labels.tolist() == [0, 0, E, 3, 3] + [E] * 5
    assert [record(r) for r in records] == [(0, 2 | 8 | 16 | 32, 2, (0, 1, 0), (2, 2, 1)), (3, 1 | 8 | 16 | 32, 2, (3, 1, 0), (5, 2, 1))]


def test_nan_negative_and_zero_densities_are_empty_and_material_ids_do_not_matter():
    d = np.zeros((1, 1, 6), dtype=np.float32)
    d[0, 0] = [1.0, np.nan, 0.5, -2.0, 1e-30, -0.0]
    labels, records = both(d)
    assert labels.tolist() == [0, E, 2, E, 4, E]
    assert records["n_voxels"].tolist() == [1, 1, 1]
    # (the labelling takes no material ids at all: a filled voxel with id 0 is a filled voxel; the capture's ids are the GPU tests')


def test_touches_on_each_side_and_bounds_at_a_negative_origin():
    origin, shape = (-7, -3, -9), (5, 5, 6)
    for face, voxel in enumerate(((4, 2, 2), (0, 2, 2), (2, 4, 2), (2, 0, 2), (2, 2, 5), (2, 2, 0))):
        labels, records = both(grid(shape, [voxel, (2, 2, 2)]), origin)
        assert len(records) == 2
        rec = records[records["label"] == voxel[0] + 5 * voxel[1] + 25 * voxel[2]][0]
        assert int(rec["touches"]) == 1 << face, (face, int(rec["touches"]))
        assert tuple(rec["lo"]) == tuple(origin[a] + voxel[a] for a in range(3)) and tuple(rec["hi"]) == tuple(origin[a] + voxel[a] + 1 for a in range(3))
        inner = records[records["label"] == 2 + 10 + 50][0]
        assert int(inner["touches"]) == 0 and tuple(inner["lo"]) == (-5, -1, -7)
    # a region inside the box: touches speaks of the REGION's sides, bounds of the world
    labels, records = both(grid(shape, [(1, 1, 2), (3, 2, 4)]), origin, (-6, -2, -7), (-3, 0, -4))
    assert [record(r) for r in records] == [(0, 2 | 8 | 32, 1, (-6, -2, -7), (-5, -1, -6)), (2 + 3 * 1 + 6 * 2, 1 | 4 | 16, 1, (-4, -1, -5), (-3, 0, -4))]


# ---- the host build on the GPU tests' cases -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.cases()))
def test_host_build_equals_the_reference(name):
    d, _, lo, hi = R.cases()[name]
    labels, records = R.expected(name)
    got_labels, got_records = label_components_host(d, R.ORIGIN, lo, hi)
    assert got_labels.tobytes() == labels.tobytes(), int((got_labels != labels).sum())
    assert got_records.tobytes() == records.tobytes()
    assert label_components_host.totals == (len(records), int(records["n_voxels"].sum()))


def test_the_cases_are_what_they_claim():
    """From the reference alone: the shapes keep the properties that make them hard."""
    for voxels, n in R.border_cases():
        labels = R.expected("brick borders")[0].reshape(R.SHAPE[::-1])
        assert len({int(labels[z, y, x]) for x, y, z in voxels}) == n, voxels
    for name in ("path from one end", "path from the middle"):
        labels, records = R.expected(name)
        assert len(records) == 1 and int(records[0]["n_voxels"]) == 5903 == int((labels != E).sum()) and int(records[0]["label"]) == 0
    assert R.boustrophedon(R.PATH_EXT)[0] == (0, 0, 0) and 2000 < R.boustrophedon_from_the_middle(R.PATH_EXT).index((0, 0, 0)) < 4000
    assert arms("combs") >= 8
    assert len(R.expected("checkerboard")[1]) == 16384
    assert R.expected("solid box")[1]["n_voxels"].tolist() == [140000]
    labels, records = R.expected("random 0.3116")
    assert len(records) > 1000 and bricks_of_largest("random 0.3116") > 100
    assert sorted(R.expected("bridges outside the region")[1]["touches"].tolist()) == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]


def arms(name):
    """Voxels of the largest component with no member below them in x, y or z: each is the lowest index of its own neighbourhood, so it
    starts as a root of its own tree, and all of them but the label must be joined to it root to root."""
    d, _, lo, hi = R.cases()[name]
    labels, records = R.expected(name)
    big = records[np.argmax(records["n_voxels"])]
    member = np.pad(labels.reshape(d.shape if lo is None else tuple(hi[a] - lo[a] for a in (2, 1, 0))) == big["label"], 1)
    return int((member[1:-1, 1:-1, 1:-1] & ~member[:-2, 1:-1, 1:-1] & ~member[1:-1, :-2, 1:-1] & ~member[1:-1, 1:-1, :-2]).sum())


def bricks_of_largest(name):
    d, _, lo, hi = R.cases()[name]
    labels, records = R.expected(name)
    big = records[np.argmax(records["n_voxels"])]
    r = np.nonzero(labels == big["label"])[0]
    ext = [hi[a] - lo[a] for a in range(3)]
    local = [lo[a] - R.ORIGIN[a] for a in range(3)]
    x, y, z = r % ext[0] + local[0], (r // ext[0]) % ext[1] + local[1], r // (ext[0] * ext[1]) + local[2]
    return len(set(zip((x // 4).tolist(), (y // 4).tolist(), (z // 4).tolist())))


def test_scipy_agrees_on_count_and_sizes():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name in ("random 0.15", "random 0.3116", "random 0.5", "ragged region", "combs"):
        d, _, lo, hi = R.cases()[name]
        _, _, sl = R.region_slices(d.shape, R.ORIGIN, lo, hi)
        with np.errstate(invalid="ignore"):
            lab, n = ndimage.label(d[sl] > 0)                  # the default structure is the 6-neighbourhood
        _, records = R.expected(name)
        assert n == len(records), name
        assert sorted(np.bincount(lab.reshape(-1))[1:].tolist()) == sorted(records["n_voxels"].tolist()), name


# ---- errors and capacities ----------------------------------------------------------------------------------------------------------

def test_errors_and_capacities():
    lib = _ffi.host_lib()
    d = np.ascontiguousarray(R.cases()["ragged region"][0])
    nz, ny, nx = d.shape
    o = (C.c_int32 * 3)(*R.ORIGIN)
    lo3, hi3 = (C.c_int32 * 3)(-30, -30, -20), (C.c_int32 * 3)(-20, -25, -10)
    nc, nv = C.c_uint64(7), C.c_uint64(7)

    def call(density, lo, hi, flags=0, labels=None, lcap=0, records=None, rcap=0, dims=(nx, ny, nz)):
        nc.value = nv.value = 7
        return lib.blok_components_label(density, o, *dims, lo, hi, flags, labels, lcap, records, rcap, C.byref(nc), C.byref(nv))

    for tag, status, args in (("unknown flag", BLOK_ERR_INVALID_ARG, dict(lo=lo3, hi=hi3, flags=1)), ("lo alone", BLOK_ERR_INVALID_ARG, dict(lo=lo3, hi=None)),
                              ("hi alone", BLOK_ERR_INVALID_ARG, dict(lo=None, hi=hi3)), ("lo above hi", BLOK_ERR_INVALID_ARG, dict(lo=hi3, hi=lo3)),
                              ("leaves the box below", BLOK_ERR_UNSUPPORTED, dict(lo=(C.c_int32 * 3)(-41, -30, -20), hi=hi3)),
                              ("leaves the box above", BLOK_ERR_UNSUPPORTED, dict(lo=lo3, hi=(C.c_int32 * 3)(-20, -25, 41))),
                              ("above 2^32 cells", BLOK_ERR_UNSUPPORTED, dict(lo=None, hi=None, dims=(2048, 2048, 1024)))):
        assert call(_ffi.ptr(d), **args) == status, tag
        assert (nc.value, nv.value) == (0, 0), tag
    assert call(None, lo3, hi3) == BLOK_ERR_INVALID_ARG           # a density the call would read
    assert call(None, lo3, lo3) == 0 and (nc.value, nv.value) == (0, 0)      # an empty region reads nothing
    assert lib.blok_components_label(_ffi.ptr(d), o, nx, ny, nz, lo3, hi3, 0, None, 0, None, 0, None, None) == 0      # null count pointers
    # capacities: prefixes of the full result, the totals always
    lo, hi = R.cases()["ragged region"][2:]
    labels, records = R.expected("ragged region")
    for lcap, rcap in ((0, 0), (1, 1), (1000, 17), (len(labels), len(records)), (len(labels) + 5, len(records) + 5)):
        got_labels, got_records = label_components_host(d, R.ORIGIN, lo, hi, label_capacity=lcap, component_capacity=rcap)
        assert len(got_labels) == min(lcap, len(labels)) and len(got_records) == min(rcap, len(records))
        assert got_labels.tobytes() == labels[:lcap].tobytes() and got_records.tobytes() == records[:rcap].tobytes()
        assert label_components_host.totals == (len(records), int(records["n_voxels"].sum()))
    # a capacity below the buffer's length writes nothing past it
    buf = np.full(10, 0xABCDABCD, dtype=np.uint32)
    rec = np.zeros(3, dtype=_ffi.COMPONENT)
    rlo, rhi = (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi)
    assert call(_ffi.ptr(d), rlo, rhi, labels=_ffi.ptr(buf), lcap=4, records=_ffi.ptr(rec), rcap=2) == 0
    assert (buf[4:] == 0xABCDABCD).all() and buf[:4].tobytes() == labels[:4].tobytes()
    assert rec[:2].tobytes() == records[:2].tobytes() and rec[2].tobytes() == bytes(40)
    assert (nc.value, nv.value) == (len(records), int(records["n_voxels"].sum()))
