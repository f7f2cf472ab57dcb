"""GPU: blok_hip_volume_apply_shapes against the host build (blok_amd/shapes.py: apply_host, itself pinned to the numpy model in
tests/test_shapes_cpu.py): after every call the downloaded arrays bit for bit and the written count; after a rebuild the tree against
volume_tree_reference byte for byte, which is what proves the masks, occupancy words and dirty flags.  Both brick layouts.

Not covered: BLOK_ERR_UNSUPPORTED for a volume above 2^32 cells (its two arrays alone are 32 GiB)."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import shapes as SH
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import limit_cases as LC
from tests import shapes_cases as K
from tests import shapes_reference as R
from tests.conftest import SEED
from tests.volume_tree_reference import box_levels, reference_tree

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
RAGGED_ORIGIN, RAGGED = (-7, 3, -20), (70, 37, 33)              # tail lanes in x (70 = 64 + 6), ragged tiles in y and z
CUBE_ORIGIN, CUBE = (-32, -32, -32), (64, 64, 64)


def _tracer(w=64, h=64):
    from blok_amd.tracer import HipTracer
    return HipTracer(w, h).init()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def arrays_equal(t, d, m, tag):
    gd, gm = t.volume_download()
    assert gd.tobytes() == d.tobytes(), (tag, "density", int((gd.view(np.uint32) != d.view(np.uint32)).sum()))
    assert gm.tobytes() == m.tobytes(), (tag, "ids", int((gm != m).sum()))


def tree_equal(t, d, m, origin, mats, tag):
    """After a rebuild the tree is reference_tree of the host arrays, byte for byte.  Returns (nodes, material ids)."""
    st = t.volume_rebuild(mats)
    levels = box_levels(d.shape[::-1])
    ref_nodes, ref_mats = reference_tree(R.filled(d), m, levels)
    assert (st.n_voxels, st.n_tree_nodes, st.levels, tuple(st.origin)) == (len(ref_mats), len(ref_nodes), levels, tuple(origin)), tag
    nodes, ids = t.download_tree()
    assert nodes.tobytes() == ref_nodes.tobytes(), (tag, "nodes")
    assert ids.tobytes() == ref_mats.tobytes(), (tag, "materials")
    return nodes, ids


class Both:
    """The same tables to the volume and to the host build's arrays."""

    def __init__(self, t, keyed, origin, dims, d0, m0):
        self.t, self.origin, self.dims = t, origin, dims
        t.set_volume_layout(keyed)
        t.volume_create(origin, dims)
        self.reset(d0, m0)

    def reset(self, d0, m0):
        self.t.volume_upload(d0, m0)
        self.d, self.m = d0.copy(), m0.copy()

    def apply(self, shapes, tag):
        table = R.record(shapes)
        want = SH.apply_host(self.d, self.m, self.origin, table)
        got = self.t.volume_apply_shapes(table)
        print(f"{tag}: written {got}, host build {want}")
        assert got == want, (tag, got, want)
        arrays_equal(self.t, self.d, self.m, tag)
        return want


# ---- ragged box and the keyed cube ------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("origin,dims", [(RAGGED_ORIGIN, RAGGED), (CUBE_ORIGIN, CUBE)], ids=["70x37x33", "64x64x64"])
def test_every_kind_and_op_on_a_ragged_box_and_a_cube(keyed, origin, dims, mats):
    t = _tracer()
    d0, m0 = R.noise(dims)
    b = Both(t, keyed, origin, dims, d0, m0)
    total = 0
    for k, (tag, shapes) in enumerate(K.kinds_by_ops(origin, dims)):
        if k % 7 == 0:
            b.reset(d0, m0)
        total += b.apply(shapes, tag)
        if k % 7 in (2, 6):                                        # behind the ERASE of each kind, and behind all seven ops
            tree_equal(t, b.d, b.m, origin, mats, tag)
    for tag, shapes in K.placements(origin, dims)[::3] + K.zero_radii(origin, dims):
        total += b.apply(shapes, tag)
    # one table of everything, over the prior content: shapes of all kinds overlapping in order
    b.reset(d0, m0)
    table = [s for _, shapes in K.kinds_by_ops(origin, dims) for s in shapes]
    rng = np.random.default_rng(3)
    table = [table[i] for i in rng.permutation(len(table))]
    total += b.apply(table, "all 28 in one table")
    tree_equal(t, b.d, b.m, origin, mats, "all 28 in one table")
    assert total > 100000
    t.shutdown()


# ---- a long list ------------------------------------------------------------------------------------------------------------------------
def long_case():
    """(pre-state, shapes) of K.long_list on the ragged box, and — on the model alone, over the one tile the shapes lie in — how many of the
    129 adjacent pairs change the arrays when swapped, and how many of the first 129 shapes when dropped."""
    d0, m0 = R.noise(RAGGED, seed=11)
    shapes = K.long_list(RAGGED_ORIGIN, d0, m0)
    td, tm = np.ascontiguousarray(d0[:4, :4, :64]), np.ascontiguousarray(m0[:4, :4, :64])
    masks = [R.inside_box(s, RAGGED_ORIGIN, (64, 4, 4)) for s in shapes]
    assert all(mk.sum() == 3 for mk in masks), "every shape lies in the tile"

    def run(order):
        d, m = td.copy(), tm.copy()
        for i in order:
            R.apply_one(d, m, RAGGED_ORIGIN, shapes[i], masks[i])
        return d.tobytes() + m.tobytes()

    n = len(shapes)
    base = run(range(n))
    swapped = sum(run(list(range(i)) + [i + 1, i] + list(range(i + 2, n))) != base for i in range(n - 1))
    dropped = sum(run(list(range(i)) + list(range(i + 1, n))) != base for i in range(n - 1))
    return d0, m0, shapes, swapped, dropped


@pytest.fixture(scope="module")
def long_list_case():
    return long_case()


@LAYOUTS
def test_a_list_of_130_shapes_on_one_tile_keeps_its_order(keyed, mats, long_list_case):
    d0, m0, shapes, swapped, dropped = long_list_case
    print(f"adjacent pairs whose swap changes the arrays: {swapped} of 129; shapes whose loss does: {dropped} of 129")
    assert len(shapes) == 130 and swapped >= 100 and dropped >= 100
    t = _tracer()
    b = Both(t, keyed, RAGGED_ORIGIN, RAGGED, d0, m0)
    assert b.apply(shapes, "130 on one tile") >= 300
    tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, "130 on one tile")
    # the same 130 behind and among larger shapes that cover the tile and its neighbours: lists of 130 and more, several tiles
    b.reset(d0, m0)
    around = [R.vbox(RAGGED_ORIGIN, tuple(RAGGED_ORIGIN[k] + (70, 9, 6)[k] for k in range(3)), R.ADD, value=0.125),
              R.shape(R.ELLIPSOID, R.PAINT, a=K.c_of((RAGGED_ORIGIN[0] + 60, RAGGED_ORIGIN[1] + 3, RAGGED_ORIGIN[2] + 3)), r=(40, 12, 12), material=90)]
    b.apply(around[:1] + shapes[:70] + around[1:] + shapes[70:] + around, "130 among larger shapes")
    tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, "130 among larger shapes")
    t.shutdown()


# ---- a stroke ---------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_a_stroke_of_40_capsules_across_tiles(keyed, mats):
    t = _tracer()
    d0, m0 = R.noise(RAGGED, seed=2)
    b = Both(t, keyed, RAGGED_ORIGIN, RAGGED, d0, m0)
    add = K.stroke(RAGGED_ORIGIN, RAGGED, R.ADD, value=0.75)
    lo = np.min([[R.extent(s, k)[0] for k in range(3)] for s in add], axis=0) // 2 - np.array(RAGGED_ORIGIN)
    hi = np.max([[R.extent(s, k)[1] for k in range(3)] for s in add], axis=0) // 2 - np.array(RAGGED_ORIGIN)
    assert lo[0] < 64 <= hi[0] and hi[1] // 4 - lo[1] // 4 >= 4 and hi[2] // 4 - lo[2] // 4 >= 4, "the chain crosses tiles on all three axes"
    assert len(add) == 40 and b.apply(add, "stroke ADD") > 5000
    tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, "stroke ADD")
    assert b.apply(K.stroke(RAGGED_ORIGIN, RAGGED, R.PAINT, radius=9, material=33), "stroke PAINT") > 2000
    tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, "stroke PAINT")
    assert b.apply(K.stroke(RAGGED_ORIGIN, RAGGED, R.SUBTRACT, radius=5, value=-0.5), "stroke SUBTRACT") > 1000
    tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, "stroke SUBTRACT")
    t.shutdown()


# ---- commit groups ----------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_far_apart_shapes_commit_apart_and_joined_ones_together(keyed, mats):
    origin, dims = (-40, -44, -24), (96, 80, 64)
    t = _tracer()
    d0, m0 = R.noise(dims, seed=7)
    b = Both(t, keyed, origin, dims, d0, m0)
    hi = tuple(origin[k] + dims[k] for k in range(3))
    corners = [R.shape(R.ELLIPSOID, R.SET, a=K.c_of((origin[0] + 5, origin[1] + 6, origin[2] + 5)), r=(9, 11, 9), material=11, value=1.0),
               R.vbox((hi[0] - 9, hi[1] - 7, hi[2] - 10), (hi[0] - 1, hi[1], hi[2] - 2), R.ERASE)]
    bridge = R.shape(R.CAPSULE, R.KEEP, a=K.c_of((origin[0] + 5, origin[1] + 6, origin[2] + 5)), b=K.c_of((hi[0] - 5, hi[1] - 4, hi[2] - 6)), r=(3, 0, 0), material=12, value=0.5)
    path = 0 if keyed else 2                                       # volume_refresh_counts: the keyed edit path, or the general layout's

    def refreshes(shapes, tag):
        before = t.volume_refresh_counts()
        b.apply(shapes, tag)
        after = t.volume_refresh_counts()
        tree_equal(t, b.d, b.m, origin, mats, tag)
        return tuple(x - y for x, y in zip(after, before))

    apart = refreshes(corners, "two corners")
    assert apart[path] == 2 and sum(apart) == 2, apart             # one commit each: nothing between them is refreshed
    b.reset(d0, m0)
    joined = refreshes(corners + [bridge], "two corners and a bridge")
    assert joined[path] == 1 and sum(joined) == 1, joined
    b.reset(d0, m0)
    assert sum(refreshes([bridge] + corners + K.outside(origin, dims), "bridge first, outsiders dropped")) == 1
    t.shutdown()


# ---- clipping ---------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_clipping_at_every_face_and_a_table_wholly_outside(keyed, mats):
    t = _tracer()
    d0, m0 = R.noise(RAGGED, seed=4)
    b = Both(t, keyed, RAGGED_ORIGIN, RAGGED, d0, m0)
    for op in (R.SET, R.ERASE, R.PAINT):
        b.reset(d0, m0)
        for tag, shapes in K.clipped(RAGGED_ORIGIN, RAGGED, op):
            assert b.apply(shapes, (op, tag)) > 0
        # (the last of them covers the whole box: behind ERASE nothing is left, and an empty world has no tree to compare)
        b.apply([K.kind_shape(R.ELLIPSOID, RAGGED_ORIGIN, RAGGED, R.KEEP, material=9, value=0.5)], (op, "keep"))
        tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, ("clipped", op))
    b.reset(d0, m0)
    before = t.volume_refresh_counts()
    assert b.apply(K.outside(RAGGED_ORIGIN, RAGGED), "all outside") == 0
    assert t.volume_refresh_counts() == before                     # nothing to commit
    arrays_equal(t, d0, m0, "all outside")
    t.shutdown()


# ---- ids under an unchanged mask --------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("op", [R.PAINT, R.REPLACE], ids=["PAINT", "REPLACE"])
def test_paint_and_replace_alone_change_the_material_array_and_no_node(keyed, op, mats):
    t = _tracer()
    d0, m0 = R.noise(RAGGED, seed=9)
    b = Both(t, keyed, RAGGED_ORIGIN, RAGGED, d0, m0)
    nodes0, ids0 = tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, "before")
    shape = K.kind_shape(R.CAPSULE, RAGGED_ORIGIN, RAGGED, op, material=200, match=3)
    assert b.apply([shape], "ids only") > 100
    nodes1, ids1 = tree_equal(t, b.d, b.m, RAGGED_ORIGIN, mats, "after")
    assert nodes1.tobytes() == nodes0.tobytes() and len(ids1) == len(ids0) and (ids1 != ids0).sum() > 100
    t.shutdown()


# ---- the lattice's ends -----------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("which", LC.LIMITS)
def test_shapes_at_and_past_the_ends_of_the_lattice(keyed, which, mats):
    origin, dims = LC.limit_origin(which, LC.SHAPE), LC.SHAPE
    t = _tracer()
    d0, m0 = R.noise(dims, seed=13)
    b = Both(t, keyed, origin, dims, d0, m0)
    total = 0
    for tag, shapes in K.clipped(origin, dims, R.SET) + K.clipped(origin, dims, R.SUBTRACT):      # reach past every face: past the lattice's end where the box touches it
        total += b.apply(shapes, (which, tag))
    hi = LC.box_hi(origin, dims)
    far = [R.shape(R.CAPSULE, R.KEEP, a=K.c_of(tuple(c - 900 for c in origin)), b=K.c_of(tuple(c + 900 for c in hi)), r=(1024, 0, 0), material=5, value=0.5),
           R.shape(R.ELLIPSOID, R.PAINT, a=tuple(2 * c for c in hi), r=(1024, 1024, 1024), material=6),
           R.vbox(tuple(max(c - 100, -65536) for c in origin), tuple(c + 40 for c in origin), R.ERASE)]
    assert all(abs(c) <= R.COORD_MAX for s in far for c in s["a"] + s["b"]) and SH.check_host(R.record(far)) is None
    total += b.apply(far, (which, "at the record's limits"))
    total += b.apply(K.stroke(origin, dims, R.ADD, value=1.25) + K.outside(origin, dims), (which, "stroke"))
    tree_equal(t, b.d, b.m, origin, mats, which)
    assert total > 100000
    t.shutdown()


# ---- the entry's checks -----------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing():
    import ctypes as C
    t = _tracer()
    good = R.vbox((-5, 5, -18), (20, 30, 5), R.SET, material=2, value=1.0)
    with pytest.raises(BlokError) as e:                             # no volume
        t.volume_apply_shapes(R.record([good]))
    assert e.value.status == R.NO_WORLD
    d0, m0 = R.noise(K.CPU_SHAPE)
    t.volume_create(K.CPU_ORIGIN, K.CPU_SHAPE)
    t.volume_upload(d0, m0)
    before = t.volume_refresh_counts()
    for text, bad in K.bad_shapes():
        for at in (0, 2):
            table = [good, good, good]
            table[at] = bad
            with pytest.raises(BlokError) as e:
                t.volume_apply_shapes(R.record(table))
            assert e.value.status == R.INVALID_ARG and f"shape {at}: " in str(e.value) and text in str(e.value), (text, str(e.value))
    lib, n = _ffi.hip_lib(), C.c_uint64(7)
    assert lib.blok_hip_volume_apply_shapes(t._ctx, None, 2, C.byref(n)) == R.INVALID_ARG and n.value == 0
    many = np.repeat(R.record([good]), R.SHAPES_MAX + 1)
    assert lib.blok_hip_volume_apply_shapes(t._ctx, _ffi.ptr(many), len(many), C.byref(n)) == R.INVALID_ARG
    assert lib.blok_hip_volume_apply_shapes(None, _ffi.ptr(many), 1, None) == R.INVALID_ARG
    arrays_equal(t, d0, m0, "refused")
    assert t.volume_refresh_counts() == before
    # n = 0 is fine, with or without a table or a counter
    assert t.volume_apply_shapes(np.zeros(0, _ffi.SHAPE)) == 0
    assert lib.blok_hip_volume_apply_shapes(t._ctx, _ffi.ptr(many), 0, None) == 0
    arrays_equal(t, d0, m0, "empty table")
    # and a good call with a null counter writes
    d, m = d0.copy(), m0.copy()
    SH.apply_host(d, m, K.CPU_ORIGIN, R.record([good]))
    assert lib.blok_hip_volume_apply_shapes(t._ctx, _ffi.ptr(many), 1, None) == 0
    arrays_equal(t, d, m, "null counter")
    t.shutdown()
