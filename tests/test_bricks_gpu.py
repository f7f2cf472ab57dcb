"""GPU: blok_hip_volume_encode_bricks / restore_bricks / decode_bricks against the numpy reference of the contract (tests/bricks_reference.py,
pinned in tests/test_bricks_cpu.py) over volume_download(): info, records and both payloads byte for byte, whole and in pieces, in both
modes and both brick layouts, on the shapes at which each load path can go wrong; restore and decode checked like check() of
tests/test_volume_rebuild_gpu.py (arrays, then the rebuilt tree); the snapshot's life and the error table."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import bricks as B
from blok_amd import stamp as S
from blok_amd import world as W
from blok_amd._ffi import BlokError
from tests import bricks_reference as R
from tests.conftest import SEED
from tests.test_volume_rebuild_gpu import check
from tests.volume_tree_reference import DenseModel

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
_cache = {}


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def reference(key, vol, origin, lo, hi, flags):
    """The reference's stream, computed once per content (the layouts share it; `key` names content that is never changed)."""
    k = (key, lo, hi, flags)
    if key is None or k not in _cache:
        s = R.encode(vol[0], vol[1], origin, lo, hi, flags)
        if key is None:
            return s
        _cache[k] = s
    return _cache[k]


def encode_check(t, vol, origin, lo=None, hi=None, flags=0, key=None):
    """The device's stream for the region equals the reference's over `vol` (the downloaded arrays); returns it."""
    want = reference(key, vol, origin, lo, hi, flags)
    info = t.volume_encode_bricks(lo, hi, bool(flags & R.FILLED_ONLY))
    got = t.volume_bricks_download()
    print(f"region {lo}..{hi} flags={flags}: reference {[int(want[0][k][0]) for k in ('n_bricks', 'n_density', 'n_material', 'n_voxels')]}, "
          f"device {[int(info[k][0]) for k in ('n_bricks', 'n_density', 'n_material', 'n_voxels')]}")
    assert info.tobytes() == want[0].tobytes() == got[0].tobytes()
    assert R.same_stream(got, want)
    assert R.same_stream(t.volume_bricks_download(page=7), want)           # in pieces
    return got


def make(t, keyed, origin, shape, d=None, m=None):
    t.set_volume_layout(keyed)
    t.volume_create(origin, shape)
    if d is not None:
        t.volume_upload(d, m)
    vol = t.volume_download()
    if d is not None:
        assert vol[0].tobytes() == np.ascontiguousarray(d).tobytes() and vol[1].tobytes() == np.ascontiguousarray(m).tobytes()
    return vol


def model_of(origin, shape, d, m):
    model = DenseModel(origin, shape)
    model.upload(d, m)
    return model


# ---- encode ----------------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_encode_the_shared_scene_whole_and_over_ragged_regions(tr, keyed):
    vol = make(tr, keyed, R.SCENE_ORIGIN, R.SCENE_SHAPE, *R.scene())
    for flags in (0, R.FILLED_ONLY):
        for lo, hi in R.SCENE_REGIONS + R.SCENE_ALIGNED[1:]:
            encode_check(tr, vol, R.SCENE_ORIGIN, lo, hi, flags, key="scene")


@LAYOUTS
def test_encode_the_small_volumes(tr, keyed):
    """24 x 13 x 9 with regions off the brick grid (dword loads under nx % 4 == 0), 26 x 8 x 8 (nx % 4 != 0), 264 x 8 x 8 (66 bricks along
    x: a full wave and a partial one per brick row on the vector path), 13 x 6 x 5, 1 x 2 x 3 and 5 x 9 x 2."""
    for name, origin, shape, d, m, regions in R.small_volumes():
        vol = make(tr, keyed, origin, shape, d, m)
        for flags in (0, R.FILLED_ONLY):
            for lo, hi in regions:
                got = encode_check(tr, vol, origin, lo, hi, flags, key=name)
                assert len(got[1]) > 0 or int(np.prod(got[0]["ext"][0])) < 64, (name, lo, flags)      # (a region of a cell or two may hold nothing)


@LAYOUTS
def test_encode_empty_region_nothing_stored_and_one_value(tr, keyed):
    origin, shape = (3, -2, 1), (13, 6, 5)
    vol = make(tr, keyed, origin, shape)
    for flags in (0, R.FILLED_ONLY):
        got = encode_check(tr, vol, origin, flags=flags)                                     # nothing stored
        assert int(got[0]["n_bricks"][0]) == 0 and got[0]["ext"][0].tolist() == [13, 6, 5]
    ones = np.full(shape[::-1], 1.5, np.float32), np.full(shape[::-1], 6, np.uint32)
    vol = make(tr, keyed, origin, shape, *ones)
    for flags in (0, R.FILLED_ONLY):
        got = encode_check(tr, vol, origin, flags=flags)                                     # all one value: kind 3 throughout, no payload
        assert (got[1]["kind"] == 3).all() and len(got[1]) == 4 * 2 * 2 and len(got[2]) == len(got[3]) == 0
        got = encode_check(tr, vol, origin, (5, 0, 2), (5, 3, 4), flags)                     # an empty region
        assert int(got[0]["n_bricks"][0]) == 0 and got[0]["ext"][0].tolist() == [0, 3, 2] and got[0]["lo"][0].tolist() == [5, 0, 2]
    tr.volume_restore_bricks()                                                               # of an empty region: nothing to write
    assert tr.volume_download()[0].tobytes() == ones[0].tobytes()


# ---- restore and decode ----------------------------------------------------------------------------------------------------------------------
ORIGIN, SHAPE = (-7, 3, -20), (44, 37, 30)


def content(seed=17):
    rng = np.random.default_rng(seed)
    s = SHAPE[::-1]
    d = np.where(rng.random(s) < 0.3, rng.choice(np.array([0.25, 1.0, 1.5], np.float32), s), 0.0).astype(np.float32)
    d[::3, ::2, ::5] = -0.5
    d[1::7, ::3, ::2] = np.nan
    d[rng.random(s) < 0.01] = -0.0
    m = np.where(d > 0, rng.integers(1, 6, s), 0).astype(np.uint32)
    m[rng.random(s) < 0.02] = 9
    d[10:18, 8:20, 4:30] = 1.0                                  # a solid block: uniform bricks
    m[10:18, 8:20, 4:30] = 3
    return d, m


@LAYOUTS
def test_undo_restores_the_region_bit_for_bit(tr, mats, keyed):
    d0, m0 = content()
    make(tr, keyed, ORIGIN, SHAPE, d0, m0)
    tr.volume_rebuild(mats)
    lo, hi = (2, 10, -15), (29, 33, 6)                          # around the edits below, off the brick grid
    before = encode_check(tr, (d0, m0), ORIGIN, lo, hi)
    tr.volume_apply_brush((15.5, 21.0, -4.5), 9.0, 2.0, 0)      # ADD
    tr.volume_apply_brush((12.0, 18.5, -7.0), 6.5, 0.0, 1)      # SUBTRACT: ids stay behind under density 0
    xyz = np.array([[x, y, z] for x in range(5) for y in range(3) for z in range(4)], np.int32)
    model = tr.model_create(xyz, np.full(len(xyz), 11, np.uint32))
    assert tr.volume_stamp_models(S.placement((8, 14, -12), model=model), _ffi.STAMP_SET, 1.25) == len(xyz)
    tr.model_destroy(model)
    edited = tr.volume_download()
    assert edited[0].tobytes() != d0.tobytes() and edited[1].tobytes() != m0.tobytes()
    tr.volume_restore_bricks()
    assert R.same_stream(tr.volume_bricks_download(), before)   # the snapshot is what it was
    check(tr, model_of(ORIGIN, SHAPE, d0, m0), "undo", mats)    # NaNs, negative densities and bare ids included


@LAYOUTS
def test_restore_moved_off_the_brick_grid_and_keep_others(tr, mats, keyed):
    d0, m0 = content()
    make(tr, keyed, ORIGIN, SHAPE, d0, m0)
    for flags in (0, R.FILLED_ONLY):
        lo, hi = (-3, 6, -17), (18, 25, -2)
        s = encode_check(tr, tr.volume_download(), ORIGIN, lo, hi, flags)
        for dst, keep in (((10, 14, -9), False), ((-7, 3, -20), True), ((16, 21, -5), True), (None, False)):
            now = tr.volume_download()
            want = R.decode(now[0], now[1], ORIGIN, s, dst, R.KEEP_OTHERS if keep else 0)
            tr.volume_restore_bricks(dst, keep)
            check(tr, model_of(ORIGIN, SHAPE, *want), (flags, dst, keep), mats)


@LAYOUTS
def test_decode_host_streams_into_fresh_volumes(tr, mats, keyed):
    d0, m0 = content(23)
    for flags in (0, R.FILLED_ONLY):
        s = B.encode_host(d0, m0, ORIGIN, (-3, 6, -17), (30, 38, 7), flags)          # the host build's stream
        assert R.same_stream(s, R.encode(d0, m0, ORIGIN, (-3, 6, -17), (30, 38, 7), flags))
        # into a fresh volume of the other layout than the one the parameter names, where it was taken
        zero = make(tr, not keyed, ORIGIN, SHAPE)
        tr.volume_decode_bricks(*s)
        check(tr, model_of(ORIGIN, SHAPE, *R.decode(*zero, ORIGIN, s)), ("fresh", flags), mats)
        # into a volume at another origin and of another shape, at a destination of its own, over content, both ways of writing
        origin2, shape2 = (100, -60, 5), (41, 40, 29)
        rng = np.random.default_rng(3)
        d2 = np.where(rng.random(shape2[::-1]) < 0.5, np.float32(0.75), np.float32(0)).astype(np.float32)
        m2 = np.where(d2 > 0, 2, 0).astype(np.uint32)
        for keep in (False, True):
            make(tr, keyed, origin2, shape2, d2, m2)
            dst = (104, -59, 6)
            tr.volume_decode_bricks(*s, dst_lo=dst, keep_others=keep)
            check(tr, model_of(origin2, shape2, *R.decode(d2, m2, origin2, s, dst, R.KEEP_OTHERS if keep else 0)), ("elsewhere", flags, keep), mats)


@LAYOUTS
def test_ten_encode_edit_restore_rounds(tr, mats, keyed):
    d0, m0 = content(31)
    make(tr, keyed, ORIGIN, SHAPE, d0, m0)
    tr.volume_rebuild(mats)
    rng = np.random.default_rng(41)
    model = model_of(ORIGIN, SHAPE, d0, m0)
    for k in range(10):
        c = tuple(float(v) for v in rng.uniform((5, 15, -8), (25, 28, -2)))
        r = float(rng.integers(2, 7))
        lo = tuple(int(np.floor(c[a] - r)) - 1 for a in range(3))      # the brush's box and a voxel around it
        hi = tuple(int(np.floor(c[a] + r)) + 2 for a in range(3))
        tr.volume_encode_bricks(lo, hi)
        tr.volume_apply_brush(c, r, 1.75, 0) if k % 2 == 0 else tr.volume_apply_brush(c, r, 0.0, 1)
        if k % 3 == 0:                                          # every third stroke is kept: the next rounds start from an edited world
            model.brush(c, r, 1.75 if k % 2 == 0 else 0.0, k % 2)
        else:
            tr.volume_restore_bricks()
        if k % 4 == 3:
            check(tr, model, k, mats)
    check(tr, model, "end", mats)


def test_restore_that_adds_tall_geometry_keeps_the_sun_map_valid():
    """A restore may fill voxels: after one that puts back a tower taller than anything around it, every path-traced plane is
    bit-identical with the shadow rays' map on and off (as tests/test_brush.py::test_sun_map_stays_valid_across_volume_edits does it)."""
    from blok_amd.tracer import HipTracer
    w, h = 160, 120
    mats = W.scene_materials(SEED)
    t = HipTracer(w, h).init()
    t.volume_create((0, 0, 0), (64, 96, 64), 128, 1.0)
    ids = W.scene_dense(64, SEED)
    z, y, x = np.nonzero(ids)
    t.volume_set_voxels(np.stack([x, y, z], 1).astype(np.int32), ids[z, y, x], np.ones(len(x), dtype=np.float32))
    top = int(y.max())
    tower = np.array([[x0, y0, z0] for x0 in range(28, 34) for z0 in range(30, 35) for y0 in range(top + 1, min(top + 30, 95))], np.int32)
    assert len(tower) > 100
    t.volume_set_voxels(tower, np.full(len(tower), 7, np.uint32), np.ones(len(tower), np.float32))
    lo, hi = (26, 0, 28), (37, 96, 37)
    t.volume_encode_bricks(lo, hi)                              # the world with the tower
    t.volume_apply_brush((31.0, top + 14.0, 32.5), 16.0, 0.0, 1)      # the tower dug away, and ground with it
    t.volume_rebuild(mats)
    cams = [W.scene_camera(64, 0, w, h, SEED), W.camera_look_at((5.0, 30.0, 5.0), (40.0, 12.0, 40.0), 70.0, w, h)]

    def same(tag):
        planes = []
        for cam in cams:
            t.set_sun_map(False)
            plain = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            t.set_sun_map(True)
            got = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            for k in plain:
                assert got[k].tobytes() == plain[k].tobytes(), (tag, k)
            planes.append(plain["color"].tobytes())
        return planes
    dug = same("dug")
    t.volume_restore_bricks()                                   # the tower is back: new shadows the map has to know of
    t.volume_rebuild(mats)
    assert same("restored") != dug
    t.shutdown()


# ---- the snapshot's life and the error table ---------------------------------------------------------------------------------------------------
def refused(status, call, *args, **kw):
    with pytest.raises(BlokError) as e:
        call(*args, **kw)
    assert e.value.status == status, (e.value, args, kw)


def test_snapshot_survives_edits_is_replaced_and_is_freed(tr, mats):
    d0, m0 = content()
    make(tr, True, ORIGIN, SHAPE, d0, m0)
    first = encode_check(tr, (d0, m0), ORIGIN, (0, 5, -18), (21, 30, 3))
    tr.volume_apply_brush((10.0, 20.0, -8.0), 6.0, 2.0, 0)
    tr.volume_set_voxels(np.array([[1, 6, -17]], np.int32), [4], [3.0])
    tr.volume_rebuild(mats)
    assert R.same_stream(tr.volume_bricks_download(), first)                   # later edits and a rebuild do not touch it
    second = encode_check(tr, tr.volume_download(), ORIGIN, flags=R.FILLED_ONLY)
    assert not R.same_stream(second, first) and R.same_stream(tr.volume_bricks_download(), second)      # the next encode replaces it
    tr.volume_destroy()
    for call in (tr.volume_bricks_info, tr.volume_bricks_download):
        refused(BLOK_ERR_INVALID_ARG, call)                                                            # freed with the volume
    refused(BLOK_ERR_NO_WORLD, tr.volume_encode_bricks)
    refused(BLOK_ERR_NO_WORLD, tr.volume_restore_bricks)
    refused(BLOK_ERR_NO_WORLD, tr.volume_decode_bricks, *first)
    make(tr, True, ORIGIN, SHAPE, d0, m0)
    tr.volume_encode_bricks()
    tr.volume_create(ORIGIN, SHAPE)                                                                    # a new volume frees it too
    refused(BLOK_ERR_INVALID_ARG, tr.volume_bricks_download)
    refused(BLOK_ERR_INVALID_ARG, tr.volume_restore_bricks)


@LAYOUTS
def test_error_table_leaves_volume_and_snapshots_as_they_were(tr, keyed):
    import ctypes as C
    d0, m0 = content()
    make(tr, keyed, ORIGIN, SHAPE, d0, m0)
    quads = tr.volume_extract_quads((0, 5, -18), (21, 30, 3))
    n_components = tr.volume_label_components((0, 5, -18), (21, 30, 3))[0]
    components = tr.volume_components_download(0, n_components)
    snap = encode_check(tr, (d0, m0), ORIGIN, (0, 5, -18), (21, 30, 3))
    info, records, dp, mp = snap
    lib, ctx = tr._lib, tr._ctx
    lo3, hi3 = (C.c_int32 * 3)(0, 5, -18), (C.c_int32 * 3)(21, 30, 3)
    one = np.zeros(4, np.uint32)
    hi_x, hi_y, hi_z = (ORIGIN[a] + SHAPE[a] for a in range(3))
    table = [
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_encode_bricks(ctx, lo3, hi3, 2, None))),                  # unknown flag bits
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_encode_bricks(ctx, lo3, None, 0, None))),                 # one region pointer
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_encode_bricks(ctx, None, hi3, 0, None))),
        (BLOK_ERR_INVALID_ARG, lambda: tr.volume_encode_bricks((5, 5, 5), (4, 9, 9))),                                         # lo > hi
        (BLOK_ERR_UNSUPPORTED, lambda: tr.volume_encode_bricks((ORIGIN[0] - 1, 5, -18), (21, 30, 3))),                         # leaves the box
        (BLOK_ERR_UNSUPPORTED, lambda: tr.volume_encode_bricks((0, 5, -18), (21, hi_y + 1, 3))),
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_restore_bricks(ctx, None, 2))),
        (BLOK_ERR_UNSUPPORTED, lambda: tr.volume_restore_bricks((hi_x - 20, 5, -18))),                                         # 21 cells from 20 before the end
        (BLOK_ERR_UNSUPPORTED, lambda: tr.volume_restore_bricks((0, 5, ORIGIN[2] - 1))),
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_bricks_download(ctx, _ffi.ptr(one), len(records), 1))),   # past the end
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_bricks_download(ctx, _ffi.ptr(one), len(records) + 1, 0))),
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_bricks_download(ctx, None, 0, 1))),                       # null with a count
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_brick_payload_download(ctx, 2, _ffi.ptr(one), 0, 1))),    # plane > 1
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_brick_payload_download(ctx, 0, _ffi.ptr(one), len(dp) - 1, 2))),
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_brick_payload_download(ctx, 1, None, 0, 1))),
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_decode_bricks(ctx, None, None, None, None, None, 0))),
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_decode_bricks(ctx, _ffi.ptr(info), _ffi.ptr(records), _ffi.ptr(dp), _ffi.ptr(mp), None, 2))),
        (BLOK_ERR_INVALID_ARG, lambda: tr._check(lib.blok_hip_volume_decode_bricks(ctx, _ffi.ptr(info), None, _ffi.ptr(dp), _ffi.ptr(mp), None, 0))),
        (BLOK_ERR_UNSUPPORTED, lambda: tr.volume_decode_bricks(*snap, dst_lo=(0, hi_y - 24, -18))),                            # 25 cells from 24 before the end
        (BLOK_ERR_UNSUPPORTED, lambda: tr.volume_decode_bricks(*snap, dst_lo=(0, 5, hi_z))),
    ]
    assert len(dp) >= 2 and len(mp) >= 1 and len(records) >= 4
    # a corrupted host stream, one field per case: refused on the host, nothing written
    k = int(np.flatnonzero(records["kind"] == 0)[1])
    for field, at, value in (("kind", 1, 4), ("mask", 2, 0), ("brick", 3, int(records["brick"][2])), ("density", k, int(records["density"][k]) + 1),
                             ("material", k, int(records["material"][k]) + 1), ("brick", len(records) - 1, 6 * 7 * 6)):
        bad = records.copy()
        bad[field][at] = value
        table.append((BLOK_ERR_INVALID_ARG, lambda bad=bad: tr.volume_decode_bricks(info, bad, dp, mp)))
    for field in ("version", "n_density", "n_material", "n_voxels"):
        bad = info.copy()
        bad[field] += 1
        table.append((BLOK_ERR_INVALID_ARG, lambda bad=bad: tr.volume_decode_bricks(bad, records, dp, mp)))
    for i, (status, call) in enumerate(table):
        with pytest.raises(BlokError) as e:
            call()
        assert e.value.status == status, (i, e.value)
        now = tr.volume_download()
        assert now[0].tobytes() == d0.tobytes() and now[1].tobytes() == m0.tobytes(), i
        assert R.same_stream(tr.volume_bricks_download(), snap), i
        assert tr.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes(), i
        assert tr.volume_components_download(0, n_components).tobytes() == components.tobytes(), i
    with pytest.raises(BlokError) as e:
        bad = records.copy()
        bad["kind"][5] = 9
        tr.volume_decode_bricks(info, bad, dp, mp)
    assert "kind above 3" in str(e.value) and "(record 5)" in str(e.value)       # the message names the first record that fails
    # zero counts with null arrays are no errors
    tr._check(lib.blok_hip_volume_bricks_download(ctx, None, len(records), 0))
    tr._check(lib.blok_hip_volume_brick_payload_download(ctx, 1, None, len(mp), 0))
    assert tr.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes()
