"""CPU: blok_stamp_voxels / blok_capture_voxels (blok_amd/csrc/host/stamp.cpp through blok_amd/stamp.py) against the independent numpy
model of the contract (tests/stamp_reference.py), and that model against hand-computed cases."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import stamp as ST
from blok_amd._ffi import BlokError
from tests import stamp_reference as R

BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
MODES = (R.SET, R.KEEP, R.ERASE)
ORIGIN, SHAPE_ZYX = (-9, -7, -5), (16, 20, 24)               # a 24 x 20 x 16 box at a negative origin


def prior_content(shape_zyx=SHAPE_ZYX, seed=5):
    """Filled voxels of several densities next to every kind of empty one: 0, -0.0, negative and NaN, all with non-zero ids."""
    rng = np.random.default_rng(seed)
    values = np.array([0.0, -0.0, -0.5, np.nan, 0.7, 2.0, 1.0, 0.25], dtype=np.float32)
    d = values[rng.integers(0, len(values), size=shape_zyx)]
    m = rng.integers(1, 1 << 20, size=shape_zyx).astype(np.uint32)
    return np.ascontiguousarray(d), np.ascontiguousarray(m)


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def both(prior, origin, xyz, mats, placement, mode, value=1.5):
    """(reference arrays and count, host library arrays and count) for one stamp over copies of `prior`."""
    rd, rm = prior[0].copy(), prior[1].copy()
    n_ref = R.stamp(rd, rm, origin, xyz, mats, placement, mode, value)
    hd, hm = prior[0].copy(), prior[1].copy()
    offset, axis, flip = placement
    n_host = ST.stamp_voxels_host(hd, hm, origin, xyz, mats, ST.placement(offset, axis, flip), mode, value)
    return (rd, rm, n_ref), (hd, hm, n_host)


# ---- the reference itself, against cases worked out by hand ------------------------------------------------------------------------

L_MODEL = (np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], dtype=np.int32), np.array([1, 2, 3], dtype=np.uint32))


@pytest.mark.parametrize("axis, flip, expected", [
    ((0, 1, 2), 0, {(3, 3, 3): 1, (4, 3, 3): 2, (3, 4, 3): 3}),          # identity: w = offset + v'
    ((0, 1, 2), 1, {(2, 3, 3): 1, (1, 3, 3): 2, (2, 4, 3): 3}),          # x flipped: w.x = 3 - 1 - v'.x
    # local x -> world y flipped, local y -> world z, local z -> world x flipped:  w = (3 - 1 - v'.z, 3 - 1 - v'.x, 3 + v'.y)
    ((1, 2, 0), 5, {(2, 2, 3): 1, (2, 1, 3): 2, (2, 2, 4): 3}),
])
def test_reference_places_an_l_shaped_model_where_the_contract_says(axis, flip, expected):
    d = np.zeros((8, 8, 8), dtype=np.float32)
    m = np.zeros((8, 8, 8), dtype=np.uint32)
    assert R.stamp(d, m, (0, 0, 0), *L_MODEL, ((3, 3, 3), axis, flip), R.SET, 2.0) == 3
    got = {(int(x), int(y), int(z)): int(m[z, y, x]) for z, y, x in zip(*np.nonzero(d > 0))}
    assert got == expected
    assert set(np.unique(d)) == {np.float32(0.0), np.float32(2.0)}
    # the same three voxels at a negative box origin
    d2 = np.zeros((8, 8, 8), dtype=np.float32)
    m2 = np.zeros((8, 8, 8), dtype=np.uint32)
    R.stamp(d2, m2, (-5, -6, -7), *L_MODEL, ((3 - 5, 3 - 6, 3 - 7), axis, flip), R.SET, 2.0)
    assert d2.tobytes() == d.tobytes() and m2.tobytes() == m.tobytes()


def test_reference_keep_erase_and_last_duplicate():
    d = np.zeros((4, 4, 4), dtype=np.float32)
    m = np.zeros((4, 4, 4), dtype=np.uint32)
    d[0, 0, 0], m[0, 0, 0] = 1.0, 9                            # filled: KEEP leaves it
    d[0, 0, 1], m[0, 0, 1] = np.nan, 8                         # NaN is empty: KEEP fills it
    d[0, 1, 0], m[0, 1, 0] = -1.0, 7                           # negative is empty
    assert R.stamp(d, m, (0, 0, 0), *L_MODEL, ((0, 0, 0), (0, 1, 2), 0), R.KEEP, 3.0) == 2
    assert (d[0, 0, 0], m[0, 0, 0], d[0, 0, 1], m[0, 0, 1], d[0, 1, 0], m[0, 1, 0]) == (1.0, 9, 3.0, 2, 3.0, 3)
    assert R.stamp(d, m, (0, 0, 0), *L_MODEL, ((0, 0, 0), (0, 1, 2), 0), R.ERASE, 3.0) == 3
    assert not d.any() and not m.any()
    xyz = np.array([(1, 1, 1), (2, 1, 1), (1, 1, 1)], dtype=np.int32)
    assert R.stamp(d, m, (0, 0, 0), xyz, np.array([4, 5, 6], dtype=np.uint32), ((0, 0, 0), (0, 1, 2), 0), R.KEEP, 1.0) == 2
    assert m[1, 1, 1] == 6 and m[1, 1, 2] == 5                 # the last entry of a voxel named twice wins, also under KEEP


# ---- the host library against the reference -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_every_orientation_equals_the_reference(mode):
    xyz, mats = R.small_model()
    prior = prior_content()
    results = set()
    for axis, flip in R.ORIENTATIONS:
        ref, host = both(prior, ORIGIN, xyz, mats, ((2, 3, 1), axis, flip), mode)
        assert R.clipped(xyz, ORIGIN, SHAPE_ZYX, ((2, 3, 1), axis, flip)) == 0
        assert host[2] == ref[2] and same(host, ref), (axis, flip)
        assert ref[2] > 0
        results.add(ref[0].tobytes() + ref[1].tobytes())
    assert len(results) == 48, "two orientations gave the same arrays: an ignored orientation could pass"


# an offset ON a face of the box [-9, 15) x [-7, 13) x [-5, 11): the model has voxels on both sides of zero along every local axis, so under
# every orientation some of it lands on either side of that face
CLIP_OFFSETS = {"-x": (-9, 3, 1), "+x": (15, 3, 1), "-y": (2, -7, 1), "+y": (2, 13, 1), "-z": (2, 3, -5), "+z": (2, 3, 11)}


@pytest.mark.parametrize("mode", MODES)
def test_clipping_at_each_face_and_wholly_outside(mode):
    xyz, mats = R.small_model()
    prior = prior_content()
    for face, offset in CLIP_OFFSETS.items():
        for axis, flip in (((0, 1, 2), 0), ((1, 2, 0), 5), ((2, 1, 0), 2)):
            place = (offset, axis, flip)
            ref, host = both(prior, ORIGIN, xyz, mats, place, mode)
            n_clipped = R.clipped(xyz, ORIGIN, SHAPE_ZYX, place)
            assert 0 < n_clipped < len(xyz), (face, axis, flip)
            assert ref[2] > 0, (face, axis, flip)
            assert host[2] == ref[2] and same(host, ref), (face, axis, flip)
    for offset in ((60, 3, 1), (2, -40, 1), (2, 3, 2 ** 31 - 1), (-2 ** 31, 3, 1)):      # wholly outside, also at the ends of int32
        ref, host = both(prior, ORIGIN, xyz, mats, (offset, (0, 1, 2), 3), mode)
        assert ref[2] == 0 and host[2] == 0 and same(host, ref) and same(host, prior)


@pytest.mark.parametrize("mode", MODES)
def test_two_overlapping_placements_in_order(mode):
    xyz_a, mats_a = R.small_model()
    xyz_b, mats_b = xyz_a.copy(), mats_a + np.uint32(5000)
    place_a, place_b = ((2, 3, 1), (0, 1, 2), 0), ((4, 2, 2), (1, 0, 2), 2)
    wa = {tuple(w): int(m) for w, m in zip(R.world_voxels(xyz_a, *place_a), mats_a)}
    wb = {tuple(w): int(m) for w, m in zip(R.world_voxels(xyz_b, *place_b), mats_b)}
    overlap = set(wa) & set(wb)
    assert overlap and any(wa[w] != wb[w] for w in overlap)
    prior = prior_content()
    rd, rm = prior[0].copy(), prior[1].copy()
    hd, hm = prior[0].copy(), prior[1].copy()
    for (xyz, mats), place in (((xyz_a, mats_a), place_a), ((xyz_b, mats_b), place_b)):
        n_ref = R.stamp(rd, rm, ORIGIN, xyz, mats, place, mode, 1.5)
        n_host = ST.stamp_voxels_host(hd, hm, ORIGIN, xyz, mats, ST.placement(*place), mode, 1.5)
        assert n_ref == n_host
    assert same((hd, hm), (rd, rm))
    if mode == R.SET:                                          # the later placement won where both wrote
        assert all(int(rm[w[2] - ORIGIN[2], w[1] - ORIGIN[1], w[0] - ORIGIN[0]]) == wb[w] for w in overlap)


def test_duplicates_in_the_list_follow_the_last_one():
    xyz, mats = R.small_model()
    xyz2 = np.concatenate([xyz, xyz[::3]])
    mats2 = np.concatenate([mats, mats[::3] + np.uint32(77)])
    for mode in MODES:
        ref, host = both(prior_content(), ORIGIN, xyz2, mats2, ((2, 3, 1), (2, 0, 1), 6), mode)
        assert host[2] == ref[2] and same(host, ref)


REGIONS = [(None, None), ((-8, -5, -4), (11, 9, 8)), ((-3, -7, -5), (-2, 13, 11)), ((-9, 2, -5), (15, 3, 11)), ((-9, -7, 6), (15, 13, 7)),
           ((0, 0, 0), (1, 1, 1))]


def test_capture_equals_the_reference():
    d, m = prior_content()
    m[d > 0.9] = 0                                             # filled voxels with material id 0 are filled voxels
    assert ((d > 0) & (m == 0)).sum() > 100
    for lo, hi in REGIONS:
        want = R.capture(d, m, ORIGIN, lo, hi)
        got = ST.capture_voxels_host(d, m, ORIGIN, lo, hi)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (lo, hi)
        assert ST.capture_voxels_host(d, m, ORIGIN, lo, hi, count_only=True) == len(want[1])
        if lo is not None and len(want[1]):
            assert (want[0] >= 0).all() and (want[0] < np.array(hi) - np.array(lo)).all()
    assert len(R.capture(d, m, ORIGIN, (-8, -5, -4), (11, 9, 8))[1]) > 500
    assert (R.capture(d, m, ORIGIN)[1] == 0).any()


def test_capture_writes_a_prefix_when_the_capacity_is_smaller():
    d, m = prior_content()
    want = R.capture(d, m, ORIGIN)
    xyz = np.full((10, 3), -1, dtype=np.int32)
    mats = np.zeros(10, dtype=np.uint32)
    n = C.c_uint64(0)
    o = (C.c_int32 * 3)(*ORIGIN)
    assert _ffi.host_lib().blok_capture_voxels(_ffi.ptr(d), _ffi.ptr(m), o, 24, 20, 16, None, None, _ffi.ptr(xyz), _ffi.ptr(mats), 7, C.byref(n)) == 0
    assert n.value == len(want[1])
    assert (xyz[:7] == want[0][:7]).all() and (mats[:7] == want[1][:7]).all() and (xyz[7:] == -1).all()


def test_round_trip_capture_stamp_capture():
    d, m = prior_content()
    lo, hi = (-8, -5, -4), (11, 9, 8)
    xyz, mats = ST.capture_voxels_host(d, m, ORIGIN, lo, hi)
    d2, m2 = np.zeros_like(d), np.zeros_like(m)
    assert ST.stamp_voxels_host(d2, m2, ORIGIN, xyz, mats, ST.placement(lo), R.SET, 1.0) == len(mats)
    xyz2, mats2 = ST.capture_voxels_host(d2, m2, ORIGIN, lo, hi)
    assert xyz2.tobytes() == xyz.tobytes() and mats2.tobytes() == mats.tobytes()
    assert ST.capture_voxels_host(d2, m2, ORIGIN, count_only=True) == len(mats)      # nothing landed outside the region


def test_refused_arguments_leave_the_arrays_untouched():
    xyz, mats = R.small_model()
    prior = prior_content()
    d, m = prior[0].copy(), prior[1].copy()
    good = ST.placement((2, 3, 1))

    def refused(status, place=good, mode=R.SET, value=1.0):
        with pytest.raises(BlokError) as e:
            ST.stamp_voxels_host(d, m, ORIGIN, xyz, mats, place, mode, value)
        assert e.value.status == status
        assert same((d, m), prior)

    refused(BLOK_ERR_INVALID_ARG, mode=3)
    refused(BLOK_ERR_INVALID_ARG, mode=-1)
    for value in (0.0, -1.0, float("nan"), float("inf")):
        refused(BLOK_ERR_INVALID_ARG, value=value)
        refused(BLOK_ERR_INVALID_ARG, mode=R.KEEP, value=value)
    bad = good.copy(); bad["axis"] = (0, 0, 2)
    refused(BLOK_ERR_INVALID_ARG, place=bad)
    bad = good.copy(); bad["flip"] = 8
    refused(BLOK_ERR_INVALID_ARG, place=bad)
    bad = good.copy(); bad["reserved"] = (0, 1, 0)
    refused(BLOK_ERR_INVALID_ARG, place=bad)
    # ERASE ignores the value
    assert ST.stamp_voxels_host(d, m, ORIGIN, xyz, mats, good, R.ERASE, float("nan")) == len(mats)
    lib, o, n = _ffi.host_lib(), (C.c_int32 * 3)(*ORIGIN), C.c_uint64(9)
    assert lib.blok_stamp_voxels(_ffi.ptr(d), _ffi.ptr(m), o, 24, 20, 16, None, _ffi.ptr(mats), len(mats), _ffi.ptr(good), 0, 1.0, C.byref(n)) == BLOK_ERR_INVALID_ARG
    assert lib.blok_stamp_voxels(_ffi.ptr(d), _ffi.ptr(m), o, 24, 20, 16, _ffi.ptr(xyz), _ffi.ptr(mats), len(mats), None, 0, 1.0, C.byref(n)) == BLOK_ERR_INVALID_ARG
    assert n.value == 0
    # capture: the region convention of blok_quads_extract
    for lo, hi, status in (((0, 0, 0), None, BLOK_ERR_INVALID_ARG), (None, (0, 0, 0), BLOK_ERR_INVALID_ARG), ((3, 0, 0), (2, 5, 5), BLOK_ERR_INVALID_ARG),
                           ((-10, 0, 0), (2, 5, 5), BLOK_ERR_UNSUPPORTED), ((0, 0, 0), (2, 5, 12), BLOK_ERR_UNSUPPORTED)):
        with pytest.raises(BlokError) as e:
            ST.capture_voxels_host(d, m, ORIGIN, lo, hi)
        assert e.value.status == status
    assert ST.capture_voxels_host(d, m, ORIGIN, (1, 1, 1), (1, 5, 5), count_only=True) == 0      # an empty region is not an error
