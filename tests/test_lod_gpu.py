"""GPU: blok_hip_volume_reduce / lod_info / lod_download / lod_model against the numpy model of the contract (tests/lod_reference.py, pinned
in tests/test_lod_cpu.py) over volume_download(): planes and infos byte for byte, whole and in pieces, in both brick layouts, on the shapes at
which the level-1 pass can go wrong (odd and negative origins, regions off the brick and off the 2^K grid, the seams of a wave's 128 voxels,
the ends of the lattice, 16384 cells on an axis); the level as a model against blok_hip_model_create of the model's list; the snapshot's
life and independence; the error tables; and the coarse world traced.  Every comparison is exact."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd._ffi import BlokError
from tests import limit_cases as LC
from tests import lod_reference as R

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
X = R.VOTE_EXPOSED


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    yield t
    t.shutdown()


def make(t, keyed, origin, shape, d=None, m=None):
    t.set_volume_layout(keyed)
    t.volume_create(origin, shape)
    if d is not None:
        t.volume_upload(d, m)
    return t.volume_download()


def counts(info):
    return [[int(L[k]) for k in ("n_cells", "n_filled", "n_exposed", "sum_n", "sum_e")] for L in info["level"][0][:int(info["levels"][0])]]


def planes_of(t, levels):
    return [tuple(t.volume_lod_download(j, plane) for plane in range(3)) for j in range(1, levels + 1)]


def reduce_check(t, want, lo, hi, levels, flags, pieces=True, tag=""):
    """The device's pyramid equals `want` = (levels, info) of the reference; returns the downloaded planes."""
    info = t.volume_reduce(lo, hi, levels, flags)
    got = planes_of(t, levels)
    differ = [int((g[p] != w[p]).sum()) if g[p].shape == w[p].shape else -1 for g, w in zip(got, want[0]) for p in range(3)]
    print(f"{tag} region {lo}..{hi} K {levels} flags {flags}: reference {counts(want[1])}, device {counts(info)}, cells that differ per plane {differ}")
    assert info.tobytes() == want[1].tobytes() == t.volume_lod_info().tobytes()
    for j, (g, w) in enumerate(zip(got, want[0]), start=1):
        for plane in range(3):
            assert g[plane].dtype == w[plane].dtype and g[plane].shape == w[plane].shape and g[plane].tobytes() == w[plane].tobytes(), (tag, j, plane)
            n = w[plane].size
            if pieces and n:
                assert t.volume_lod_download(j, plane, 0, n, page=7).tobytes() == w[plane].tobytes()
                assert t.volume_lod_download(j, plane, n // 3, n - n // 3).tobytes() == w[plane].reshape(-1)[n // 3:].tobytes()
    return got


@functools.lru_cache(maxsize=None)
def noise_table():
    return [(c, R.model_of(c)) for c in R.noise_cases()]


@functools.lru_cache(maxsize=None)
def seam_table():
    return [(c, R.model_of(c)) for c in R.seam_cases()]


@functools.lru_cache(maxsize=None)
def limit_table(which):
    c = R.limit_case(which)
    return c, R.model_of(c)


def table_check(t, keyed, table, pieces=lambda i: True):
    uploaded = None
    for i, (c, want) in enumerate(table):
        if uploaded is not c["d"]:
            d, m = make(t, keyed, c["origin"], c["shape"], c["d"], c["m"])
            assert d.tobytes() == c["d"].tobytes() and m.tobytes() == c["m"].tobytes()
            uploaded = c["d"]
        reduce_check(t, want, c["lo"], c["hi"], c["levels"], c["flags"], pieces(i), c["name"])


# ---- device against reference ------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_reduce_of_the_noise_box(tr, keyed):
    """13 x 10 x 7 at (-5, -3, -2), fill 0.05 and 0.5, five ids with 0 and 0xFFFFFFFF among them, K = 1 .. 5: the whole box, regions off the
    brick grid and off the 2^K grid, a one-cell region, an empty region."""
    table_check(tr, keyed, noise_table(), pieces=lambda i: i % 7 == 0)
    info = tr.volume_lod_info()                                     # the last case: the empty region
    assert int(info["ext"][0][0]) == 0 and counts(info) == [[0] * 5] * int(info["levels"][0])
    assert tr.volume_lod_download(1, 0).size == 0 and tr.volume_lod_download(1, 2, 0, 0).size == 0


@LAYOUTS
def test_reduce_at_the_seams(tr, keyed):
    """5 x 300 x 6 and its permutations: filled cells at 0, 1, 3, 4, 63, 64, 255, 256, 298, 299 along the long axis and their neighbours."""
    table_check(tr, keyed, seam_table())


@LAYOUTS
@pytest.mark.parametrize("which", LC.LIMITS)
def test_reduce_in_the_limit_boxes(tr, keyed, which):
    table_check(tr, keyed, [limit_table(which)], pieces=lambda i: False)


@pytest.mark.parametrize("box", LC.LONG_BOXES, ids=LC.LONG_IDS)
def test_reduce_of_the_long_boxes(tr, box):
    """16384 cells on one axis (always the general layout): the closed form of lod_reference.long_fill, pinned in test_lod_cpu.py."""
    d, m = R.long_fill(box)
    make(tr, True, box.origin, box.shape, d, m)
    want = R.long_expected(box, d, m)
    info = tr.volume_reduce(None, None, R.LONG_LEVELS, 0)
    for j in range(1, R.LONG_LEVELS + 1):
        L = info["level"][0][j - 1]
        assert [int(c) for c in L["clo"]] == [box.origin[a] >> j for a in range(3)]
        assert [int(L[k]) for k in ("n_filled", "n_exposed", "sum_n", "sum_e")] == [int((want[j - 1][0] > 0).sum()), int((want[j - 1][1] > 0).sum()),
                                                                                   int(want[j - 1][0].sum()), int(want[j - 1][1].sum())]
        for plane in range(3):
            assert tr.volume_lod_download(j, plane).tobytes() == want[j - 1][plane].tobytes(), (box.name, j, plane)
    assert int(info["level"][0][0]["sum_n"]) == int((d > 0).sum()) > 1000


# ---- a level as a model -----------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_lod_model_equals_model_create_of_the_reference_list(tr, keyed):
    d, m = R.noise(0.5)
    make(tr, keyed, R.NOISE_ORIGIN, R.NOISE_SHAPE, d, m)
    for levels in (1, 3):
        want, _ = R.reduce(d, m, R.NOISE_ORIGIN, None, None, levels, X)
        tr.volume_reduce(None, None, levels, X)
        for min_count in (1, 4):
            xyz, ids = R.model_voxels(want[levels - 1], min_count)
            assert len(xyz) > 0
            got = tr.volume_lod_model(levels, min_count)
            assert tr.last_capture_voxels == len(xyz)
            ref = tr.model_create(xyz, ids)
            gn, gm, gi = tr.model_download(got)
            wn, wm, wi = tr.model_download(ref)
            print(f"K {levels} min {min_count}: {len(xyz)} voxels, info {gi}")
            assert gi == wi and gn.tobytes() == wn.tobytes() and gm.tobytes() == wm.tobytes(), (levels, min_count, gi, wi)
            tr.model_destroy(ref); tr.model_destroy(got)


def test_lod_model_of_a_level_without_such_a_cell_and_the_error_table(tr):
    d, m = R.noise(0.05)
    make(tr, True, R.NOISE_ORIGIN, R.NOISE_SHAPE, d, m)
    tr.volume_reduce(None, None, 2, 0)
    n2 = tr.volume_lod_download(2, 0)
    before = tr.model_create([(0, 0, 0)], [1])
    assert int(n2.max()) < 64
    for args, status in (((2, 64), BLOK_ERR_UNSUPPORTED), ((0, 1), BLOK_ERR_INVALID_ARG), ((3, 1), BLOK_ERR_INVALID_ARG), ((2, 0), BLOK_ERR_INVALID_ARG),
                         ((2, 65), BLOK_ERR_INVALID_ARG), ((1, 9), BLOK_ERR_INVALID_ARG)):
        with pytest.raises(BlokError) as e:
            tr.volume_lod_model(*args)
        assert e.value.status == status, args
    assert tr._lib.blok_hip_volume_lod_model(tr._ctx, 2, 1, None, None) == BLOK_ERR_INVALID_ARG
    tr.volume_reduce((0, 0, 0), (0, 4, 4), 2, 0)                    # an empty region: no cell at all
    with pytest.raises(BlokError) as e:
        tr.volume_lod_model(1, 1)
    assert e.value.status == BLOK_ERR_UNSUPPORTED
    assert tr.model_create([(0, 0, 0)], [1]) == before + 1          # no id was consumed


# ---- errors -------------------------------------------------------------------------------------------------------------------------------------
def test_reduce_and_download_errors_leave_everything_as_it_was():
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    try:
        for call, status in ((t.volume_reduce, BLOK_ERR_NO_WORLD), (t.volume_lod_info, BLOK_ERR_INVALID_ARG), (lambda: t.volume_lod_download(1, 0), BLOK_ERR_INVALID_ARG),
                             (lambda: t.volume_lod_model(1, 1), BLOK_ERR_INVALID_ARG)):      # no volume
            with pytest.raises(BlokError) as e:
                call()
            assert e.value.status == status
        d, m = R.noise(0.5)
        o = R.NOISE_ORIGIN
        make(t, True, o, R.NOISE_SHAPE, d, m)
        for call in (t.volume_lod_info, lambda: t.volume_lod_download(1, 0), lambda: t.volume_lod_model(1, 1)):      # a volume, no snapshot yet
            with pytest.raises(BlokError) as e:
                call()
            assert e.value.status == BLOK_ERR_INVALID_ARG
        info = t.volume_reduce(None, None, 2, X)
        kept = [[p.copy() for p in level] for level in planes_of(t, 2)]
        for kw, status in ((dict(levels=0), BLOK_ERR_INVALID_ARG), (dict(levels=6), BLOK_ERR_INVALID_ARG), (dict(flags=2), BLOK_ERR_INVALID_ARG),
                           (dict(lo=(0, 0, 0)), BLOK_ERR_INVALID_ARG), (dict(hi=(1, 1, 1)), BLOK_ERR_INVALID_ARG), (dict(lo=(1, 0, 0), hi=(0, 1, 1)), BLOK_ERR_INVALID_ARG),
                           (dict(lo=(-6, 0, 0), hi=(0, 1, 1)), BLOK_ERR_UNSUPPORTED), (dict(lo=(0, 0, 0), hi=(9, 1, 1)), BLOK_ERR_UNSUPPORTED)):
            with pytest.raises(BlokError) as e:
                t.volume_reduce(**kw)
            assert e.value.status == status, kw
        n1 = kept[0][0].size
        out = np.zeros(4, np.uint32)
        lib, ctx = t._lib, t._ctx
        for level, plane, ptr, first, count in ((0, 0, out, 0, 1), (3, 0, out, 0, 1), (1, 3, out, 0, 1), (1, 0, out, n1, 1), (1, 0, out, 0, n1 + 1),
                                                (1, 2, out, n1 + 1, 0), (1, 0, None, 0, 1)):
            assert lib.blok_hip_volume_lod_download(ctx, level, plane, None if ptr is None else _ffi.ptr(ptr), first, count) == BLOK_ERR_INVALID_ARG, (level, plane, first, count)
        assert lib.blok_hip_volume_lod_download(ctx, 2, 2, None, kept[1][2].size, 0) == 0      # an empty range at the end is fine
        assert lib.blok_hip_volume_lod_info(ctx, None) == BLOK_ERR_INVALID_ARG
        assert t.volume_lod_info().tobytes() == info.tobytes()
        for a, b in zip(planes_of(t, 2), kept):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        d2, m2 = t.volume_download()
        assert d2.tobytes() == d.tobytes() and m2.tobytes() == m.tobytes()
    finally:
        t.shutdown()


# ---- independence and life ----------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_snapshot_life_and_independence(keyed):
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    try:
        d, m = R.noise(0.5)
        o = R.NOISE_ORIGIN
        make(t, keyed, o, R.NOISE_SHAPE, d, m)
        # the other snapshots, taken first
        quads = t.volume_extract_quads()
        t.volume_label_components()
        labels = t.volume_labels_download(0, d.size)
        t.volume_encode_bricks()
        bricks = t.volume_bricks_download()
        t.volume_distance_field(None, None, 3)
        distance = t.volume_distance_download()
        t.volume_column_field()
        columns = t.volume_columns_download(0), t.volume_columns_download(1)
        want = R.reduce(d, m, o, None, None, 3, X)
        kept = reduce_check(t, want, None, None, 3, X, pieces=False, tag="life")
        # reduce changes nothing
        d1, m1 = t.volume_download()
        assert d1.tobytes() == d.tobytes() and m1.tobytes() == m.tobytes()
        assert t.volume_quads_download(0, len(quads)).tobytes() == quads.tobytes() and t.volume_labels_download(0, d.size).tobytes() == labels.tobytes()
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(t.volume_bricks_download(), bricks))
        assert t.volume_distance_download().tobytes() == distance.tobytes()
        assert t.volume_columns_download(0).tobytes() == columns[0].tobytes() and t.volume_columns_download(1).tobytes() == columns[1].tobytes()
        # later edits do not touch it
        t.volume_set_voxels([(o[0] + 1, o[1] + 1, o[2] + 1), (o[0] + 2, o[1] + 1, o[2] + 1)], [9, 9], [1.0, 0.0])
        assert t.volume_lod_info().tobytes() == want[1].tobytes()
        assert all(a[p].tobytes() == b[p].tobytes() for a, b in zip(planes_of(t, 3), kept) for p in range(3))
        # a scroll leaves it alone: it is a record of world cells
        scrolled = t.volume_scroll((4, 0, -4))
        assert t.volume_lod_info().tobytes() == want[1].tobytes()
        assert all(a[p].tobytes() == b[p].tobytes() for a, b in zip(planes_of(t, 3), kept) for p in range(3))
        # the next reduce replaces it (of the scrolled, edited volume)
        d2, m2 = t.volume_download()
        o2 = tuple(int(c) for c in scrolled["origin"][0])
        assert o2 == (o[0] + 4, o[1], o[2] - 4)
        reduce_check(t, R.reduce(d2, m2, o2, None, None, 1, 0), None, None, 1, 0, pieces=False, tag="after the scroll")
        with pytest.raises(BlokError):
            t.volume_lod_download(2, 0)                              # the new snapshot has one level
        # the volume's end is the snapshot's
        t.volume_destroy()
        with pytest.raises(BlokError) as e:
            t.volume_lod_info()
        assert e.value.status == BLOK_ERR_INVALID_ARG
        make(t, keyed, o, R.NOISE_SHAPE, d, m)
        t.volume_reduce(None, None, 1, 0)
        t.volume_create(o, R.NOISE_SHAPE)
        with pytest.raises(BlokError) as e:
            t.volume_lod_download(1, 0)
        assert e.value.status == BLOK_ERR_INVALID_ARG
    finally:
        t.shutdown()


# ---- the coarse world -----------------------------------------------------------------------------------------------------------------------------
def test_coarse_world_is_traced_at_voxel_size_4():
    """Level 2 of a box with three isolated coarse cells, installed as a dense world at voxel size 4: axis-parallel rays through each cell
    report its lattice coordinates, its voted id and the exact t of its near face (every term a product of powers of two and small integers)."""
    from blok_amd.tracer import HipTracer
    origin, shape = (-8, 4, 0), (32, 32, 32)
    cells = {(-1, 2, 3): 5, (3, 5, 1): 6, (5, 8, 7): 7}             # level-2 cell -> id; no two share a row along any axis
    d, m = np.zeros(shape[::-1], np.float32), np.zeros(shape[::-1], np.uint32)
    for k, (c, ident) in enumerate(cells.items()):
        for dx, dy, dz in ((0, 0, 0), (3, 3, 3), (1, 2, 0))[:k + 1]:
            x, y, z = 4 * c[0] + dx - origin[0], 4 * c[1] + dy - origin[1], 4 * c[2] + dz - origin[2]
            d[z, y, x], m[z, y, x] = 1.0, ident
    t = HipTracer(96, 64).init()
    try:
        make(t, True, origin, shape, d, m)
        info = t.volume_reduce(None, None, 2, X)
        n, ids = t.volume_lod_download(2, 0), t.volume_lod_download(2, 2)
        clo = [int(c) for c in info["level"][0][1]["clo"]]
        assert clo == [-2, 1, 0] and int(info["level"][0][1]["n_filled"]) == 3
        t.volume_destroy()
        t.set_voxel_size(4.0)
        t.add_dense(np.where(n >= 1, ids, 0).astype(np.uint32), tuple(clo))
        rays, want = [], []
        for c, ident in cells.items():
            for axis in range(3):
                for sign in (1, -1):
                    org = [4.0 * c[a] + 2.0 for a in range(3)]
                    org[axis] = -64.0 if sign > 0 else 192.0
                    direction = [0.0, 0.0, 0.0]
                    direction[axis] = float(sign)
                    rays.append((tuple(org), 0.0, tuple(direction), 1000.0))
                    want.append((4.0 * c[axis] + 64.0 if sign > 0 else 192.0 - 4.0 * (c[axis] + 1), ident, c))
        hits = t.trace_rays(np.array(rays, dtype=_ffi.RAY))
        for h, (t_near, ident, c) in zip(hits, want):
            print(f"cell {c}: t {float(h['t'])} (want {t_near}), voxel {h['voxel'].tolist()}, id {int(h['material_id'])}")
            assert int(h["hit"]) == 1 and tuple(int(v) for v in h["voxel"]) == c and int(h["material_id"]) == ident and float(h["t"]) == t_near
    finally:
        t.shutdown()
