"""CPU: the terrain function's host build (include/blok_world.h: blok_terrain_*, through blok_amd/csrc/common/terrain_core.h) against the
independent numpy reference (tests/terrain_reference.py), analytic cases, the refusals and the record's layout.  Every comparison is exact."""
from __future__ import annotations

import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import terrain as T
from blok_amd._ffi import BlokError
from tests import terrain_reference as R

from tests.terrain_cases import FIELDS, ISSUE, params, prior      # noqa: F401


def same(p, d, lo, hi, prior=None):
    dd, mm = (None, None) if prior is None else prior
    got_d, got_m, n = T.eval_box(p, lo, hi, dd, mm)
    ref_d, ref_m = R.eval_box(d, lo, hi, dd, mm)
    assert np.array_equal(got_d.view(np.uint32), ref_d.view(np.uint32)) and np.array_equal(got_m, ref_m)
    return got_d, got_m, n


def test_record_layout():
    assert C.sizeof(_ffi.TerrainParams) == 72
    assert [getattr(_ffi.TerrainParams, f).offset for f in FIELDS] == list(range(0, 72, 4))
    assert FIELDS[1] == "base_height" and FIELDS[16] == "density" and FIELDS[17] == "flags"


def test_quoted_values_and_digest():
    p, d = params(density=1.0)
    cols = [[0, 0], [-1, -1], [1000, -777], [-100000, 65536]]
    assert T.height(p, cols).tolist() == [17, 18, 5, -6]
    assert [int(R.height(d, x, z)) for x, z in cols] == [17, 18, 5, -6]
    lo, hi = (-32, -40, -32), (32, 24, 32)
    dd, mm, n = same(p, d, lo, hi)
    assert n == 165076 and [int((mm == k).sum()) for k in (1, 2, 3, 4)] == [4096, 11187, 141919, 7874]
    assert hashlib.sha256(mm.tobytes()).hexdigest() == "478f1291a017bb31d5478a1b78ffa954b3a0d476e72672b0215c8f3bb0b0d208"
    at = lambda x, y, z: int(mm[z - lo[2], y - lo[1], x - lo[0]])
    assert (at(0, -30, 0), at(5, -25, -7), at(-32, -40, -32)) == (0, 3, 4)
    assert np.array_equal(dd > 0, mm != 0)


@pytest.mark.parametrize("origin", [(-37, -33, -21), (-9, -25, -6), (16777210, -30, -16777230), (1073741815, -28, -1073741840), (0, -12, 0)])
@pytest.mark.parametrize("flags", [0, 1, 3, 4, 5, 7])
def test_eval_equals_the_reference(origin, flags):
    size = (23, 41, 18)                                  # ragged: no multiple of four
    hi = tuple(o + s for o, s in zip(origin, size))
    p, d = params(flags=flags)
    same(p, d, origin, hi, prior(size[::-1]) if flags & 4 else None)


@pytest.mark.parametrize("kw", [dict(cave_octaves=0), dict(cave_octaves=1), dict(cave_octaves=3, cave_cell_log2=5), dict(cave_octaves=4, cave_cell_log2=3),
                                dict(height_octaves=1), dict(height_octaves=8, height_cell_log2=7, amplitude=65536, base_height=-30000),
                                dict(height_cell_log2=0, height_octaves=1, cave_cell_log2=0, cave_octaves=1, ore_cell_log2=0),
                                dict(height_cell_log2=12, cave_cell_log2=12, ore_cell_log2=12, cave_octaves=4),
                                dict(cave_threshold=0), dict(cave_threshold=65536), dict(ore_threshold=0), dict(ore_threshold=65536),
                                dict(cave_roof=0, soil_depth=0), dict(base_height=1 << 24, amplitude=0), dict(base_height=-(1 << 24))])
def test_parameter_extremes_equal_the_reference(kw):
    for flags in (0, 3):
        p, d = params(flags=flags, **kw)
        y0 = d["base_height"] + (int(R.height(d, 5, -3)) - d["base_height"]) - 14
        same(p, d, (-3, y0, -11), (18, y0 + 27, 9))


@pytest.mark.parametrize("flags", [0, 1])
def test_regions_side_by_side_are_one_region(flags):
    p, d = params(flags=flags)
    lo, hi, mid = (-13, -31, -10), (21, 9, 16), (5, -12, 1)
    whole_d, whole_m, n = T.eval_box(p, lo, hi)
    parts_d, parts_m, total = np.zeros_like(whole_d), np.zeros_like(whole_m), 0
    for pick in itertools.product((0, 1), repeat=3):
        l = [lo[a] if pick[a] == 0 else mid[a] for a in range(3)]
        h = [mid[a] if pick[a] == 0 else hi[a] for a in range(3)]
        dd, mm, k = T.eval_box(p, l, h)
        sl = tuple(slice(l[a] - lo[a], h[a] - lo[a]) for a in (2, 1, 0))
        parts_d[sl], parts_m[sl] = dd, mm
        total += k
    assert np.array_equal(parts_d, whole_d) and np.array_equal(parts_m, whole_m) and total == n


def test_close_sides_adds_exactly_the_walls():
    p1, d1 = params(flags=1)
    p3, _ = params(flags=3)
    lo, hi = (-13, -31, -10), (21, 9, 16)
    _, open_m, _ = T.eval_box(p1, lo, hi)
    _, closed_m, _ = T.eval_box(p3, lo, hi)
    S, _ = R.solid_box(d1, lo, hi)
    wall = np.zeros_like(S)
    wall[0], wall[-1], wall[:, :, 0], wall[:, :, -1] = True, True, True, True
    extra = (closed_m != 0) & (open_m == 0)
    assert np.array_equal(extra, S & wall & (open_m == 0)) and not ((open_m != 0) & (closed_m == 0)).any()
    assert np.array_equal(closed_m[open_m != 0], open_m[open_m != 0])


def test_closed_sub_regions_add_exactly_their_walls():
    """A region tiled by 2 x 2 x 2 closed sub-regions: the open shell of the whole plus every solid voxel on an x or z face of a tile."""
    p1, d1 = params(flags=1)
    p3, _ = params(flags=3)
    lo, hi, mid = (-13, -31, -10), (21, 9, 16), (5, -12, 1)
    _, open_m, _ = T.eval_box(p1, lo, hi)
    S, _ = R.solid_box(d1, lo, hi)
    tiled, wall = np.zeros_like(open_m), np.zeros_like(S)
    for pick in itertools.product((0, 1), repeat=3):
        l = [lo[a] if pick[a] == 0 else mid[a] for a in range(3)]
        h = [mid[a] if pick[a] == 0 else hi[a] for a in range(3)]
        sl = tuple(slice(l[a] - lo[a], h[a] - lo[a]) for a in (2, 1, 0))
        tiled[sl] = T.eval_box(p3, l, h)[1]
        w = wall[sl]
        w[0], w[-1], w[:, :, 0], w[:, :, -1] = True, True, True, True
    assert np.array_equal(tiled != 0, (open_m != 0) | (S & wall))
    assert np.array_equal(tiled[open_m != 0], open_m[open_m != 0])


def test_shell_is_the_solid_voxels_with_an_empty_neighbour():
    p1, d = params(flags=1)
    lo, hi = (-20, -36, -20), (20, 12, 20)
    _, shell, _ = T.eval_box(p1, lo, hi)
    S, _ = R.solid_box(d, [v - 1 for v in lo], [v + 1 for v in hi])
    c = S[1:-1, 1:-1, 1:-1]
    assert not ((shell != 0) & ~c).any()
    six = S[1:-1, 1:-1, :-2] & S[1:-1, 1:-1, 2:] & S[1:-1, :-2, 1:-1] & S[1:-1, 2:, 1:-1] & S[:-2, 1:-1, 1:-1] & S[2:, 1:-1, 1:-1]
    assert np.array_equal(c & (shell == 0), c & six)


def test_analytic_cases():
    p, _ = params(amplitude=0, base_height=7, cave_octaves=0, ore_threshold=65536, soil_depth=3)
    _, m, _ = T.eval_box(p, (-5, -2, -5), (6, 12, 6))
    col = m[:, :, 0][0]
    assert np.array_equal(m, np.broadcast_to(col[None, :, None], m.shape))
    assert col.tolist() == [3] * 6 + [2] * 3 + [1] + [0] * 4           # y = -2..3 rock, 4..6 soil, 7 surface, above empty
    p, _ = params(cave_threshold=65536, cave_roof=0)
    assert T.eval_box(p, (-8, -60, -8), (8, 40, 8))[2] == 0
    rng = np.random.default_rng(5)
    xz = rng.integers(-(1 << 30), 1 << 30, (100000, 2))
    p, d = params(base_height=-123, amplitude=77)
    h = T.height(p, xz)
    assert h.min() >= -123 and h.max() < -123 + 77
    assert np.array_equal(h, R.height(d, xz[:, 0], xz[:, 1]))
    p, _ = params(cave_octaves=0)
    for x, z in [(3, 4), (-70, 15)]:
        _, m, _ = T.eval_box(p, (x, -30, z), (x + 1, 40, z + 1))
        assert int(np.nonzero(m[0, :, 0])[0].max()) - 30 == int(T.height(p, [[x, z]])[0])


def test_default_params_are_valid_and_make_a_landscape():
    for n in (16, 64, 100, 1024):
        p = T.default_params(n, 7)
        assert T.validate(p) and p.seed == 7 and 0 <= p.base_height and p.base_height + p.amplitude <= n
    p = T.default_params(64)
    _, m, n = T.eval_box(p, (0, 0, 0), (64, 64, 64))
    assert 0.1 * 64 ** 3 < n < 0.6 * 64 ** 3 and set(np.unique(m)) == {0, 1, 2, 3, 4}


def test_refusals():
    bad = [dict(height_octaves=0), dict(height_octaves=9, height_cell_log2=12), dict(height_octaves=4, height_cell_log2=2), dict(height_cell_log2=13),
           dict(cave_octaves=5, cave_cell_log2=12), dict(cave_octaves=3, cave_cell_log2=1), dict(cave_cell_log2=13), dict(ore_cell_log2=13),
           dict(cave_threshold=65537), dict(ore_threshold=65537), dict(amplitude=65537), dict(base_height=(1 << 24) + 1),
           dict(base_height=-(1 << 24) - 1), dict(density=0.0), dict(density=-1.0), dict(density=float("inf")), dict(density=float("nan")),
           dict(flags=8), dict(flags=2), dict(flags=6)]
    lib = _ffi.host_lib()
    for kw in bad:
        p, _ = params(**kw)
        assert not T.validate(p), kw
        d0, m0 = prior((4, 4, 4))
        with pytest.raises(BlokError) as e:
            T.eval_box(p, (0, 0, 0), (4, 4, 4), d0, m0)
        assert e.value.status == -1
        with pytest.raises(BlokError):
            T.height(p, [[0, 0]])
    p, _ = params()
    assert T.validate(p)
    with pytest.raises(BlokError):
        T.eval_box(p, (0, 5, 0), (4, 4, 4))
    assert T.eval_box(p, (0, 4, 0), (4, 4, 4))[2] == 0                    # an empty region is fine
    assert lib.blok_terrain_validate(None) == -1 and lib.blok_terrain_default_params(0, 1, C.byref(p)) == -1


def test_benchmark_scene_is_unchanged():
    """G(64, seed) as the parent commit 82fa3a7 generates it (its hash now comes from the header shared with the terrain)."""
    from blok_amd import world as W
    ids = W.scene_dense(64)
    assert int((ids != 0).sum()) == 10082
    assert hashlib.sha256(ids.tobytes()).hexdigest() == "3ca6742de5d10d9be585dc43ae1ccb473190f14481b1027ec73868fe2fe7ed37"
