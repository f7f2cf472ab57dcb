"""GPU: blok_hip_terrain_reduce (HipTracer.terrain_reduce) against the composition that defines it — terrain.eval_box, then lod.reduce_host
(tests/terrain_lod_cases.py, the reference of tests/test_terrain_lod_cpu.py) — over the same case table: planes whole and in pieces, out_info
and volume_lod_info, byte for byte, for 1, 3 and 5 levels and all four flag combinations; one run on a context that never had a volume; the
level as a model against the composed route on the device; and the independence of the volume and of the other snapshots.  The entry reads
no volume, so the two brick layouts are irrelevant here: nothing is parametrised over them."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd._ffi import BlokError
from tests import terrain_lod_cases as TLC

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    yield t
    t.shutdown()


def counts(info):
    return [[int(L[k]) for k in ("n_cells", "n_filled", "n_exposed", "sum_n", "sum_e")] for L in info["level"][0][:int(info["levels"][0])]]


def planes_of(t, levels):
    return [tuple(t.volume_lod_download(j, plane) for plane in range(3)) for j in range(1, levels + 1)]


def reduce_check(t, kw, lo, hi, levels, flags, tag=""):
    want = TLC.reference(kw, lo, hi, levels, flags)
    info = t.terrain_reduce(TLC.params_of(kw), lo, hi, levels, flags)
    got = planes_of(t, levels)
    differ = [int((g[p] != w[p]).sum()) if g[p].shape == w[p].shape else -1 for g, w in zip(got, want[0]) for p in range(3)]
    print(f"{tag} region {lo}..{hi} K {levels} flags {flags}: reference {counts(want[1])}, device {counts(info)}, cells that differ per plane {differ}")
    assert info.tobytes() == want[1].tobytes() == t.volume_lod_info().tobytes(), tag
    for j, (g, w) in enumerate(zip(got, want[0]), start=1):
        for plane in range(3):
            assert g[plane].dtype == w[plane].dtype and g[plane].shape == w[plane].shape and g[plane].tobytes() == w[plane].tobytes(), (tag, j, plane)
            n = w[plane].size
            if n:
                assert t.volume_lod_download(j, plane, 0, n, page=n // 5 + 1).tobytes() == w[plane].tobytes()
                assert t.volume_lod_download(j, plane, n // 3, n - n // 3).tobytes() == w[plane].reshape(-1)[n // 3:].tobytes()


def test_a_context_that_never_had_a_volume():
    """Runs first in its own context: no volume_create before or after."""
    from blok_amd.tracer import HipTracer
    t = HipTracer(32, 32).init()
    try:
        TLC.check_reference_tells_the_flags_apart()
        lo, hi = TLC.LARGE["large_b"]
        for flags in TLC.ALL_FLAGS:
            reduce_check(t, {}, lo, hi, 3, flags, "no volume")
        with pytest.raises(BlokError) as e:
            t.volume_reduce(None, None, 1, 0)
        assert e.value.status == BLOK_ERR_NO_WORLD
    finally:
        t.shutdown()


@pytest.mark.parametrize("name,kw,lo,hi", TLC.CASES, ids=TLC.CASE_IDS)
def test_device_matches_the_composition(tr, name, kw, lo, hi):
    TLC.check_reference_tells_the_flags_apart()
    for levels in TLC.ALL_LEVELS:
        for flags in TLC.ALL_FLAGS:
            reduce_check(tr, kw, lo, hi, levels, flags, name)


def test_seamless_planes_of_a_union_are_the_parts_concatenated(tr):
    lo, hi = TLC.LARGE["large_a"]
    cut = (8, 0, 0)
    flags = TLC.SEAMLESS | TLC.VOTE_EXPOSED
    p = TLC.params_of({})
    want = TLC.reference({}, lo, hi, 3, flags)
    built = [[np.full_like(plane, 0xABCD) for plane in level] for level in want[0]]
    for part in range(8):
        plo = tuple(cut[a] if (part >> a) & 1 else lo[a] for a in range(3))
        phi = tuple(hi[a] if (part >> a) & 1 else cut[a] for a in range(3))
        info = tr.terrain_reduce(p, plo, phi, 3, flags)
        for j in range(3):
            off = [int(info["level"][0][j]["clo"][a]) - int(want[1]["level"][0][j]["clo"][a]) for a in range(3)]
            ext = [int(c) for c in info["level"][0][j]["cext"]]
            for plane in range(3):
                built[j][plane][off[2]:off[2] + ext[2], off[1]:off[1] + ext[1], off[0]:off[0] + ext[0]] = tr.volume_lod_download(j + 1, plane)
    for j in range(3):
        for plane in range(3):
            assert built[j][plane].tobytes() == want[0][j][plane].tobytes(), (j + 1, plane)


def test_lod_model_behind_terrain_reduce_equals_the_composed_route(tr):
    """volume_lod_model(K, MIN) behind terrain_reduce against volume_create at the region, volume_generate_terrain, volume_reduce,
    volume_lod_model: the voxel counts and the downloaded models."""
    lo, hi = TLC.LARGE["large_b"]
    K, MIN = 2, 3
    p = TLC.params_of({})
    tr.volume_create(lo, tuple(h - l for l, h in zip(lo, hi)))
    tr.volume_generate_terrain(p)
    composed_info = tr.volume_reduce(None, None, K, TLC.VOTE_EXPOSED)
    composed = tr.volume_lod_model(K, MIN)
    composed_voxels = tr.last_capture_voxels
    info = tr.terrain_reduce(p, lo, hi, K, TLC.VOTE_EXPOSED)
    assert info.tobytes() == composed_info.tobytes()
    direct = tr.volume_lod_model(K, MIN)
    want_voxels = int((TLC.reference({}, lo, hi, K, TLC.VOTE_EXPOSED)[0][K - 1][0] >= MIN).sum())
    print(f"model voxels: composed {composed_voxels}, direct {tr.last_capture_voxels}, host {want_voxels}")
    assert tr.last_capture_voxels == composed_voxels == want_voxels and want_voxels > 0
    a, b = tr.model_download(composed), tr.model_download(direct)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_the_volume_and_the_other_snapshots_are_left_alone_and_a_failure_keeps_the_snapshot(tr):
    rng = np.random.default_rng(11)
    shape = (32, 32, 32)
    d = np.where(rng.random(shape) < 0.3, rng.uniform(0.1, 2.0, shape), 0.0).astype(np.float32)
    m = np.where(d > 0, rng.integers(1, 9, shape), 0).astype(np.uint32)
    tr.volume_create((-16, -16, -16), shape)
    tr.volume_upload(d, m)
    tr.volume_encode_bricks()
    before = tr.volume_download()
    stream = tr.volume_bricks_download()
    p = TLC.params_of({})
    lo, hi = TLC.LARGE["large_b"]                               # overlaps the volume's box: still neither read nor written
    reduce_check(tr, {}, lo, hi, 2, TLC.VOTE_EXPOSED | TLC.SEAMLESS, "beside a volume")
    after = tr.volume_download()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(stream, tr.volume_bricks_download()))
    # every failing call leaves the snapshot: the planes and the info as they were
    kept_info, kept = tr.volume_lod_info(), planes_of(tr, 2)
    shell = TLC.params_of(dict(flags=1))
    for args, status in (((p, lo, hi, 6, 0), BLOK_ERR_INVALID_ARG), ((p, lo, hi, 0, 0), BLOK_ERR_INVALID_ARG), ((p, lo, hi, 1, 4), BLOK_ERR_INVALID_ARG),
                         ((shell, lo, hi, 1, 0), BLOK_ERR_INVALID_ARG), ((p, None, hi, 1, 0), BLOK_ERR_INVALID_ARG), ((p, lo, None, 1, 0), BLOK_ERR_INVALID_ARG),
                         ((p, (9, 0, 0), (8, 1, 1), 1, 0), BLOK_ERR_INVALID_ARG), ((p, (0, 0, 0), (65537, 1, 1), 1, 0), BLOK_ERR_UNSUPPORTED),
                         ((p, ((1 << 30) - 3, 0, 0), ((1 << 30) + 1, 4, 4), 1, 0), BLOK_ERR_UNSUPPORTED), ((p, (0, 0, 0), (65536, 65536, 4), 1, 0), BLOK_ERR_UNSUPPORTED)):
        with pytest.raises(BlokError) as e:
            tr.terrain_reduce(*args)
        assert e.value.status == status, args[1:]
    assert tr.volume_lod_info().tobytes() == kept_info.tobytes()
    assert all(x.tobytes() == y.tobytes() for a, b in zip(kept, planes_of(tr, 2)) for x, y in zip(a, b))
    # volume_reduce goes on refusing bit 2
    with pytest.raises(BlokError) as e:
        tr.volume_reduce(None, None, 1, TLC.SEAMLESS)
    assert e.value.status == BLOK_ERR_INVALID_ARG
    # an empty region is an empty, taken snapshot
    info = tr.terrain_reduce(p, (0, 0, 0), (8, 0, 8), 2, 0)
    assert int(info["level"][0][0]["n_cells"]) == 0 and tr.volume_lod_info().tobytes() == info.tobytes() and tr.volume_lod_download(1, 0).size == 0
