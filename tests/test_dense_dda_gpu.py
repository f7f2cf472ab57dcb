"""GPU (-m gpu): the dense-grid kernel (dense_kernels.hip over dense_core.h) through the C ABI, against the oracle on every pixel — and, where
a world is too large to hand to the oracle whole, against the tree kernel on every pixel plus the oracle on what it can hold.  Cameras inside,
outside and grazing; extents around a tile edge (the tiling kernel's padding); the tile bits at and past the LDS limit; every output
combination at the frame's borders; TAA jitter; the lifetime of the kept grid; determinism.  No record is excluded anywhere; the hit / miss
floors are figures the oracle alone reaches (it reports 1.2 to 1.5 times each floor)."""
import itertools

import numpy as np
import pytest

from blok_amd import world as W
from tests import oracle_ffi as O
from tests.conftest import SEED, records_equal
from tests.test_dense_dda_cpu import DIMS, ORIGINS, SIGNS, fill_grid, oracle_world

pytestmark = pytest.mark.gpu
FW, FH = 203, 117                                  # odd, no multiple of the 8 x 8 wave tile


@pytest.fixture(scope="module")
def tracer_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from blok_amd.tracer import HipTracer
    from blok_amd import _ffi
    assert _ffi.HIP_LIB.exists(), "libblok_hip.so must be built in-tree"
    return HipTracer


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def dense_tracer(tracer_cls, w, h):
    tr = tracer_cls(w, h).init()
    tr.set_dense_dda(True)
    return tr


def ragged_grid(fill, seed=12):
    """37 x 22 x 51 [z][y][x] at a negative origin: no extent a multiple of 8."""
    rng = np.random.default_rng(seed)
    shape = (37, 22, 51)
    if fill >= 1.0:
        return rng.integers(1, 300, size=shape).astype(np.uint32)
    return np.where(rng.random(shape) < fill, rng.integers(1, 300, size=shape), 0).astype(np.uint32)


RAGGED_ORIGIN = (-20, 5, -9)


def random_cameras(lo, hi, n_each, seed, w=FW, h=FH):
    """n_each cameras inside the box, outside it looking in, and grazing (in the plane of a face of the box, looking along it), with
    10 to 140 degree fields of view."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    mid, ext = 0.5 * (lo + hi), hi - lo
    cams = []
    for k in range(3 * n_each):
        fov = float(rng.uniform(10.0, 140.0))
        kind = k % 3
        if kind == 0:
            pos = rng.uniform(lo, hi)
            tgt = rng.uniform(lo, hi)
        elif kind == 1:
            d = rng.normal(size=3)
            pos = mid + d / np.linalg.norm(d) * float(rng.uniform(0.8, 2.5)) * np.linalg.norm(ext)
            tgt = rng.uniform(lo, hi)
        else:
            a = int(rng.integers(0, 3))
            pos = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext)
            pos[a] = (lo, hi)[int(rng.integers(0, 2))][a]           # exactly in the plane of a face
            b = (a + 1 + int(rng.integers(0, 2))) % 3
            pos[b] = lo[b] - float(rng.uniform(1.0, 30.0))
            tgt = pos.copy()
            tgt[b] = hi[b] + 10.0                                    # along the face
        cams.append(W.camera_look_at(tuple(pos), tuple(tgt), fov, w, h))
    return cams


def camera_octants(cams, w, h):
    seen = set()
    for c in cams:
        d = O.primary_rays(c, w, h, stride=7)["dir"]
        seen |= {tuple(np.sign(v)) for v in d[(d != 0).all(axis=1)]}
    return seen


# floors (hits, misses) over the 33 cameras of one fill: test_random_cameras
CAMERA_FLOORS = {0.001: (9500, 600000), 0.03: (190000, 420000), 0.5: (250000, 350000), 1.0: (280000, 320000)}


@pytest.mark.parametrize("fill", [0.001, 0.03, 0.5, 1.0])
def test_random_cameras(tracer_cls, mats, fill):
    ids = ragged_grid(fill)
    nz, ny, nx = ids.shape
    lo = np.array(RAGGED_ORIGIN)
    cams = random_cameras(lo, lo + (nx, ny, nz), 11, seed=int(fill * 1000))
    assert len(cams) >= 30 and camera_octants(cams, FW, FH) == set(SIGNS)
    pw = oracle_world(ids, RAGGED_ORIGIN)
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    tr = dense_tracer(tracer_cls, FW, FH)
    tr.add_dense(ids, RAGGED_ORIGIN, mats)
    hits = misses = 0
    for k, cam in enumerate(cams):
        ref, ctr = lat.trace_primary(cam, FW, FH, threads=8)
        got = tr.draw_frame(cam).reshape(-1)
        eq = records_equal(got, ref)
        assert eq.all(), (fill, k, int((~eq).sum()), got[~eq][:3], ref[~eq][:3])
        hits += int(ctr["hits"])
        misses += int(ctr["rays"] - ctr["hits"])
    tr.shutdown()
    print(f"fill {fill}: oracle hits {hits}, misses {misses}")
    assert hits >= CAMERA_FLOORS[fill][0] and misses >= CAMERA_FLOORS[fill][1], (fill, hits, misses)


# ---- extents: dense_tile_kernel's padding ----------------------------------------------------------------------------------------------------
SWEEP_SHAPES = [s for k, s in enumerate(itertools.product(DIMS, repeat=3)) if k % 6 == 0 or s in ((1, 1, 1), (8, 8, 8), (9, 9, 9), (17, 17, 17))]   # (nx, ny, nz)


def test_extent_sweep(tracer_cls, mats):
    """A fifth of the CPU file's 125 extent combinations plus the four cubes, both origins, corner / half / solid fills, three cameras each
    at 61 x 37, one context re-uploaded every time."""
    w, h = 61, 37
    tr = dense_tracer(tracer_cls, w, h)
    rng = np.random.default_rng(6)
    hits = misses = 0
    seen = set()
    assert len(SWEEP_SHAPES) >= 24
    for origin in ORIGINS:
        for nx, ny, nz in SWEEP_SHAPES:
            lo = np.array(origin, dtype=np.float64)
            hi = lo + (nx, ny, nz)
            cams = [W.camera_look_at(tuple(hi + (6.0, 9.0, 7.0)), tuple(0.5 * (lo + hi)), 50.0, w, h),
                    W.camera_look_at(tuple(lo - (11.0, 3.0, 5.0)), tuple(hi - 0.25), 35.0, w, h),
                    W.camera_look_at(tuple(0.5 * (lo + hi) + (0.3, 0.2, 0.1)), tuple(hi + (1.0, -2.0, 3.0)), 120.0, w, h)]
            seen |= camera_octants(cams, w, h)
            for fill in ("corners", "half", "solid"):
                ids = fill_grid((nz, ny, nx), fill, rng)
                ids.flat[0] = ids.flat[0] or 5
                pw = oracle_world(ids, origin)
                lat = O.Lattice(pw.nodes, pw.sub_chunks)
                tr.add_dense(ids, origin, mats)
                for k, cam in enumerate(cams):
                    ref, ctr = lat.trace_primary(cam, w, h)
                    got = tr.draw_frame(cam).reshape(-1)
                    eq = records_equal(got, ref)
                    assert eq.all(), ((nx, ny, nz), origin, fill, k, int((~eq).sum()), got[~eq][:3], ref[~eq][:3])
                    hits += int(ctr["hits"])
                    misses += int(ctr["rays"] - ctr["hits"])
    tr.shutdown()
    print(f"extent sweep: oracle hits {hits}, misses {misses}")
    assert seen == set(SIGNS)
    assert hits >= SWEEP_GPU_FLOORS[0] and misses >= SWEEP_GPU_FLOORS[1], (hits, misses)


SWEEP_GPU_FLOORS = (250000, 500000)


# ---- the tile bits at and past the LDS limit ----------------------------------------------------------------------------------------------------
def slab(tiles_x):
    """One voxel thick in y, tiles_x x 1 x 512 tiles, filled in a few places only (so that the oracle's chunked world stays small): the four
    corners, the middle, and — where there is one — the tile column past x = 4096, whose tiles' bits lie in words 8192 and up."""
    nx, nz = tiles_x * 8, 4096
    ids = np.zeros((nz, 1, nx), np.uint32)
    rng = np.random.default_rng(tiles_x)
    spots = [(0, 0), (nx - 100, 0), (0, nz - 100), (nx - 100, nz - 100), (2000, 2000), (nx - 100, 2000), (nx - 100, 3000)]
    for x0, z0 in spots:
        blk = np.where(rng.random((100, 100)) < 0.3, rng.integers(1, 300, size=(100, 100)), 0).astype(np.uint32)
        ids[z0:z0 + 100, 0, x0:x0 + 100] = blk
    ids[nz - 1, 0, nx - 1] = 299                                    # the last cell of the last tile
    ids[0, 0, nx - 1] = 298
    return ids, spots


@pytest.mark.parametrize("tiles_x", [512, 513], ids=["lds_8192_words", "global_8208_words"])
def test_tile_bits_at_and_past_the_lds_limit(tracer_cls, mats, tiles_x):
    """512 x 1 x 512 tiles = exactly kDenseLdsWords words (the LDS path at its limit); 513 x 1 x 512 = the global path.  The device build
    accepts both extents (7 levels, inside int16).  The oracle on every pixel (its world holds the filled spots' chunks only), the tree
    kernel on every pixel too."""
    w, h = 403, 227
    ids, spots = slab(tiles_x)
    nz, _, nx = ids.shape
    words = (tiles_x * 512 + 31) // 32
    assert (words == 8192) if tiles_x == 512 else (words > 8192)              # kDenseLdsWords (dense_kernels.h)
    z, y, x = np.nonzero(ids)
    assert ((x >> 3) + tiles_x * (z >> 3)).max() // 32 == words - 1             # the last word holds a set bit
    pw = oracle_world(ids, (0, 0, 0))
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    tr = dense_tracer(tracer_cls, w, h)
    tree = tracer_cls(w, h).init()
    tr.add_dense(ids, (0, 0, 0), mats)
    tree.add_dense(ids, (0, 0, 0), mats)
    cams = []
    for x0, z0 in spots:
        c = (x0 + 50.0, 0.5, z0 + 50.0)
        cams.append(W.camera_look_at((c[0] + 3.0, 90.0, c[2] + 5.0), c, 70.0, w, h))                      # above
        cams.append(W.camera_look_at((c[0] - 49.7, 0.5, c[2] - 48.3), (c[0] + 50.0, 0.5, c[2] + 41.0), 100.0, w, h))   # inside the slab's plane
        cams.append(W.camera_look_at((c[0] - 120.0, 1.0 + 1e-3, c[2] - 90.0), (c[0] + 60.0, 1.0, c[2] + 55.0), 40.0, w, h))   # grazing its top
    cams.append(W.camera_look_at((nx + 40.0, 30.0, nz + 40.0), (nx - 200.0, 0.0, nz - 200.0), 60.0, w, h))
    cams.append(W.camera_look_at((-500.0, 3000.0, -500.0), (nx / 2.0, 0.0, nz / 2.0), 90.0, w, h))          # the whole slab from far above
    assert camera_octants(cams, w, h) == set(SIGNS)
    hits = misses = 0
    for k, cam in enumerate(cams):
        got = tr.draw_frame(cam).reshape(-1)
        ref, ctr = lat.trace_primary(cam, w, h, threads=8)
        eq = records_equal(got, ref)
        assert eq.all(), (tiles_x, k, int((~eq).sum()), got[~eq][:3], ref[~eq][:3])
        assert records_equal(got, tree.draw_frame(cam).reshape(-1)).all(), (tiles_x, k)
        hits += int(ctr["hits"])
        misses += int(ctr["rays"] - ctr["hits"])
    tr.shutdown(); tree.shutdown()
    print(f"slab {tiles_x}: oracle hits {hits}, misses {misses}")
    assert hits >= SLAB_FLOORS[0] and misses >= SLAB_FLOORS[1], (hits, misses)


SLAB_FLOORS = (300000, 1200000)


# ---- outputs, jitter, lifetime, determinism -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(mats):
    ids = ragged_grid(0.03)
    pw = oracle_world(ids, RAGGED_ORIGIN)
    cams = [W.camera_look_at((80.0, 60.0, -70.0), (5.0, 15.0, 9.0), 60.0, FW, FH), W.camera_look_at((3.3, 14.2, 7.7), (40.0, 9.0, 31.0), 110.0, FW, FH),
            W.camera_look_at((5.5, 200.0, 9.5), (5.5, 0.0, 9.5), 30.0, FW, FH), W.camera_look_at((-60.0, 20.0, 40.0), (31.0, 5.0, -9.0), 25.0, FW, FH)]
    return ids, pw, cams


GUARD = 64


def device_frame(tr, cam, rect, want_hits, want_rgba, stream=None):
    """One launch into fresh device buffers with a guard of GUARD elements behind each; (records or None, pixels or None)."""
    import torch
    x0, y0, w, h = rect
    n = w * h
    hits = torch.full((n + GUARD, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want_hits else None
    rgba = torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want_rgba else None
    torch.cuda.synchronize()
    tr.draw_frame_device(cam, hits.data_ptr() if want_hits else 0, rgba.data_ptr() if want_rgba else 0, rect=rect,
                         stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    out = []
    for buf in (hits, rgba):
        if buf is None:
            out.append(None)
            continue
        a = buf.cpu().numpy()
        assert (a[n:] == 0x5A5A5A5A).all(), "wrote behind the rectangle"
        out.append(a[:n].copy())
    return out[0], None if out[1] is None else out[1].view(np.uint32)


def test_outputs_and_rectangles(tracer_cls, mats, ragged):
    ids, pw, cams = ragged
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    tr = dense_tracer(tracer_cls, FW, FH)
    tree = tracer_cls(FW, FH).init()
    tr.add_dense(ids, RAGGED_ORIGIN, mats); tree.add_dense(ids, RAGGED_ORIGIN, mats)
    rects = [(0, 0, FW, FH), (0, 0, 1, 1), (FW - 1, 0, 1, 1), (0, FH - 1, 1, 1), (FW - 1, FH - 1, 1, 1), (100, 60, 1, 1),
             (0, 13, 9, 70), (FW - 11, 5, 11, 90), (20, 0, 150, 7), (33, FH - 10, 99, 10), (0, 0, FW, 1), (0, 0, 1, FH), (7, 9, 64, 8), (60, 30, 65, 17)]
    hits = misses = 0
    for k, cam in enumerate(cams):
        full_ref, ctr = lat.trace_primary(cam, FW, FH, threads=8)
        full_ref = full_ref.reshape(FH, FW)
        hits += int(ctr["hits"]); misses += int(ctr["rays"] - ctr["hits"])
        for rect in rects:
            x0, y0, w, h = rect
            ref = np.ascontiguousarray(full_ref[y0:y0 + h, x0:x0 + w]).reshape(-1)
            ref_rgba = tree.shade_rgba8(cam, rect).reshape(-1)
            only_hits, none = device_frame(tr, cam, rect, True, False)
            none2, only_rgba = device_frame(tr, cam, rect, False, True)
            both_hits, both_rgba = device_frame(tr, cam, rect, True, True)
            assert none is None and none2 is None
            assert records_equal(only_hits, ref).all() and records_equal(both_hits, ref).all(), (k, rect)
            assert np.array_equal(only_rgba, ref_rgba) and np.array_equal(both_rgba, ref_rgba), (k, rect)
            assert records_equal(tr.draw_frame(cam, rect).reshape(-1), ref).all(), (k, rect)
        assert len(np.unique(tree.shade_rgba8(cam))) > 5
    tr.shutdown(); tree.shutdown()
    print(f"outputs: oracle hits {hits}, misses {misses}")
    assert hits >= 25000 and misses >= 45000, (hits, misses)


def test_taa_jitter(tracer_cls, mats, ragged):
    ids, pw, cams = ragged
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    tr = dense_tracer(tracer_cls, FW, FH)
    tree = tracer_cls(FW, FH).init()
    tr.add_dense(ids, RAGGED_ORIGIN, mats); tree.add_dense(ids, RAGGED_ORIGIN, mats)
    hits = misses = changed = 0
    try:
        for frame in (5, 11):                                        # frame indices above 0: jitterSequence[frame mod 16]
            j = W.taa_jitter(frame)
            assert j[0] != 0.0 or j[1] != 0.0
            for k, cam in enumerate(cams):
                plain = tr.draw_frame(cam).reshape(-1)
                tr.set_taa_jitter(j); tree.set_taa_jitter(j)
                O.set_jitter_clip(j, FW, FH)
                ref, ctr = lat.trace_primary(cam, FW, FH, threads=8)
                got = tr.draw_frame(cam).reshape(-1)
                assert records_equal(got, ref).all(), (frame, k)
                assert records_equal(got, tree.draw_frame(cam).reshape(-1)).all(), (frame, k)
                rect = (FW - 50, FH - 30, 50, 30)
                assert np.array_equal(device_frame(tr, cam, rect, False, True)[1], tree.shade_rgba8(cam, rect).reshape(-1)), (frame, k)
                changed += int((~records_equal(got, plain)).sum())
                hits += int(ctr["hits"]); misses += int(ctr["rays"] - ctr["hits"])
                tr.set_taa_jitter(None); tree.set_taa_jitter(None)
                O.set_jitter_clip(None)
                assert records_equal(tr.draw_frame(cam).reshape(-1), plain).all()
    finally:
        O.set_jitter_clip(None)
    tr.shutdown(); tree.shutdown()
    print(f"jitter: oracle hits {hits}, misses {misses}, records the jitter changed {changed}")
    assert changed >= 50000 and hits >= 50000 and misses >= 90000, (hits, misses, changed)


def test_lifetime_of_the_kept_grid(tracer_cls, mats, ragged):
    """After every step a dense-DDA context's frames equal a fresh tree-kernel context holding the same final world (and the oracle's)."""
    import torch
    ids1, pw1, cams = ragged
    rng = np.random.default_rng(77)
    ids2 = np.where(rng.random((19, 40, 26)) < 0.1, rng.integers(1, 300, size=(19, 40, 26)), 0).astype(np.uint32)
    origin2 = (-3, -11, 2)
    ids3 = np.where(rng.random((30, 30, 30)) < 0.05, rng.integers(1, 300, size=(30, 30, 30)), 0).astype(np.uint32)
    origin3 = (4, 0, -6)
    pw3 = oracle_world(ids3, origin3)
    ids4 = np.where(rng.random((24, 16, 40)) < 0.2, rng.integers(1, 300, size=(24, 16, 40)), 0).astype(np.uint32)
    origin4 = (-8, 8, 0)
    totals = [0, 0]

    def fresh_tree(load):
        t = tracer_cls(FW, FH).init()
        load(t)
        frames = [t.draw_frame(c).reshape(-1).copy() for c in cams]
        t.shutdown()
        return frames

    def same(tr, frames, ids, origin, step):
        pw = oracle_world(ids, origin)
        lat = O.Lattice(pw.nodes, pw.sub_chunks)
        for k, c in enumerate(cams):
            got = tr.draw_frame(c).reshape(-1)
            assert records_equal(got, frames[k]).all(), (step, k)
            ref, ctr = lat.trace_primary(c, FW, FH, threads=8)
            assert records_equal(got, ref).all(), (step, k)
            totals[0] += int(ctr["hits"]); totals[1] += int(ctr["rays"] - ctr["hits"])

    f1 = fresh_tree(lambda t: t.add_dense(ids1, RAGGED_ORIGIN, mats))
    f2 = fresh_tree(lambda t: t.add_dense(ids2, origin2, mats))
    f3 = fresh_tree(lambda t: t.add_world(pw3))
    f4 = fresh_tree(lambda t: t.add_dense(ids4, origin4, mats))
    tr = tracer_cls(FW, FH).init()
    tr.add_dense(ids1, RAGGED_ORIGIN, mats)
    tr.set_dense_dda(True)                                           # enabled only after the upload: no grid was kept, the tree kernel serves
    same(tr, f1, ids1, RAGGED_ORIGIN, "enabled after the upload")
    tr.add_dense(ids1, RAGGED_ORIGIN, mats)                          # now the grid is kept
    same(tr, f1, ids1, RAGGED_ORIGIN, "dense")
    tr.set_dense_dda(False)
    same(tr, f1, ids1, RAGGED_ORIGIN, "toggled off")
    tr.set_dense_dda(True)
    same(tr, f1, ids1, RAGGED_ORIGIN, "toggled on again")
    tr.add_dense(ids2, origin2, mats)
    same(tr, f2, ids2, origin2, "second upload_dense of another shape and origin")
    tr.add_world(pw3)
    same(tr, f3, ids3, origin3, "upload_world after upload_dense")
    tr.add_dense(ids1, RAGGED_ORIGIN, mats)
    same(tr, f1, ids1, RAGGED_ORIGIN, "upload_dense again")
    nz, ny, nx = ids4.shape
    tr.volume_create(origin4, (nx, ny, nz), 128, 1.0)
    tr.volume_upload((ids4 != 0).astype(np.float32), ids4)
    tr.volume_rebuild(mats)
    same(tr, f4, ids4, origin4, "volume_create + volume_rebuild after upload_dense")
    tr.volume_destroy()
    tr.set_host_build(True)                                          # blok_hip_debug.h: the host-build fallback of upload_dense, which keeps the grid too
    tr.add_dense(ids2, origin2, mats)
    assert not tr.built_on_device()
    same(tr, f2, ids2, origin2, "host-build fallback")
    tr.set_host_build(False)
    tr.add_dense(ids1, RAGGED_ORIGIN, mats)
    assert tr.built_on_device()
    # the same frame on two streams at once
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    h1 = torch.zeros((FW * FH, 4), dtype=torch.int32, device="cuda"); h2 = torch.zeros_like(h1)
    torch.cuda.synchronize()
    for _ in range(4):
        tr.draw_frame_device(cams[0], h1.data_ptr(), 0, stream=s1.cuda_stream)
        tr.draw_frame_device(cams[0], h2.data_ptr(), 0, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(h1, h2) and records_equal(h1.cpu().numpy(), f1[0]).all()
    tr.release_stream(s1.cuda_stream); tr.release_stream(s2.cuda_stream)
    tr.set_timing(True)
    same(tr, f1, ids1, RAGGED_ORIGIN, "timing on")
    assert tr.last_kernel_ms() > 0.0
    tr.set_timing(False)
    tr.shutdown()
    print(f"lifetime: oracle hits {totals[0]}, misses {totals[1]}")
    assert totals[0] >= 250000 and totals[1] >= 480000, totals


def test_determinism(tracer_cls, mats, ragged):
    ids, pw, cams = ragged
    tr = dense_tracer(tracer_cls, FW, FH)
    tr.add_dense(ids, RAGGED_ORIGIN, mats)
    for cam in cams:
        a_hits, a_rgba = device_frame(tr, cam, (0, 0, FW, FH), True, True)
        b_hits, b_rgba = device_frame(tr, cam, (0, 0, FW, FH), True, True)
        assert a_hits.tobytes() == b_hits.tobytes() and a_rgba.tobytes() == b_rgba.tobytes()
        assert tr.draw_frame(cam).tobytes() == tr.draw_frame(cam).tobytes() == a_hits.tobytes()
        flags = a_hits.view(np.uint8).reshape(-1, 16)[:, 15]
        assert (flags == 1).sum() > 500 and (flags == 0).sum() > 2000                # frames with something in them (the oracle: 887 hits at least, 4965 misses)
    tr.shutdown()
