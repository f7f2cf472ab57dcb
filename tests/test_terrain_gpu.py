"""GPU: blok_hip_volume_generate_terrain against the host build of the same function (blok_terrain_eval), bit for bit on the volume's
arrays, and the bookkeeping it leaves for the rebuild, the tracer and the shadow rays' sun map."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from blok_amd import terrain as T
from blok_amd._ffi import BlokError
from tests.terrain_cases import params, prior

pytestmark = pytest.mark.gpu

BLOK_ERR_INVALID_ARG, BLOK_ERR_NO_WORLD, BLOK_ERR_UNSUPPORTED = -1, -4, -5
ALL_FLAGS = [0, 1, 3, 4, 5, 7]


def _tracer():
    from blok_amd.tracer import HipTracer
    return HipTracer(64, 64).init()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_region(t, p, origin, shape, lo, hi, d0, m0):
    """generate over [lo, hi) on top of (d0, m0): equals the host evaluation inside, the prior content outside."""
    t.volume_upload(d0, m0)
    n = t.volume_generate_terrain(p, lo, hi)
    d, m = t.volume_download()
    sl = tuple(slice(lo[a] - origin[a], hi[a] - origin[a]) for a in (2, 1, 0))
    ed, em, en = T.eval_box(p, lo, hi, d0[sl], m0[sl])
    rd, rm = d0.copy(), m0.copy()
    rd[sl], rm[sl] = ed, em
    assert _bits_equal(d, rd) and np.array_equal(m, rm) and n == en
    return d, m


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_whole_box_and_interior_region_equal_the_host(keyed, flags):
    t = _tracer()
    t.set_volume_layout(keyed)
    origin, shape = (-40, -44, -24), (96, 80, 64)
    p, _ = params(flags=flags)
    t.volume_create(origin, shape)
    d0, m0 = prior(shape[::-1])
    hi = tuple(o + s for o, s in zip(origin, shape))
    t.volume_upload(d0, m0)
    n = t.volume_generate_terrain(p)                               # both NULL: the whole box
    d, m = t.volume_download()
    ed, em, en = T.eval_box(p, origin, hi, d0, m0)
    assert _bits_equal(d, ed) and np.array_equal(m, em) and n == en
    _check_region(t, p, origin, shape, (-31, -39, -13), (38, 21, 30), d0, m0)      # ragged, unaligned in x
    _check_region(t, p, origin, shape, (-8, -20, 0), (24, 4, 1), d0, m0)
    t.shutdown()


def test_prior_content_from_set_voxels_and_a_voxelized_mesh_is_kept():
    from tests import voxelize_meshes as M
    t = _tracer()
    origin, shape = (-32, -40, -32), (64, 64, 64)
    t.volume_create(origin, shape)
    rng = np.random.default_rng(2)
    xyz = (rng.integers(0, 64, (500, 3)) + np.array(origin)).astype(np.int32)
    t.volume_set_voxels(xyz, rng.integers(9, 20, 500).astype(np.uint32), np.full(500, 0.75, np.float32))
    pos, tri = M.icosphere([0.0, 10.0, 0.0], 9.0, 3)
    assert t.volume_voxelize_mesh(pos, tri, material=21, solid=True) > 0
    d0, m0 = t.volume_download()
    for flags in (0, 4, 5):
        p, _ = params(flags=flags)
        _check_region(t, p, origin, shape, (-20, -30, -20), (20, 20, 20), d0, m0)
    t.shutdown()


@pytest.mark.parametrize("kw", [dict(cave_octaves=0), dict(cave_octaves=4, cave_cell_log2=3), dict(height_cell_log2=0, height_octaves=1, cave_cell_log2=1, ore_cell_log2=0),
                                dict(height_octaves=8, height_cell_log2=9, cave_roof=0, soil_depth=0)])
def test_ragged_box_at_a_negative_origin(kw):
    t = _tracer()
    origin, shape = (-211, -50, -97), (200, 72, 136)
    t.volume_create(origin, shape)
    hi = tuple(o + s for o, s in zip(origin, shape))
    for flags in (0, 3):
        p, _ = params(flags=flags, **kw)
        n = t.volume_generate_terrain(p)
        d, m = t.volume_download()
        ed, em, en = T.eval_box(p, origin, hi)
        assert _bits_equal(d, ed) and np.array_equal(m, em) and n == en
    t.shutdown()


def test_box_whose_rows_are_no_multiple_of_four():
    t = _tracer()
    origin, shape = (-37, -30, -11), (83, 61, 67)
    t.volume_create(origin, shape)
    d0, m0 = prior(shape[::-1])
    for flags in ALL_FLAGS:
        p, _ = params(flags=flags)
        _check_region(t, p, origin, shape, origin, tuple(o + s for o, s in zip(origin, shape)), d0, m0)
        _check_region(t, p, origin, shape, (-30, -25, -5), (41, 30, 50), d0, m0)
    t.shutdown()


def test_512_cubed_whole_box():
    t = _tracer()
    n = 512
    p = T.default_params(n, 0xB10C0001)
    t.volume_create((0, 0, 0), (n, n, n))
    written = t.volume_generate_terrain(p)
    d, m = t.volume_download()
    slabs = [(z, min(z + 16, n)) for z in range(0, n, 16)]                 # the host side in slabs of z, a few at a time
    with ThreadPoolExecutor(max_workers=8) as pool:
        parts = list(pool.map(lambda s: T.eval_box(p, (0, 0, s[0]), (n, n, s[1])), slabs))
    total = 0
    for (z0, z1), (ed, em, en) in zip(slabs, parts):
        assert _bits_equal(d[z0:z1], ed) and np.array_equal(m[z0:z1], em)
        total += en
    assert written == total and total > n ** 3 // 8
    t.shutdown()


def test_rebuild_equals_a_fresh_upload():
    """Masks, occupancy words and dirty flags as an upload of the same arrays leaves them: the same tree, also after a brush on top."""
    for flags in (0, 3, 4):
        a, b = _tracer(), _tracer()
        origin, shape = (-45, -38, -40), (90, 70, 80)
        d0, m0 = prior(shape[::-1], 4)
        for t in (a, b):
            t.volume_create(origin, shape)
            t.volume_upload(d0, m0)
            t.volume_rebuild()
        p, _ = params(flags=flags)
        a.volume_generate_terrain(p, (-40, -30, -33), (37, 25, 31))
        d, m = a.volume_download()
        b.volume_upload(d, m)
        for step in range(2):
            sa, sb = a.volume_rebuild(), b.volume_rebuild()
            assert (sa.n_voxels, sa.n_tree_nodes) == (sb.n_voxels, sb.n_tree_nodes)
            assert step or sa.n_voxels == int((d > 0).sum())
            na, ma = a.download_tree()
            nb, mb = b.download_tree()
            assert np.array_equal(na, nb) and np.array_equal(ma, mb)
            for t in (a, b):
                t.volume_apply_brush((0.0, -5.0, 0.0), 9.0, 1.0, 0 if step == 0 else 1)
        a.shutdown()
        b.shutdown()


def _world_voxels(d, m, origin):
    z, y, x = np.nonzero(d > 0)
    return np.stack([x + origin[0], y + origin[1], z + origin[2]], 1).astype(np.int32), m[z, y, x]


def test_shell_frames_equal_solid_frames_and_the_oracle():
    """Every ray that starts in air meets a shell voxel first: the SHELL | CLOSE_SIDES world traces like the solid one."""
    from blok_amd import world as W
    from tests import oracle_ffi as O
    from tests.conftest import records_equal
    w, h = 160, 120
    origin, shape = (-48, -40, -48), (96, 80, 96)
    top = origin[1] + shape[1]
    p0, d = params(flags=0)
    p3, _ = params(flags=3)
    assert origin[1] <= d["base_height"] and d["base_height"] + d["amplitude"] <= top        # no column is cut off by the box's top
    eyes = [((90.0, 70.0, -80.0), (0.0, 0.0, 0.0)), ((-70.0, 45.0, 100.0), (5.0, -10.0, 5.0)), ((3.5, 36.5, 2.5), (30.0, 0.0, 20.0))]
    solid_d, solid_m, _ = T.eval_box(p0, origin, tuple(o + s for o, s in zip(origin, shape)))
    for eye, _ in eyes:
        assert eye[1] >= origin[1]                                                         # not below the (open) floor
        v = [int(np.floor(c)) - o for c, o in zip(eye, origin)]
        inside = all(0 <= v[a] < shape[a] for a in range(3))
        assert not inside or solid_m[v[2], v[1], v[0]] == 0                                # the camera's own voxel is empty
    frames = {}
    for name, p in (("solid", p0), ("shell", p3)):
        t = _tracer()
        t.resize(w, h)
        t.volume_create(origin, shape)
        t.volume_generate_terrain(p)
        t.volume_rebuild(W.scene_materials())
        dd, mm = t.volume_download()
        xyz, ids = _world_voxels(dd, mm, origin)
        ow = O.OracleWorld(128, 1.0)
        ow.set_voxels(xyz, ids)
        ow.rebuild()
        lat = O.Lattice(*ow.pack())
        frames[name] = []
        for eye, at in eyes:
            cam = W.camera_look_at(eye, at, 60.0, w, h)
            got = t.draw_frame(cam).reshape(-1)
            ref, ctr = lat.trace(O.primary_rays(cam, w, h), threads=8)
            assert ctr["hits"] > 1000 and records_equal(got, ref).all()
            frames[name].append(got)
        t.shutdown()
    for a, b in zip(frames["solid"], frames["shell"]):
        assert records_equal(a, b).all()


def test_path_traced_frames_with_and_without_the_sun_map():
    """The edited box and its fill bit (gpu_build.h: gpu_volume_commit) reach the shadow rays' last-occluder map, also when a taller terrain replaces the first."""
    from blok_amd import world as W
    w, h = 160, 120
    mats = W.scene_materials()
    t = _tracer()
    t.resize(w, h)
    t.volume_create((0, 0, 0), (64, 96, 64), 128, 1.0)
    cams = [W.scene_camera(64, 0, w, h), W.camera_look_at((5.0, 90.0, 5.0), (40.0, 30.0, 40.0), 70.0, w, h)]

    def same(tag):
        for cam in cams:
            t.set_sun_map(False)
            plain = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            t.set_sun_map(True)
            got = t.trace_paths(cam, spp=3, max_bounces=2, frame_index=4)
            for k in plain:
                assert got[k].tobytes() == plain[k].tobytes(), (tag, k)

    low, _ = params(base_height=8, amplitude=24, flags=0)
    tall, _ = params(base_height=30, amplitude=50, seed=77, flags=0)
    for tag, p in (("low", low), ("tall", tall), ("low again", low)):
        assert t.volume_generate_terrain(p) > 0
        t.volume_rebuild(mats)
        same(tag)
    add, _ = params(base_height=40, amplitude=40, seed=5, flags=5)
    assert t.volume_generate_terrain(add, (10, 0, 10), (40, 96, 40)) > 0
    t.volume_rebuild(mats)
    same("add")
    t.shutdown()


def test_runs_are_bit_identical_and_the_count_is_the_filled_voxels():
    t = _tracer()
    out = []
    for _ in range(2):
        t.volume_create((-64, -64, -64), (128, 128, 128))
        for flags in (0, 3):
            p, _ = params(flags=flags)
            n = t.volume_generate_terrain(p)
            d, m = t.volume_download()
            assert n == int((d > 0).sum()) == int((m != 0).sum())
            out.append((d, m))
    assert all(_bits_equal(out[i][0], out[i + 2][0]) and np.array_equal(out[i][1], out[i + 2][1]) for i in (0, 1))
    t.shutdown()


def test_errors_write_nothing():
    t = _tracer()
    good, _ = params()
    with pytest.raises(BlokError) as e:
        t.volume_generate_terrain(good)
    assert e.value.status == BLOK_ERR_NO_WORLD
    t.volume_create((0, -16, 0), (16, 32, 16))
    d0, m0 = prior((16, 32, 16), 9)
    t.volume_upload(d0, m0)
    for kw in (dict(height_octaves=0), dict(height_octaves=9, height_cell_log2=12), dict(height_cell_log2=13), dict(cave_octaves=5, cave_cell_log2=12),
               dict(cave_octaves=3, cave_cell_log2=1), dict(ore_cell_log2=13), dict(cave_threshold=65537), dict(ore_threshold=65537),
               dict(amplitude=65537), dict(base_height=(1 << 24) + 1), dict(density=0.0), dict(density=float("nan")), dict(density=float("inf")),
               dict(flags=8), dict(flags=2)):
        with pytest.raises(BlokError) as e:
            t.volume_generate_terrain(params(**kw)[0])
        assert e.value.status == BLOK_ERR_INVALID_ARG, kw
    with pytest.raises(BlokError) as e:
        t.volume_generate_terrain(good, (0, 0, 0), None)
    assert e.value.status == BLOK_ERR_INVALID_ARG
    with pytest.raises(BlokError) as e:
        t.volume_generate_terrain(good, (0, 5, 0), (4, 4, 4))
    assert e.value.status == BLOK_ERR_INVALID_ARG
    for lo, hi in (((-1, 0, 0), (4, 4, 4)), ((0, -16, 0), (16, 17, 16))):
        with pytest.raises(BlokError) as e:
            t.volume_generate_terrain(good, lo, hi)
        assert e.value.status == BLOK_ERR_UNSUPPORTED
    assert t._lib.blok_hip_volume_generate_terrain(t._ctx, None, None, None, None) == BLOK_ERR_INVALID_ARG
    assert t.volume_generate_terrain(good, (3, 2, 1), (3, 9, 8)) == 0          # an empty region
    d, m = t.volume_download()
    assert _bits_equal(d, d0) and np.array_equal(m, m0)
    t.shutdown()


def test_headless_driver_renders_terrain_and_a_mesh_on_it(tmp_path):
    import subprocess
    from blok_amd import build as b
    from tests import voxelize_meshes as M
    exe = b.build_tools()
    pos, tri = M.icosphere([0.0, 0.0, 0.0], 1.0, 3)
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 0.9 0.1 0.8\n")
    lines = ["mtllib m.mtl"] + [f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in pos.tolist()] + ["usemtl a"]
    lines += [f"f {a + 1} {b_ + 1} {c + 1}" for a, b_, c in tri.tolist()]
    (tmp_path / "m.obj").write_text("\n".join(lines) + "\n")
    head = b"P6\n320 200\n255\n"

    def render(extra):
        out = tmp_path / "frame.ppm"
        proc = subprocess.run([str(exe), "--terrain", "0xB10C0001", "--terrain-size", "128", "--size", "320x200", "--frames", "2", "--out", str(out), *extra],
                              capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr
        assert "voxels filled" in proc.stdout and "frame 1:" in proc.stdout
        data = out.read_bytes()
        assert data.startswith(head) and len(data) == len(head) + 320 * 200 * 3
        return proc.stdout, np.frombuffer(data[len(head):], np.uint8).reshape(200, 320, 3)

    for extra in ([], ["--obj", str(tmp_path / "m.obj"), "--solid"]):
        stdout, img = render(extra)                                   # first-hit frame: flat material colours over one sky colour
        colours, counts = np.unique(img.reshape(-1, 3), axis=0, return_counts=True)
        sky = img[0, 0]
        is_sky = (img == sky).all(axis=2)
        assert is_sky[0].all()                                        # the top row is sky,
        assert not is_sky[-40:].any()                                 # the bottom rows are ground,
        assert 0.05 < is_sky.mean() < 0.8 and len(colours) >= 3        # and the horizon lies between them
        ground = img[~is_sky].astype(int)
        assert (ground[:, 1] > ground[:, 0] + 30).mean() > 0.3         # mostly grass
        if extra:
            assert "voxels written on the ground" in stdout
            assert ((ground[:, 0] > ground[:, 1] + 60) & (ground[:, 2] > ground[:, 1] + 60)).sum() > 100      # the magenta mesh stands in view
        _, rt = render(extra + ["--rt", "--spp", "2"])
        assert len(np.unique(rt.reshape(-1, 3), axis=0)) > 200         # shaded, filtered colours
