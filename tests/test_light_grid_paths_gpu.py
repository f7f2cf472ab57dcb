"""GPU: the lit path loop under a light grid (include/blok_hip.h, "the light grid"; path_core.h: grid_light_sample,
shade_pixel<…, kGrid>; trace_kernels.hip: path_kernel_lit_grid).  The routing — a grid changes the colour of
every entry family and nothing of the G-buffer, clearing it restores the lit frames' bytes, the three families agree under it — and the
estimator: in two rooms, of which the camera's holds 4 of the table's 404 faces, the grid loop has the global-pick loop's expectation
and less variance; the direct term against a numpy restatement of the rule; the device against the host shim; the motion chain; and
that a launch with lit lattice instances (model light tables) keeps path_kernel_lit_placed and its global pick."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import pose as P
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, POSE
from tests import instance_oracle as IO
from tests import lights_reference as LR
from tests.test_lit_paths_gpu import GLOW, GLOW2, GREY, HT, PLANES, PLATE_CAM, WD, f32, install, plate_scene, same_planes, tracer, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def test_build_then_clear_restores_every_entry_and_the_entries_agree_under_a_grid(torch_cuda):
    t = tracer()
    d, m = plate_scene()
    d[2:6, 2, 2:6] = 1.0                               # a second light far from the plate: cells that list one, the other, both or none
    m[2:6, 2, 2:6] = GLOW2
    install(t, d, m)
    cam = W.camera_look_at(*PLATE_CAM, 60.0, WD, HT)
    cube = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    model = t.model_create(cube, np.full(len(cube), GREY, dtype=np.uint32))
    inst = np.array([IO.instance(model, (10, 4, 12))], dtype=INSTANCE)
    pose = P.rotation(model, 0.5, 0.3, 0.0, 1.0, (1.5, 1.5, 1.5), (20.0, 5.0, 14.0))
    none_i, none_p = np.zeros(0, dtype=INSTANCE), np.zeros(0, dtype=POSE)

    def entries():
        out = {"world": t.trace_paths(cam, 2, 2, frame_index=5), "instanced": t.trace_paths_instanced(cam, inst, 2, 2, frame_index=5),
               "posed": t.trace_paths_posed(cam, inst, pose, 2, 2, frame_index=5)}
        t.post_reset()
        out["chain"] = [t.draw_frame_rt(cam, 2, 2)[0] for _ in range(3)]
        t.post_reset()
        return out

    before = entries()                                 # the lit loop, before any grid existed
    g = LT.build_grid(t, 2, 1, 192)
    assert 0 < int(g["n_nonempty"][0]) < int(g["n_cells"][0])
    grid = entries()
    LT.clear_grid(t)
    after = entries()
    for k in ("world", "instanced", "posed"):
        same_planes(before[k], after[k], k)
        differ = float((grid[k]["color"] != before[k]["color"]).any(-1).mean())
        print(f"{k}: {100.0 * differ:.1f} % of the pixels change colour under the grid")
        assert differ > 0.05, k
        same_planes(grid[k], before[k], k, PLANES[1:])                # the G-buffer is the first hit's either way
        assert np.isfinite(grid[k]["color"]).all()
    assert before["instanced"]["ids"].tobytes() == after["instanced"]["ids"].tobytes() == grid["instanced"]["ids"].tobytes()
    for x, y, z in zip(before["chain"], after["chain"], grid["chain"]):
        assert x.tobytes() == y.tobytes() and x.tobytes() != z.tobytes()
    # under a grid the world-only entry, the instanced entry with no instance and the posed entry with both tables empty are one frame
    LT.build_grid(t, 2, 1, 192)
    a = t.trace_paths(cam, 2, 3, frame_index=1)
    b = t.trace_paths_instanced(cam, none_i, 2, 3, frame_index=1)
    c = t.trace_paths_posed(cam, none_i, none_p, 2, 3, frame_index=1)
    same_planes(a, b, "world / instanced")
    same_planes(a, c, "world / posed")
    # a share of 1/256 and of 255/256 are different frames of the same scene
    LT.build_grid(t, 2, 1, 1)
    e = t.trace_paths(cam, 2, 3, frame_index=1)
    assert (e["color"] != a["color"]).any()
    t.shutdown()


ROOMS_SPP = 64      # the first of 64, 128, ... at which the global loop alone meets the 10 % cap: 6.59 % (DESIGN.md §34 has the search's figures)


def two_rooms():
    """A 128 x 24 x 24 solid volume [z][y][x]; room A hollow over x in [1, 23) with a 2 x 2 GLOW2 patch in its two-thick ceiling, room B over
    x in [97, 119) with a 20 x 20 GLOW ceiling plate."""
    d = np.ones((24, 24, 128), dtype=f32)
    m = np.full((24, 24, 128), GREY, dtype=np.uint32)
    d[1:23, 1:22, 1:23] = 0.0
    d[1:23, 1:22, 97:119] = 0.0
    m[11:13, 22, 11:13] = GLOW2
    m[2:22, 22, 98:118] = GLOW
    return d, m


def rooms_means(t, cam, floor, spp, K):
    return np.array([t.trace_paths(cam, spp, 3, frame_index=k)["color"][..., :3][floor].astype(np.float64).mean() for k in range(K)])


def test_grid_loop_has_the_global_loops_expectation_and_less_variance(torch_cuda):
    """The camera in room A looks at its floor; 32 x 24 pixels, three bounces, K = 16 frames of each loop.  Grid c = 3, R = 2, s = 192:
    room A's cells (x 0..2) list the patch alone, the plate's (x 12..14) reach no further than x 10.  The reference is the global-pick lit
    loop, the grid cleared.  |mean_grid - mean_global| <= 4 sqrt(var_grid / K + var_global / K), that bound below 10 % of mean_global (a
    condition on the reference's own spread: ROOMS_SPP is the first of 64, 128, ... at which the global loop alone meets it), and
    var_grid < var_global."""
    w, h, K = 32, 24, 16
    t = tracer(w, h)
    info = install(t, *two_rooms())
    table = LT.download(t)
    assert int(info["n"][0]) == 2 and sorted((table["du"] * table["dv"]).tolist()) == [4, 400]
    cam = W.camera_look_at((12.0, 14.0, 4.0), (12.0, 1.0, 13.0), 70.0, w, h)
    hits = t.draw_frame(cam)
    floor = (hits["hit"] == 1) & (hits["face"] == 2) & (hits["voxel"][..., 1] == 0)
    assert floor.sum() > 300
    g = LT.build_grid(t, 3, 2, 192)
    start, faces = LT.grid_download(t, 0), LT.grid_download(t, 1)
    lo, dim = g["cell_lo"][0], g["dim"][0]
    room_a = [int(faces[((z - lo[2]) * dim[1] + (y - lo[1])) * dim[0] + (x - lo[0])]) for x in range(3) for y in range(3) for z in range(3)]
    assert set(room_a) == {4}, room_a
    m_grid = rooms_means(t, cam, floor, ROOMS_SPP, K)
    LT.clear_grid(t)
    m_glob = rooms_means(t, cam, floor, ROOMS_SPP, K)
    bound = 4.0 * np.sqrt(m_grid.var(ddof=1) / K + m_glob.var(ddof=1) / K)
    print(f"spp {ROOMS_SPP}: mean grid {m_grid.mean():.6g} global {m_glob.mean():.6g} difference {abs(m_grid.mean() - m_glob.mean()):.3g} bound {bound:.3g} "
          f"({100.0 * bound / m_glob.mean():.2f} % of the global mean); var grid {m_grid.var(ddof=1):.3g} global {m_glob.var(ddof=1):.3g} "
          f"(ratio {m_glob.var(ddof=1) / m_grid.var(ddof=1):.1f})")
    assert m_glob.mean() > 0 and bound < 0.10 * m_glob.mean()
    assert abs(m_grid.mean() - m_glob.mean()) <= bound
    assert m_grid.var(ddof=1) < m_glob.var(ddof=1)
    t.shutdown()


# ---- the direct term, exact rule ------------------------------------------------------------------------------------------------------------------
def two_plates():
    """plate_scene stretched to 96 voxels in x, with a second 4 x 4 plate (GLOW2) at its far end: outside the first plate's reach."""
    d = np.zeros((32, 32, 96), dtype=f32)
    m = np.zeros((32, 32, 96), dtype=np.uint32)
    d[:, 0:2, :] = 1.0
    m[:, 0:2, :] = GREY
    d[14:18, 14, 14:18] = 1.0
    m[14:18, 14, 14:18] = GLOW
    d[14:18, 14, 88:92] = 1.0
    m[14:18, 14, 88:92] = GLOW2
    return d, m


def nee_reference_grid(t, planes, hits, table, grid, mats, vs=1.0, frame=0):
    """tests/test_lit_paths_gpu.py's nee_reference under a grid: the four draws, the strategy, the pick and area_eff by the numpy rule of
    tests/test_light_grid_paths_cpu.py, from the frame's own planes, the table, the grid's downloads and trace_rays' visibility.
    (term where unoccluded, term, skip, occluded, kinds): kinds[y, x] = 1 local, 2 global with inlist, 3 global without, 4 no cell."""
    from tests.test_light_grid_paths_cpu import numpy_grid_sample
    from blok_amd._ffi import RAY
    h, w = hits.shape
    pos = planes["world_pos"][..., :3].astype(f32)
    nrm = planes["normal_roughness"][..., :3].astype(f32)
    mat = mats[LR.material_index(hits["material_id"], len(mats))]
    found = hits["hit"] == 1
    e = mat["emission"].astype(f32)
    glows = ((e[..., 0] + e[..., 1]) + e[..., 2]) > f32(0.01)
    lum = (e[..., 0] * f32(0.2126) + e[..., 1] * f32(0.7152)) + e[..., 2] * f32(0.0722)
    ended = glows & (lum > f32(5.0))
    metallic = ((mat["flags"] >> 24) & 0xFF).astype(f32) / f32(255.0)
    diffuse = mat["albedo"].astype(f32) * (f32(1.0) - metallic)[..., None]
    eligible = found & ~ended & (diffuse.max(-1) > 0)
    py, px = np.meshgrid(np.arange(h, dtype=np.uint32), np.arange(w, dtype=np.uint32), indexing="ij")
    rng = LR.init_rng(px, py, w, frame, 0)
    rng, r = LR.pcg(rng)
    rng, u1 = LR.random_float(rng)
    rng, u2 = LR.random_float(rng)
    rng, mm = LR.pcg(rng)
    term = np.zeros((h, w, 3), dtype=f32)
    kinds = np.zeros((h, w), dtype=np.uint8)
    rays = np.zeros((h, w), dtype=RAY)
    rays["dir"] = (1.0, 0.0, 0.0)
    has_ray = np.zeros((h, w), dtype=bool)
    for y, x in np.argwhere(eligible):
        has, q, le, g, (local, inlist, a_g), (org, dr, dist) = numpy_grid_sample(table, grid, mats, vs, pos[y, x], nrm[y, x], int(r[y, x]), u1[y, x], u2[y, x], int(mm[y, x]))
        kinds[y, x] = 1 if local else (4 if a_g == 0 else (2 if inlist else 3))
        if not has:
            continue
        term[y, x] = ((f32(1.0) * diffuse[y, x]) * np.asarray(le, dtype=f32)) * g
        rays[y, x] = (org, f32(0.001), dr, dist - LR.K_LIGHT_EPS)
        has_ray[y, x] = True
    shadow = t.trace_rays(rays[has_ray])
    occluded = np.zeros((h, w), dtype=bool)
    occluded[has_ray] = shadow["hit"] == 1
    skip = np.zeros((h, w), dtype=bool)
    skip[has_ray] = (shadow["hit"] == 1) & ((shadow["t"] - rays[has_ray]["tmin"] < 1e-3) | (rays[has_ray]["tmax"] - shadow["t"] < 1e-3))
    return np.where(occluded[..., None], f32(0.0), term), term, skip, occluded, kinds


def test_direct_term_under_a_grid_equals_the_numpy_restatement(torch_cuda):
    """64 x 48, 1 spp, 1 bounce: the colour under a grid = float32(unlit + nee_ref) at the existing direct-term test's contract,
    1e-4 + 1e-3 |ref| and at most 1 % of the pixels with a term skipped for nearness.  Both strategies and inlist false occur among the
    floor pixels.  Prints how many pixels are not bit-equal."""
    from tests.test_lit_paths_gpu import materials
    t = tracer()
    install(t, *two_plates())
    table = LT.download(t)
    assert len(table) == 12
    mats = materials()
    cam = W.camera_look_at(*PLATE_CAM, 60.0, WD, HT)
    info = LT.build_grid(t, 3, 1, 192)
    grid = (LT.grid_download(t, 0), LT.grid_download(t, 1), LT.grid_download(t, 2), info)
    lit = t.trace_paths(cam, 1, 1, frame_index=0)
    hits = t.draw_frame(cam)
    LT.clear(t)
    unlit = t.trace_paths(cam, 1, 1, frame_index=0)
    same_planes(lit, unlit, "G-buffer", PLANES[1:])
    nee, unshadowed, skip, occluded, kinds = nee_reference_grid(t, unlit, hits, table, grid, mats)
    nonzero = (unshadowed > 0).any(-1)
    floor = (hits["hit"] == 1) & (unlit["normal_roughness"][..., 1] == 1.0) & (unlit["world_pos"][..., 1] < 2.5)
    counts = {k: int(((kinds == k) & floor).sum()) for k in (1, 2, 3, 4)}
    print(f"floor pixels: local {counts[1]}, global in the list {counts[2]}, global not in the list {counts[3]}, without a list {counts[4]}; "
          f"with a term {int(nonzero.sum())}, occluded {int((occluded & nonzero).sum())}, skipped {int((skip & nonzero).sum())}")
    assert counts[1] > 0 and counts[2] > 0 and counts[3] > 0
    assert (nonzero & floor).sum() > 300
    assert (skip & nonzero).sum() <= 0.01 * nonzero.sum()
    want = (unlit["color"][..., :3] + nee).astype(f32)
    got = lit["color"][..., :3]
    keep = ~skip
    err = np.abs(got.astype(np.float64) - want)
    bound = 1e-4 + 1e-3 * np.abs(want)
    not_bit_equal = int(((got.view(np.uint32) != want.view(np.uint32)).any(-1) & keep).sum())
    print(f"not bit-equal: {not_bit_equal} of {int(keep.sum())} pixels; worst error / bound {float((err / bound)[keep].max()):.3g}")
    assert (err <= bound)[keep].all(), np.argwhere((err > bound).any(-1) & keep)[:6].tolist()
    t.shutdown()


# ---- the device against the host shim ------------------------------------------------------------------------------------------------------------
def test_gpu_frame_under_a_grid_against_the_host_shim(torch_cuda, tmp_path):
    """(4 spp, 2 bounces) on the mixed scene with an instance and a pose, the existing test's figures: first hits exact, colour within
    1e-4 + 1e-3 |ref|, mean difference below 2e-4."""
    from tests import test_light_grid_paths_cpu as GCPU
    from tests import test_lit_paths_cpu as CPU
    spp, bounces = 4, 2
    mats = CPU.materials()
    d, m = CPU.mixed_scene()
    t = tracer()
    install(t, d, m, mats=mats)
    table = LT.download(t)
    info = LT.build_grid(t, 2, 1, 192)
    grid = (LT.grid_download(t, 0), LT.grid_download(t, 1), LT.grid_download(t, 2), info)
    assert 0 < int(info["n_nonempty"][0]) < int(info["n_cells"][0])
    xyz, ids = CPU.mixed_models()
    model = t.model_create(xyz, ids)
    inst = np.array([IO.instance(model, (6, 2, 8))], dtype=INSTANCE)
    pose = P.rotation(model, 0.6, 0.25, 0.1, 1.0, (2.0, 2.0, 2.0), (21.0, 6.0, 12.0))
    cam = W.camera_look_at(*CPU.MIXED_CAM, 60.0, WD, HT)
    got = t.trace_paths_posed(cam, inst, pose, spp, bounces, frame_index=5)
    shim = GCPU.GridShim(tmp_path / "liblight_grid_paths_shim.so")
    world = shim.tree(*CPU.voxels_of(d, m))
    ref = shim.render(world, cam, mats, WD, HT, spp, bounces, 5, table, grid, models=[shim.tree(xyz, ids)], inst=inst, poses=pose)
    for k in PLANES[1:] + ("ids",):
        assert np.array_equal(got[k], ref[k]), k
    err = np.abs(got["color"] - ref["color"])
    ok = (err <= 1e-4 + 1e-3 * np.abs(ref["color"])).all(axis=2)
    print(f"({spp}, {bounces}) under a grid: {int((~ok).sum())} pixels outside the tolerance, mean |difference| {float(err.mean()):.3g}")
    assert ok.all(), np.argwhere(~ok)[:8].tolist()
    assert err.mean() < 2e-4
    t.shutdown()


# ---- the motion chain ----------------------------------------------------------------------------------------------------------------------------
def test_the_motion_chain_runs_under_a_grid(torch_cuda):
    """draw_frame_rt_posed_motion under a grid gives valid frames that differ from the gridless ones; the chain keeps its G-buffer on the
    device, so its planes are compared through trace_paths_posed, the chain's own path launch, at each frame's pose: equal to the gridless."""
    t = tracer()
    d, m = plate_scene()
    install(t, d, m)
    cam = W.camera_look_at(*PLATE_CAM, 60.0, WD, HT)
    cube = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    model = t.model_create(cube, np.full(len(cube), GREY, dtype=np.uint32))
    poses = [P.rotation(model, 0.2 * k, 0.1, 0.0, 1.0, (1.5, 1.5, 1.5), (18.0 + k, 5.0, 14.0)) for k in range(3)]
    frames, planes = {}, {}
    for grid in (True, False):
        if grid:
            LT.build_grid(t, 2, 1, 192)
        else:
            LT.clear_grid(t)
        t.post_reset()
        frames[grid] = [t.draw_frame_rt_posed_motion(cam, None, p, 2, 2)[0] for p in poses]
        planes[grid] = [t.trace_paths_posed(cam, None, p, 2, 2, frame_index=k) for k, p in enumerate(poses)]
    for a, b in zip(frames[True], frames[False]):
        assert a.shape == (HT, WD) and (a >> 24 == 0xFF).all() and a.tobytes() != b.tobytes()
    for a, b in zip(planes[True], planes[False]):
        same_planes(a, b, "G-buffer under a grid", PLANES[1:])
        assert a["ids"].tobytes() == b["ids"].tobytes()
    t.shutdown()


# ---- lit instances keep the global pick ------------------------------------------------------------------------------------------------------------
def test_a_launch_with_lit_instances_does_not_sample_through_the_grid(torch_cuda):
    """There is no grid kernel beside path_kernel_lit_placed: with a model light table and an instance of that model the
    frame under a grid is the frame without one, byte for byte; the same launch without the model's table does change under the grid."""
    t = tracer()
    d, m = plate_scene()
    install(t, d, m)
    cam = W.camera_look_at(*PLATE_CAM, 60.0, WD, HT)
    cube = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    model = t.model_create(cube, np.full(len(cube), GLOW2, dtype=np.uint32))
    inst = np.array([IO.instance(model, (10, 4, 12))], dtype=INSTANCE)
    plain = t.trace_paths_instanced(cam, inst, 2, 2, frame_index=3)
    LT.build_grid(t, 2, 1, 192)
    under = t.trace_paths_instanced(cam, inst, 2, 2, frame_index=3)
    assert (under["color"] != plain["color"]).any()
    assert int(LT.model_lights(t, model)["n"][0]) == 54
    placed_under = t.trace_paths_instanced(cam, inst, 2, 2, frame_index=3)
    LT.clear_grid(t)
    placed = t.trace_paths_instanced(cam, inst, 2, 2, frame_index=3)
    same_planes(placed, placed_under, "placed-lit under a grid")
    assert (placed["color"] != plain["color"]).any()
    t.shutdown()
