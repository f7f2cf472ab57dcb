"""GPU: the lit path loop over placed lattice instances whose models carry light tables (include/blok_hip.h, "emissive models as lights";
DESIGN.md §33; path_core.h: shade_pixel<…, kLit, kPlacedLit>).

Exact: installing and clearing a model table restores every entry's bytes; a model table that no instance uses, and a table whose instance
lights are disabled, give the world-lit frame's bytes; and with one bounce a frame over lit instances equals, byte for byte in every plane,
the frame of the same instances without model tables under blok_hip_set_lights given the world's table followed by
blok_instance_light_record of every face, instance by instance — with and without a world table."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, LIGHT, POSE
from tests import instance_oracle as IO
from tests import model_lights_cases as MC

pytestmark = pytest.mark.gpu

f32 = np.float32
PLANES = ("color", "world_pos", "normal_roughness", "albedo_metallic")
WD, HT = 64, 48
CAM = ((4.5, 13.0, -7.0), (16.0, 3.0, 16.0))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def scene(world_patch):
    """A 32^3 box: a floor two voxels thick and, with world_patch, a glowing 3 x 3 patch let into it; rebuilt, with the world's light table."""
    from blok_amd.tracer import HipTracer
    t = HipTracer(WD, HT).init()
    d = np.zeros((32, 32, 32), dtype=f32)
    m = np.zeros((32, 32, 32), dtype=np.uint32)
    d[:, 0:2, :], m[:, 0:2, :] = 1.0, MC.GREY
    if world_patch:
        m[20:23, 1, 8:11] = MC.GLOW2
    t.volume_create((0, 0, 0), (32, 32, 32))
    t.volume_upload(d, m)
    t.volume_rebuild(MC.materials())
    if world_patch:
        t.volume_extract_quads()
        assert int(LT.from_quads(t)["n_faces"][0]) == 9
    return t


def lanterns(t):
    """Two lantern models (3^3, all glowing), the second at exponent 1, and three instances in different orientations over the floor."""
    cube = MC.cube(3)
    glow = np.full(len(cube), MC.GLOW, dtype=np.uint32)
    small, big = t.model_create(cube, glow), t.model_create(cube, glow)
    t.model_set_scale(big, 1)
    inst = np.array([IO.instance(small, (8, 6, 12)), IO.instance(small, (20, 9, 18), (2, 0, 1), 5), IO.instance(big, (18, 4, 6), (1, 0, 2), 2)], dtype=INSTANCE)
    t.check_instances(inst)
    return small, big, inst


def same_planes(a, b, what, keys=PLANES):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float((a[k] != b[k]).any(-1).mean()))


def twin_table(t, inst, models):
    """[the world's table ..., then instance_light_record of every face, instance by instance], cum run again."""
    parts = [LT.download(t)]
    for rec in inst:
        e = t.model_scale(int(rec["model"]))
        parts.append(np.array([LT.instance_light_record(rec, e, face) for face in models[int(rec["model"])]], dtype=LIGHT))
    table = np.concatenate(parts)
    area = table["du"].astype(np.int64) * table["dv"]
    table["cum"] = np.concatenate([[0], np.cumsum(area)[:-1]])
    return table, int(area.sum())


@pytest.mark.parametrize("world_patch", [True, False], ids=["a world table", "no world table"])
def test_one_bounce_frame_equals_the_set_lights_twin(torch_cuda, world_patch):
    t = scene(world_patch)
    small, big, inst = lanterns(t)
    cam = W.camera_look_at(*CAM, 60.0, WD, HT)
    unlit = t.trace_paths_instanced(cam, inst, 2, 1, frame_index=3)
    for m in (small, big):
        assert int(LT.model_lights(t, m)["n"][0]) == 54
    header, icum = LT.instance_lights_info(t, inst)
    assert icum.tolist() == [0, 54, 108, 108 + 54 * 4] and int(header["a_total"][0]) == (9 if world_patch else 0) + 324
    lit = t.trace_paths_instanced(cam, inst, 2, 1, frame_index=3)
    posed_entry = t.trace_paths_posed(cam, inst, np.zeros(0, dtype=POSE), 2, 1, frame_index=3)
    models = {small: LT.model_lights_download(t, small), big: LT.model_lights_download(t, big)}
    world_table = LT.download(t)
    table, faces = twin_table(t, inst, models)
    assert faces == int(header["a_total"][0])
    for m in (small, big):
        LT.model_lights_clear(t, m)
    LT.set(t, table)
    twin = t.trace_paths_instanced(cam, inst, 2, 1, frame_index=3)
    same_planes(lit, twin, "the twin")
    same_planes(lit, posed_entry, "the posed entry with an empty pose table")
    assert lit["ids"].tobytes() == twin["ids"].tobytes() == unlit["ids"].tobytes()
    assert (lit["color"] != unlit["color"]).any()
    floor = unlit["world_pos"][..., 1] == f32(2.0)
    assert lit["color"][floor][:, :3].sum() > unlit["color"][floor][:, :3].sum()      # the lanterns light the floor
    # with the model tables gone and the world's own table back, the frame is the world-lit (or unlit) one again
    LT.set(t, world_table if len(world_table) else None)
    back = t.trace_paths_instanced(cam, inst, 2, 1, frame_index=3)
    same_planes(back, unlit, "cleared")
    t.shutdown()


def test_install_and_clear_restore_every_entry_and_tables_without_light_change_nothing(torch_cuda):
    t = scene(True)
    small, big, inst = lanterns(t)
    cam = W.camera_look_at(*CAM, 60.0, WD, HT)
    none_p = np.zeros(0, dtype=POSE)

    def entries(table):
        out = {"instanced": t.trace_paths_instanced(cam, table, 2, 2, frame_index=5), "posed": t.trace_paths_posed(cam, table, none_p, 2, 2, frame_index=5)}
        t.post_reset()
        out["chain"] = [t.draw_frame_rt_instanced(cam, table, 2, 2)[0] for _ in range(2)]
        t.post_reset()
        out["motion"] = [t.draw_frame_rt_instanced_motion(cam, table, 2, 2)[0] for _ in range(2)]
        t.post_reset()
        return out

    def same_entries(a, b, what):
        for k in ("instanced", "posed"):
            same_planes(a[k], b[k], (what, k))
            assert a[k]["ids"].tobytes() == b[k]["ids"].tobytes()
        for k in ("chain", "motion"):
            for x, y in zip(a[k], b[k]):
                assert x.tobytes() == y.tobytes(), (what, k)

    before = entries(inst)
    LT.model_lights(t, small)
    LT.model_lights(t, big)
    lit = entries(inst)
    assert (lit["instanced"]["color"] != before["instanced"]["color"]).any()
    LT.model_lights_clear(t, small)
    LT.model_lights_clear(t, big)
    same_entries(entries(inst), before, "cleared")
    # a model table, but no instance of that model: the world-lit frame
    other = t.model_create(MC.cube(2), np.full(8, MC.GLOW, dtype=np.uint32))
    assert int(LT.model_lights(t, other)["n"][0]) == 24
    header, _ = LT.instance_lights_info(t, inst)
    assert int(header["a_inst"][0]) == 0 and int(header["a_total"][0]) == 9
    same_entries(entries(inst), before, "no instance of the lit model")
    # the disabled case: a lantern of exponent 8 placed 1214 times beside the three (all of them far outside the view) carries no light
    LT.model_lights(t, small)
    LT.model_lights(t, big)
    huge = t.model_create(MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32))
    t.model_set_scale(huge, 8)
    LT.model_lights(t, huge)
    far = np.zeros(1214, dtype=INSTANCE)
    far["model"], far["axis"], far["offset"] = huge, (0, 1, 2), (-30000, -30000, -30000)
    crowd = np.concatenate([inst, far])
    header, icum = LT.instance_lights_info(t, crowd)
    assert int(header["disabled"][0]) == 1 and not icum.any()
    LT.model_lights_clear(t, small); LT.model_lights_clear(t, big); LT.model_lights_clear(t, huge); LT.model_lights_clear(t, other)
    plain = t.trace_paths_instanced(cam, crowd, 2, 2, frame_index=5)
    LT.model_lights(t, small); LT.model_lights(t, big); LT.model_lights(t, huge)
    disabled = t.trace_paths_instanced(cam, crowd, 2, 2, frame_index=5)
    same_planes(disabled, plain, "disabled")
    t.shutdown()


def test_three_bounces_never_brighter_than_the_twin_and_darker_somewhere(torch_cuda):
    """The same seeds draw the same paths in both frames (rule (e) changes what a hit adds, never a draw): where a diffuse bounce ray finds a
    lit lantern the twin adds its emission a second time and this loop does not, so no pixel or channel is brighter and some are darker."""
    t = scene(True)
    small, big, inst = lanterns(t)
    cam = W.camera_look_at(*CAM, 60.0, WD, HT)
    LT.model_lights(t, small)
    LT.model_lights(t, big)
    lit = t.trace_paths_instanced(cam, inst, 4, 3, frame_index=7)
    models = {small: LT.model_lights_download(t, small), big: LT.model_lights_download(t, big)}
    table, _ = twin_table(t, inst, models)
    LT.model_lights_clear(t, small)
    LT.model_lights_clear(t, big)
    LT.set(t, table)
    twin = t.trace_paths_instanced(cam, inst, 4, 3, frame_index=7)
    same_planes(lit, twin, "the G-buffer", PLANES[1:])
    darker = lit["color"][..., :3] < twin["color"][..., :3]
    print(f"darker in {int(darker.any(-1).sum())} of {WD * HT} pixels; sums {lit['color'][..., :3].sum():.6g} against {twin['color'][..., :3].sum():.6g}")
    assert (lit["color"][..., :3] <= twin["color"][..., :3]).all() and darker.any(-1).sum() > 20
    t.shutdown()


def test_lantern_loop_has_the_hit_counting_loops_expectation_and_less_variance(torch_cuda):
    """A closed 24^3 grey room with no world emitter; a 3^3 glowing lantern hangs as an instance under the ceiling; the camera looks at the
    floor.  32 x 24 pixels, three bounces, 64 spp, K = 16 frames with the model table and 16 without.  The rule of the world table's test:
    |mean(m_lit) - mean(m_unlit)| <= 4 sqrt(var(m_lit) / K + var(m_unlit) / K), that bound below 10 % of mean(m_unlit), var(m_lit) < var(m_unlit)."""
    from blok_amd.tracer import HipTracer
    w, h, K, spp = 32, 24, 16, 64
    t = HipTracer(w, h).init()
    d = np.ones((24, 24, 24), dtype=f32)
    m = np.full((24, 24, 24), MC.GREY, dtype=np.uint32)
    d[1:23, 1:22, 1:23] = 0.0
    t.volume_create((0, 0, 0), (24, 24, 24))
    t.volume_upload(d, m)
    t.volume_rebuild(MC.materials())
    lantern = t.model_create(MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32))
    inst = np.array([IO.instance(lantern, (10, 18, 11))], dtype=INSTANCE)
    cam = W.camera_look_at((12.0, 14.0, 4.0), (12.0, 1.0, 13.0), 70.0, w, h)
    hits = t.draw_frame(cam)
    floor = (hits["hit"] == 1) & (hits["face"] == 2) & (hits["voxel"][..., 1] == 0)
    assert floor.sum() > 300
    unlit = [t.trace_paths_instanced(cam, inst, spp, 3, frame_index=k)["color"][..., :3][floor].astype(np.float64).mean() for k in range(K)]
    assert int(LT.model_lights(t, lantern)["n"][0]) == 54
    lit = [t.trace_paths_instanced(cam, inst, spp, 3, frame_index=k)["color"][..., :3][floor].astype(np.float64).mean() for k in range(K)]
    m_lit, m_unlit = np.array(lit), np.array(unlit)
    bound = 4.0 * np.sqrt(m_lit.var(ddof=1) / K + m_unlit.var(ddof=1) / K)
    print(f"spp {spp}, K {K}: mean lit {m_lit.mean():.6g} unlit {m_unlit.mean():.6g} difference {abs(m_lit.mean() - m_unlit.mean()):.3g} bound {bound:.3g} "
          f"({100.0 * bound / m_unlit.mean():.2f} % of the unlit mean); var lit {m_lit.var(ddof=1):.3g} unlit {m_unlit.var(ddof=1):.3g}")
    assert m_unlit.mean() > 0 and bound < 0.10 * m_unlit.mean()
    assert abs(m_lit.mean() - m_unlit.mean()) <= bound
    assert m_lit.var(ddof=1) < m_unlit.var(ddof=1)
    t.shutdown()


@pytest.mark.parametrize("world_patch", [False, True], ids=["no world table", "a world table"])
def test_model_tables_that_carry_no_light_give_the_frame_taken_with_no_table(torch_cuda, world_patch):
    """With model tables installed but A_inst = 0 the placed lit kernel runs all the same.  With A_world = 0 too (no world table) its frame
    must be the unlit entry's, the one taken before any table existed; with a world table the world-lit one.  Two ways to A_inst = 0: a lit
    model that no instance uses, and the disabled crowd."""
    t = scene(world_patch)
    small, big, inst = lanterns(t)
    cam = W.camera_look_at(*CAM, 60.0, WD, HT)
    huge = t.model_create(MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32))
    t.model_set_scale(huge, 8)
    other = t.model_create(MC.cube(2), np.full(8, MC.GLOW, dtype=np.uint32))
    far = np.zeros(1214, dtype=INSTANCE)
    far["model"], far["axis"], far["offset"] = huge, (0, 1, 2), (-30000, -30000, -30000)
    crowd = np.concatenate([inst, far])
    a_world = 9 if world_patch else 0
    no_table = {"three": t.trace_paths_instanced(cam, inst, 2, 3, frame_index=5), "crowd": t.trace_paths_instanced(cam, crowd, 2, 3, frame_index=5)}
    assert int(LT.model_lights(t, other)["n"][0]) == 24
    header, icum = LT.instance_lights_info(t, inst)
    assert (int(header["a_inst"][0]), int(header["a_total"][0]), int(header["disabled"][0])) == (0, a_world, 0) and not icum.any()
    unused = t.trace_paths_instanced(cam, inst, 2, 3, frame_index=5)
    same_planes(unused, no_table["three"], "a lit model that no instance uses")
    assert unused["ids"].tobytes() == no_table["three"]["ids"].tobytes()
    for m in (small, big, huge):
        LT.model_lights(t, m)
    header, icum = LT.instance_lights_info(t, crowd)
    assert (int(header["a_inst"][0]), int(header["a_total"][0]), int(header["disabled"][0])) == (0, a_world, 1) and not icum.any()
    disabled = t.trace_paths_instanced(cam, crowd, 2, 3, frame_index=5)
    same_planes(disabled, no_table["crowd"], "disabled")
    assert disabled["ids"].tobytes() == no_table["crowd"]["ids"].tobytes()
    t.shutdown()


def test_gpu_frame_against_the_host_shim(torch_cuda, tmp_path):
    """(4 spp, 2 bounces), a world table and the three lanterns; the rule of tests/test_lit_paths_gpu.py::test_gpu_frame_against_the_host_shim:
    the first hit exact, every pixel's colour within 1e-4 + 1e-3 |ref|, the mean absolute difference below 2e-4."""
    from tests import test_model_lights_paths_cpu as CPU
    t = scene(True)
    small, big, inst = lanterns(t)
    cam = W.camera_look_at(*CAM, 60.0, WD, HT)
    LT.model_lights(t, small)
    LT.model_lights(t, big)
    got = t.trace_paths_instanced(cam, inst, 4, 2, frame_index=5)
    shim = CPU.PlacedShim(tmp_path / "libmodel_lights_paths_shim.so")
    d, m, world_table = CPU.world_scene(True)
    assert world_table[["lo", "du", "dv", "material", "face"]].tobytes() == LT.download(t)[["lo", "du", "dv", "material", "face"]].tobytes()
    cube, glow = MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32)
    lantern = LT.model_lights_download(t, small)
    ref = shim.render_placed(shim.tree(*CPU.voxels_of(d, m)), [shim.tree(cube, glow), shim.tree(cube, glow, 1)], inst, cam, MC.materials(), WD, HT, 4, 2, 5,
                             table=world_table, model_tables=[lantern, lantern])
    header, icum = LT.instance_lights_info(t, inst)
    assert ref["icum"].tobytes() == icum.tobytes() and ref["header"].tobytes() == header.tobytes()
    for k in PLANES[1:] + ("ids",):
        assert np.array_equal(got[k], ref[k]), k
    err = np.abs(got["color"] - ref["color"])
    ok = (err <= 1e-4 + 1e-3 * np.abs(ref["color"])).all(axis=2)
    print(f"(4, 2): {int((~ok).sum())} pixels outside the tolerance, mean |difference| {float(err.mean()):.3g}, lantern pixels {int((got['ids'] != 0xFFFFFFFF).sum())}")
    assert ok.all(), np.argwhere(~ok)[:8].tolist()
    assert err.mean() < 2e-4
    assert (got["ids"] != 0xFFFFFFFF).sum() > 50
    t.shutdown()


def test_the_lit_floor_follows_a_moving_lantern_through_the_motion_chain(torch_cuda):
    """No world emitter.  One lantern, 4 voxels over the floor, moves 3 voxels per frame along x through draw_frame_rt_instanced_motion, six
    frames.  In the last frame the floor under the lantern's new position is brighter than the floor under the position it started from, 15
    voxels away (floor pixels within 4 voxels of the lantern's centre in x and z, the lantern's own pixels left out); without the model table
    the two regions are lit by hits alone.  The lantern's own pixels show its emission (4, 3, 2), far above the tonemapper's shoulder, plus
    indirect light off a floor of albedo 0.6 that the two estimators form with one expectation: the history on them must have accumulated
    alike with and without the table — the denoiser's history length equal pixel for pixel and above two frames, their mean absolute
    difference below 8 of 255 per channel.  The floor's gain under the new position over the old must also exceed the same difference
    in the chain without a table, which is the sun's gradient alone."""
    t = scene(False)
    lantern = t.model_create(MC.cube(3), np.full(27, MC.GLOW, dtype=np.uint32))
    cam = W.camera_look_at(*CAM, 60.0, WD, HT)
    steps = [np.array([IO.instance(lantern, (6 + 3 * k, 6, 14))], dtype=INSTANCE) for k in range(6)]
    last = t.trace_paths_instanced(cam, steps[-1], 1, 1, frame_index=0)
    wp = last["world_pos"]
    own = last["ids"] == 0
    floor = (wp[..., 1] == f32(2.0)) & ~own

    def under(x):
        return floor & (np.abs(wp[..., 0] - (x + 1.5)) <= 4.0) & (np.abs(wp[..., 2] - 15.5) <= 4.0)

    new, old = under(6 + 15), under(6)
    print(f"floor pixels under the new position {int(new.sum())}, under the old {int(old.sum())}, the lantern's own {int(own.sum())}")
    assert new.sum() > 15 and old.sum() > 15 and own.sum() > 15 and not (new & old).any()

    def luma(frame, sel):
        rgb = np.stack([(frame >> s) & 0xFF for s in (0, 8, 16)], -1).astype(np.float64)
        return rgb[sel]

    frames = {}
    for lit in (False, True):
        if lit:
            assert int(LT.model_lights(t, lantern)["n"][0]) == 54
        t.post_reset()
        for table in steps:
            frame, count = t.draw_frame_rt_instanced_motion(cam, table, 8, 2)
        frames[lit] = (frame, count, t.denoise_state()[2])
    (dark, n_dark, hist_dark), (lit, n_lit, hist_lit) = frames[False], frames[True]
    print(f"with the table: under the new position {luma(lit, new).mean():.2f}, under the old {luma(lit, old).mean():.2f}; without: {luma(dark, new).mean():.2f}, "
          f"{luma(dark, old).mean():.2f}; the lantern's own pixels differ by {np.abs(luma(lit, own) - luma(dark, own)).mean():.2f} of 255")
    assert n_dark == n_lit == len(steps)
    assert luma(lit, new).mean() > luma(lit, old).mean()
    # ... and by more than the sun's own gradient between the two regions, which the chain without a table shows alone
    assert luma(lit, new).mean() - luma(lit, old).mean() > luma(dark, new).mean() - luma(dark, old).mean()
    # the history on the lantern's own pixels: the same length pixel for pixel with and without a table, and longer than one frame (the object
    # motion carries it along)
    print(f"history length on the lantern's own pixels: mean {hist_lit[own].mean():.2f} with the table, {hist_dark[own].mean():.2f} without")
    assert np.array_equal(hist_lit[own], hist_dark[own]) and hist_lit[own].mean() > 2.0
    assert np.abs(luma(lit, own) - luma(dark, own)).mean() < 8.0
    t.shutdown()
