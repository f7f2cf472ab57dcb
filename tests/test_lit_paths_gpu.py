"""GPU: the lit path loop (include/blok_hip.h, "emissive voxels as lights"; path_core.h: shade_pixel<…, kLit>).

Exact: a cleared table gives every entry its earlier bytes; the three entry families agree under a table.  The direct term against a numpy
restatement built from the frame's own planes, the first-hit records, the table and blok_hip_trace_rays' visibility.  The estimator's
expectation against the unlit loop's, by the data's own spread.  Shadows of a light through instances and poses."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import pose as P
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, MATERIAL, POSE, RAY
from tests import instance_oracle as IO
from tests import lights_reference as LR

pytestmark = pytest.mark.gpu

f32 = np.float32
PLANES = ("color", "world_pos", "normal_roughness", "albedo_metallic")
WD, HT = 64, 48
GREY, GLOW, GLOW2, DARK = 1, 2, 3, 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def materials():
    m = np.zeros(5, dtype=MATERIAL)
    m["albedo"] = (0.6, 0.6, 0.6)
    m["flags"] = 230 << 16                        # rough, not metallic
    m["ior"] = 1.5
    m["emission"][GLOW] = (4.0, 3.0, 2.0)         # luminance below 5: a first hit on it goes on
    m["emission"][GLOW2] = (1.0, 2.0, 6.0)
    m["albedo"][DARK] = (0.0, 0.0, 0.0)
    return m


def tracer(w=WD, h=HT):
    from blok_amd.tracer import HipTracer
    return HipTracer(w, h).init()


def install(t, d, m, origin=(0, 0, 0), lights=True, mats=None):
    nz, ny, nx = d.shape
    t.volume_create(origin, (nx, ny, nz))
    t.volume_upload(d, m)
    t.volume_rebuild(materials() if mats is None else mats)
    if lights:
        t.volume_extract_quads()
        return LT.from_quads(t)
    return None


def plate_scene():
    """A glowing 4 x 4 plate floating 12 voxels over a floor in a 32^3 world, nothing between."""
    d = np.zeros((32, 32, 32), dtype=f32)
    m = np.zeros((32, 32, 32), dtype=np.uint32)
    d[:, 0:2, :] = 1.0
    m[:, 0:2, :] = GREY
    d[14:18, 14, 14:18] = 1.0
    m[14:18, 14, 14:18] = GLOW
    return d, m


PLATE_CAM = ((4.5, 11.3, -6.2), (17.0, 1.0, 17.0))


def same_planes(a, b, what, keys=PLANES):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float((a[k] != b[k]).any(-1).mean()))


# ---- 2, 3: the routing -----------------------------------------------------------------------------------------------------------------------------
def test_install_then_clear_restores_every_entry_and_the_entries_agree_under_a_table(torch_cuda):
    t = tracer()
    d, m = plate_scene()
    install(t, d, m, lights=False)
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

    before = entries()
    t.volume_extract_quads()
    info = LT.from_quads(t)
    assert int(info["n"][0]) == 6 and int(info["n_faces"][0]) == 2 * 16 + 4 * 4
    lit = entries()
    LT.clear(t)
    after = entries()
    for k in ("world", "instanced", "posed"):
        same_planes(before[k], after[k], k)
        assert (lit[k]["color"] != before[k]["color"]).any(), k
        same_planes(lit[k], before[k], k, PLANES[1:])              # the G-buffer is the first hit's either way
    assert before["instanced"]["ids"].tobytes() == after["instanced"]["ids"].tobytes() == lit["instanced"]["ids"].tobytes()
    assert before["posed"]["ids"].tobytes() == lit["posed"]["ids"].tobytes()
    for x, y, z in zip(before["chain"], after["chain"], lit["chain"]):
        assert x.tobytes() == y.tobytes() and x.tobytes() != z.tobytes()
    # 3: under a table the world-only entry, the instanced entry with no instance and the posed entry with both tables empty are one frame
    LT.set(t, LT.host_from_quads(t.volume_extract_quads(), materials())[0])
    a = t.trace_paths(cam, 2, 3, frame_index=1)
    b = t.trace_paths_instanced(cam, none_i, 2, 3, frame_index=1)
    c = t.trace_paths_posed(cam, none_i, none_p, 2, 3, frame_index=1)
    same_planes(a, b, "world / instanced")
    same_planes(a, c, "world / posed")
    assert (b["ids"] == 0xFFFFFFFF).all() and b["ids"].tobytes() == c["ids"].tobytes()
    same_planes(a, lit["world"], "set_lights of the host build / from_quads", PLANES[1:])
    t.shutdown()


# ---- 4: the direct term ----------------------------------------------------------------------------------------------------------------------------
def nee_reference(t, cam, planes, hits, table, info, mats, vs=1.0, frame=0, trace=None):
    """The light sample of every pixel's first hit at spp = 1 (sample 0: no jitter): (term (h, w, 3) float32, skip (h, w) bool, occluded (h, w) bool).
    skip: the shadow ray's closest t lies within 1e-3 of an end of its interval."""
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
    term = np.zeros((h, w, 3), dtype=f32)
    rays = np.zeros((h, w), dtype=RAY)
    rays["dir"] = (1.0, 0.0, 0.0)
    has_ray = np.zeros((h, w), dtype=bool)
    n_faces, area = int(info["n_faces"][0]), info["area_world"][0]
    for y, x in np.argwhere(eligible):
        pick = LR.pick_of(int(r[y, x]), n_faces)
        i = LR.find_light(table, pick)
        q, nl = LR.sample_point(table[i], pick - int(table["cum"][i]), u1[y, x], u2[y, x], vs)
        g, org, dr, dist = LR.geometry(pos[y, x], nrm[y, x], q, nl, area)
        if g == 0:
            continue
        le = mats["emission"][LR.material_index(table["material"][i], len(mats))].astype(f32)
        term[y, x] = ((f32(1.0) * diffuse[y, x]) * le) * g
        rays[y, x] = (org, f32(0.001), dr, dist - LR.K_LIGHT_EPS)
        has_ray[y, x] = True
    shadow = (trace or t.trace_rays)(rays[has_ray])
    occluded = np.zeros((h, w), dtype=bool)
    occluded[has_ray] = shadow["hit"] == 1
    skip = np.zeros((h, w), dtype=bool)
    near = (shadow["hit"] == 1) & ((shadow["t"] - rays[has_ray]["tmin"] < 1e-3) | (rays[has_ray]["tmax"] - shadow["t"] < 1e-3))
    skip[has_ray] = near
    return np.where(occluded[..., None], f32(0.0), term), term, skip, occluded


def test_direct_term_equals_the_numpy_restatement(torch_cuda):
    """spp = 1, max_bounces = 1: lit colour = float32(unlit + nee_ref) at tests/test_paths.py's colour contract 1e-4 + 1e-3 |ref|.  Prints how
    many pixels are not bit-equal."""
    t = tracer()
    d, m = plate_scene()
    info = install(t, d, m)
    table = LT.download(t)
    mats = materials()
    cam = W.camera_look_at(*PLATE_CAM, 60.0, WD, HT)
    lit = t.trace_paths(cam, 1, 1, frame_index=0)
    hits = t.draw_frame(cam)
    LT.clear(t)
    unlit = t.trace_paths(cam, 1, 1, frame_index=0)
    same_planes(lit, unlit, "G-buffer", PLANES[1:])
    nee, unshadowed, skip, occluded = nee_reference(t, cam, unlit, hits, table, info, mats)
    nonzero = (unshadowed > 0).any(-1)
    floor = (hits["hit"] == 1) & (unlit["normal_roughness"][..., 1] == 1.0) & (unlit["world_pos"][..., 1] < 2.5)
    print(f"pixels with a term {int(nonzero.sum())}, of them on the floor {int((nonzero & floor).sum())}, occluded {int((occluded & nonzero).sum())}, "
          f"skipped {int((skip & nonzero).sum())}")
    assert (nonzero & floor).sum() > 500
    assert (skip & nonzero).sum() <= 0.01 * nonzero.sum()
    want = (unlit["color"][..., :3] + nee).astype(f32)
    got = lit["color"][..., :3]
    keep = ~skip
    err = np.abs(got.astype(np.float64) - want)
    bound = 1e-4 + 1e-3 * np.abs(want)
    not_bit_equal = int(((got.view(np.uint32) != want.view(np.uint32)).any(-1) & keep).sum())
    print(f"not bit-equal: {not_bit_equal} of {int(keep.sum())} pixels; worst error / bound {float((err / bound)[keep].max()):.3g}")
    assert (err <= bound)[keep].all(), np.argwhere((err > bound).any(-1) & keep)[:6].tolist()
    # no self-shadowing by the emitter's own voxels: every floor pixel with a term is brighter
    sel = floor & nonzero & keep
    assert not (occluded & sel).any()
    assert (got[sel].sum(-1) > unlit["color"][..., :3][sel].sum(-1)).all()
    t.shutdown()


# ---- 5: the device against the host shim ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp,bounces", [(4, 2), (2, 3)])
def test_gpu_frame_against_the_host_shim(torch_cuda, tmp_path, spp, bounces):
    """Two glowing materials, an instance and a pose; the rule of tests/test_paths.py::test_gpu_paths_within_tolerance_64: the first hit
    exact, every pixel's colour within 1e-4 + 1e-3 |ref|, the mean absolute difference below 2e-4."""
    from tests import test_lit_paths_cpu as CPU
    mats = CPU.materials()
    d, m = CPU.mixed_scene()
    t = tracer()
    info = install(t, d, m, mats=mats)
    table = LT.download(t)
    assert int(info["n_owned"][0]) == 2 and len(table) == 11      # (the block stands on the floor: five faces of it, six of the plate)
    xyz, ids = CPU.mixed_models()
    model = t.model_create(xyz, ids)
    inst = np.array([IO.instance(model, (6, 2, 8))], dtype=INSTANCE)
    pose = P.rotation(model, 0.6, 0.25, 0.1, 1.0, (2.0, 2.0, 2.0), (21.0, 6.0, 12.0))
    cam = W.camera_look_at(*CPU.MIXED_CAM, 60.0, WD, HT)
    got = t.trace_paths_posed(cam, inst, pose, spp, bounces, frame_index=5)
    shim = CPU.LitShim(tmp_path / "liblit_paths_shim.so")
    world = shim.tree(*CPU.voxels_of(d, m))
    ref = shim.render(world, [shim.tree(xyz, ids)], inst, pose, cam, mats, WD, HT, spp, bounces, 5, table=table)
    for k in PLANES[1:] + ("ids",):
        assert np.array_equal(got[k], ref[k]), k
    err = np.abs(got["color"] - ref["color"])
    ok = (err <= 1e-4 + 1e-3 * np.abs(ref["color"])).all(axis=2)
    print(f"({spp}, {bounces}): {int((~ok).sum())} pixels outside the tolerance, mean |difference| {float(err.mean()):.3g}, pose pixels {int(((got['ids'] != 0xFFFFFFFF) & (got['ids'] >> 31 == 1)).sum())}, "
          f"instance pixels {int((got['ids'] == 0).sum())}")
    assert ok.all(), np.argwhere(~ok)[:8].tolist()
    assert err.mean() < 2e-4
    assert (got["ids"] == 0).sum() > 20 and ((got["ids"] != 0xFFFFFFFF) & (got["ids"] >> 31 == 1)).sum() > 20
    t.shutdown()


# ---- 6: the expectation ---------------------------------------------------------------------------------------------------------------------------
ROOM_SPP = 64


def test_lit_loop_has_the_unlit_loops_expectation_and_less_variance(torch_cuda):
    """A closed 24^3 room, grey walls, a glowing 4 x 4 ceiling patch, the camera looks at the floor; 32 x 24 pixels, three bounces, K = 16
    frames of each loop.  |mean(m_lit) - mean(m_unlit)| <= 4 sqrt(var(m_lit) / K + var(m_unlit) / K), that bound below 10 % of mean(m_unlit),
    and var(m_lit) < var(m_unlit)."""
    w, h, K = 32, 24, 16
    t = tracer(w, h)
    d = np.ones((24, 24, 24), dtype=f32)
    m = np.full((24, 24, 24), GREY, dtype=np.uint32)
    d[1:23, 1:22, 1:23] = 0.0                     # (a ceiling two voxels thick: the patch's only exposed faces look into the room)
    m[10:14, 22, 10:14] = GLOW2
    install(t, d, m)
    info = LT.info(t)
    table = LT.download(t)
    assert int(info["n"][0]) == 1 and int(info["n_faces"][0]) == 16 and table["face"][0] == 3
    cam = W.camera_look_at((12.0, 14.0, 4.0), (12.0, 1.0, 13.0), 70.0, w, h)
    hits = t.draw_frame(cam)
    floor = (hits["hit"] == 1) & (hits["face"] == 2) & (hits["voxel"][..., 1] == 0)
    assert floor.sum() > 300
    lit = [t.trace_paths(cam, ROOM_SPP, 3, frame_index=k)["color"][..., :3][floor].astype(np.float64).mean() for k in range(K)]
    LT.clear(t)
    unlit = [t.trace_paths(cam, ROOM_SPP, 3, frame_index=k)["color"][..., :3][floor].astype(np.float64).mean() for k in range(K)]
    m_lit, m_unlit = np.array(lit), np.array(unlit)
    bound = 4.0 * np.sqrt(m_lit.var(ddof=1) / K + m_unlit.var(ddof=1) / K)
    print(f"spp {ROOM_SPP}: mean lit {m_lit.mean():.6g} unlit {m_unlit.mean():.6g} difference {abs(m_lit.mean() - m_unlit.mean()):.3g} bound {bound:.3g} "
          f"({100.0 * bound / m_unlit.mean():.2f} % of the unlit mean); var lit {m_lit.var(ddof=1):.3g} unlit {m_unlit.var(ddof=1):.3g}")
    assert m_unlit.mean() > 0 and bound < 0.10 * m_unlit.mean()
    assert abs(m_lit.mean() - m_unlit.mean()) <= bound
    assert m_lit.var(ddof=1) < m_unlit.var(ddof=1)
    t.shutdown()


# ---- 7: shadows see everything ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["instance", "pose"])
def test_a_placed_plate_between_light_and_floor_shadows_it(torch_cuda, kind):
    t = tracer()
    d, m = plate_scene()
    info = install(t, d, m)
    table = LT.download(t)
    mats = materials()
    cam = W.camera_look_at(*PLATE_CAM, 60.0, WD, HT)
    xyz = np.stack(np.meshgrid(np.arange(10), np.arange(1), np.arange(10), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    model = t.model_create(xyz, np.full(len(xyz), DARK, dtype=np.uint32))
    place = np.array([IO.instance(model, (11, 8, 11))], dtype=INSTANCE)
    none_i, none_p = np.zeros(0, dtype=INSTANCE), np.zeros(0, dtype=POSE)
    if kind == "instance":
        inst, poses = place, none_p
    else:
        inst, poses = none_i, P.rotation(model, 0.4, 0.0, 0.0, 1.0, (5.0, 0.5, 5.0), (16.0, 8.5, 16.0))
    with_plate = t.trace_paths_posed(cam, inst, poses, 1, 1, frame_index=0)
    bare = t.trace_paths(cam, 1, 1, frame_index=0)
    hits, ids, _ = t.trace_primary_posed(cam, inst, poses)
    LT.clear(t)
    with_plate_unlit = t.trace_paths_posed(cam, inst, poses, 1, 1, frame_index=0)
    bare_unlit = t.trace_paths(cam, 1, 1, frame_index=0)
    _, unshadowed, skip, occluded = nee_reference(t, cam, with_plate_unlit, hits, table, info, mats, trace=lambda rays: t.trace_rays_posed(rays, inst, poses)[0])
    floor = (hits["hit"] == 1) & (ids == 0xFFFFFFFF) & (with_plate_unlit["normal_roughness"][..., 1] == 1.0) & (with_plate_unlit["world_pos"][..., 1] < 2.5)
    floor &= (bare_unlit["world_pos"] == with_plate_unlit["world_pos"]).all(-1)
    sel = floor & (unshadowed > 0).any(-1) & occluded & ~skip
    print(f"{kind}: floor pixels with a term {int((floor & (unshadowed > 0).any(-1)).sum())}, of them occluded by the plate {int(sel.sum())}")
    assert sel.sum() >= 40
    assert (with_plate["color"][sel] == with_plate_unlit["color"][sel]).all()
    assert (bare["color"][..., :3][sel].sum(-1) > bare_unlit["color"][..., :3][sel].sum(-1)).all()
    t.shutdown()


# ---- 8: the chain ----------------------------------------------------------------------------------------------------------------------------------
def test_the_motion_chain_runs_lit(torch_cuda):
    t = tracer()
    d, m = plate_scene()
    install(t, d, m)
    cam = W.camera_look_at(*PLATE_CAM, 60.0, WD, HT)
    cube = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    model = t.model_create(cube, np.full(len(cube), GREY, dtype=np.uint32))
    frames = {}
    for lit in (True, False):
        if not lit:
            LT.clear(t)
        t.post_reset()
        frames[lit] = [t.draw_frame_rt_posed_motion(cam, None, P.rotation(model, 0.2 * k, 0.1, 0.0, 1.0, (1.5, 1.5, 1.5), (18.0 + k, 5.0, 14.0)), 2, 2)[0] for k in range(3)]
    for a, b in zip(frames[True], frames[False]):
        assert a.shape == (HT, WD) and (a >> 24 == 0xFF).all() and a.tobytes() != b.tobytes()
    t.shutdown()
