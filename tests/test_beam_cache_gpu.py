"""The beam bounds a view at rest keeps from launch to launch (blok_amd/csrc/hip/beam_cache.h, api_launch.hip, beam_fill_kernel): every
frame of every scenario is compared byte for byte, records and RGBA8, with the same sequence of launches made by a tracer whose cache is
switched off — into output buffers filled with a garbage pattern before every launch, so a pixel nobody rewrote shows — and the counters
say which launches searched, which filled a slot and which walked from kept bounds.  Frames of 200 x 136 (beam tiles cut at the right and
at the bottom) over the 64^3 scene, three streams as FramePipeline uses them; one test at 616 x 456, where a view at rest also gets its
longest-first order and walk workgroups for the order's live prefix only."""
import numpy as np
import pytest

from blok_amd import world as W
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

WD, HT = 200, 136
GARBAGE = 0x5A5A5A5A


@pytest.fixture(scope="module")
def tracer_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from blok_amd.tracer import HipTracer
    return HipTracer


def view(k, wd=WD, ht=HT, radius=95.0):
    a = np.radians(37.0 * k + 11.0)
    return W.camera_look_at((32.0 + radius * np.cos(a), 48.0 + 3.0 * (k % 3), 32.0 + radius * np.sin(a)), (32.0, 18.0, 32.0), 60.0, wd, ht)


def one_ulp(cam, word):
    c = cam.copy()
    f = c.view(np.float32).reshape(-1)
    f[word] = np.nextafter(f[word], np.float32(np.inf))
    assert (c.view(np.uint32) != cam.view(np.uint32)).sum() == 1
    return c


class Runner:
    """One tracer and the launches of a scenario: ("frame", camera, rectangle or None) steps go round three streams into their own garbage-filled
    buffers, without a synchronisation in between unless `lockstep`; any other step is a callable applied to the tracer (behind a synchronisation).
    Returns the frames, and the (hits, fills) counters as they stood after every frame's launch."""

    def __init__(self, tracer, wd=WD, ht=HT):
        import torch
        self.torch, self.tr, self.wd, self.ht = torch, tracer, wd, ht
        self.streams = [torch.cuda.Stream() for _ in range(3)]

    def run(self, steps, lockstep=False):
        torch = self.torch
        frames, counters, k = [], [], 0
        for step in steps:
            if step[0] != "frame":
                torch.cuda.synchronize()
                step[0](self.tr, *step[1:])
                continue
            _, cam, rect = step
            n = (rect[2] * rect[3]) if rect else self.wd * self.ht
            s = self.streams[k % 3]; k += 1
            with torch.cuda.stream(s):
                hits = torch.full((n, 4), GARBAGE, dtype=torch.int32, device="cuda")
                rgba = torch.full((n,), GARBAGE, dtype=torch.int32, device="cuda")
            self.tr.draw_frame_device(cam, hits.data_ptr(), rgba.data_ptr(), rect=rect, stream=s.cuda_stream)
            frames.append((hits, rgba)); counters.append(self.tr.beam_cache_counters())
            if lockstep:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return frames, counters

    def close(self):
        self.torch.cuda.synchronize()
        for s in self.streams:
            self.tr.release_stream(s.cuda_stream)
        self.tr.shutdown()


def pair(tracer_cls, setup, wd=WD, ht=HT):
    """The tracer under test and its twin with the cache switched off, both set up by `setup`."""
    on, off = tracer_cls(wd, ht).init(), tracer_cls(wd, ht).init()
    off.set_beam_cache(False)
    for t in (on, off):
        setup(t)
    return Runner(on, wd, ht), Runner(off, wd, ht)


def check(tracer_cls, setup, steps, lockstep=False, wd=WD, ht=HT):
    """Runs the steps on both tracers, one after the other (each has the device to itself), and compares every frame.  -> the counters of the
    tracer under test after every frame, and the reference frames."""
    import torch
    on, off = pair(tracer_cls, setup, wd, ht)
    try:
        want, ref_counters = off.run(steps, lockstep)
        got, counters = on.run(steps, lockstep)
        assert all(c == (0, 0) for c in ref_counters), "a tracer with the cache off must never hit or fill"
        assert len(got) == len(want)
        for k, ((gh, gc), (wh, wc)) in enumerate(zip(got, want)):
            assert torch.equal(gh, wh), f"frame {k}: records differ in {int((gh != wh).any(dim=1).sum())} pixels"
            assert torch.equal(gc, wc), f"frame {k}: RGBA8 differs in {int((gc != wc).sum())} pixels"
            assert not bool((wc == GARBAGE).any()), f"frame {k}: the reference left pixels unwritten"
        return counters, want
    finally:
        on.close(); off.close()


def world64(scene64):
    return lambda t: t.add_world(scene64[1])


def frames(cam, n, rect=None):
    return [("frame", cam, rect)] * n


def is_hit(counters, k):
    return counters[k][0] == (counters[k - 1][0] if k else 0) + 1


def test_the_scene_has_live_and_empty_beam_tiles(tracer_cls, scene64):
    """What every test below relies on: the views see the world and the sky, so both kinds of beam tile are there."""
    _, want = check(tracer_cls, world64(scene64), [("frame", view(k), None) for k in range(5)])
    for hits, _ in want:
        hit = ((hits[:, 3] >> 24) & 0xFF).reshape(HT, WD).cpu().numpy() != 0
        tiles = [hit[y:y + 32, x:x + 32].any() for y in range(0, HT, 32) for x in range(0, WD, 32)]
        assert any(tiles) and not all(tiles)


@pytest.mark.parametrize("lockstep", [False, True], ids=["in_flight", "one_at_a_time"])
def test_one_view_fills_once_and_hits_from_the_third_frame_on(tracer_cls, scene64, lockstep):
    """Three frames in flight (the automatic form keeps searches and walk apart), and one frame at a time (it plans a joint launch)."""
    counters, _ = check(tracer_cls, world64(scene64), frames(view(0), 8), lockstep)
    assert counters == [(0, 0), (0, 1)] + [(k, 1) for k in range(1, 7)]


def test_the_pre_pass_as_miss_writer_leaves_its_pixels_to_the_fill_kernel(tracer_cls, scene64):
    def setup(t):
        t.add_world(scene64[1]); t.set_miss_writer(False)
    counters, _ = check(tracer_cls, setup, frames(view(1), 6))
    assert counters[-1] == (4, 1)


def test_one_ulp_of_one_camera_float_is_another_view(tracer_cls, scene64):
    cam = view(0)
    steps = frames(cam, 3)
    for word in (0, 4, 7, 11, 12, 13):                   # pos.x, fwd.y, right.y, up.z, tan_half_fov, aspect
        steps += [("frame", one_ulp(cam, word), None), ("frame", cam, None)]
    counters, _ = check(tracer_cls, world64(scene64), steps)
    for k in range(3, len(steps), 2):
        assert not is_hit(counters, k) and is_hit(counters, k + 1), k
    assert counters[-1][1] == 1                          # ... and none of them was ever admitted


def test_two_views_alternating_are_both_kept(tracer_cls, scene64):
    a, b = view(0), view(3)
    steps = frames(a, 2) + frames(b, 2) + [("frame", (a, b)[k % 2], None) for k in range(8)]
    counters, _ = check(tracer_cls, world64(scene64), steps)
    assert counters[3] == (0, 2) and counters[-1] == (8, 2)


def test_five_views_cycling_through_four_slots_stay_exact_through_evictions(tracer_cls, scene64):
    steps = [("frame", view(k), None) for _ in range(3) for k in range(5) for _ in range(3)]      # 45 frames in flight, every visit evicts
    counters, _ = check(tracer_cls, world64(scene64), steps)
    assert counters[-1] == (15, 15)


def test_an_orbiting_camera_never_fills(tracer_cls, scene64):
    counters, _ = check(tracer_cls, world64(scene64), [("frame", view(0.1 * k), None) for k in range(12)])
    assert counters[-1] == (0, 0)


def test_beam_settings_budget_and_rectangle_are_part_of_the_view(tracer_cls, scene64):
    cam = view(2)
    steps = frames(cam, 3)
    steps += [(lambda t: t.set_beam(16),)] + frames(cam, 3)
    steps += [(lambda t: t.set_beam_budget(9),)] + frames(cam, 3)
    steps += frames(cam, 3, (8, 16, 171, 97)) + frames(cam, 3, (8, 16, 171, 98)) + frames(cam, 1)
    counters, _ = check(tracer_cls, world64(scene64), steps)
    # every change: a search, a fill, a hit; the whole frame under the last settings is still there at the end
    assert [c[0] for c in counters] == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6]
    assert counters[-1][1] == 5


def volume64(t):
    ids = W.scene_dense(64, SEED)
    z, y, x = np.nonzero(ids)
    t.volume_create((0, 0, 0), (64, 64, 64), 64, 1.0)
    t.volume_set_voxels(np.stack([x, y, z], 1).astype(np.int32), ids[z, y, x], np.ones(len(x), dtype=np.float32))
    t.volume_rebuild(W.scene_materials(SEED))


def test_an_edited_and_a_replaced_world_are_searched_afresh(tracer_cls, scene64):
    """A brush and a rebuild between frames of a resting view (the rebuild keeps the view's order, so only the tree's own counter tells),
    then a second add_world: no launch walks from the bounds of the world before, and every frame is the new world's."""
    import torch
    cam = view(4)
    mats = W.scene_materials(SEED)

    def ball(t):
        t.volume_apply_brush((32.0, 42.0, 32.0), 8.0, 1.0, 0)      # into the air above the scene: beam tiles that were empty are live now
        t.volume_rebuild(mats)

    def dig(t):
        t.volume_apply_brush((32.0, 20.0, 32.0), 9.0, 0.0, 1)
        t.volume_rebuild(mats)

    steps = frames(cam, 4) + [(ball,)] + frames(cam, 3) + [(dig,)] + frames(cam, 3) + [(lambda t: t.add_world(scene64[1]),)] + frames(cam, 3)
    counters, want = check(tracer_cls, volume64, steps)
    assert [c[0] for c in counters] == [0, 0, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5]
    assert counters[-1][1] == 4
    assert not torch.equal(want[3][0], want[4][0]) and not torch.equal(want[6][0], want[7][0])      # the edits are in the picture


def test_a_resting_view_with_its_order_walks_the_prefix_from_kept_bounds(tracer_cls):
    """616 x 456: enough wave tiles for the longest-first order, so launches at rest dispatch walk workgroups for the order's live prefix only and
    the fill kernel writes the empty tiles; then a cap on the prefix (the fill kernel's waves walk the rest), and an edit that keeps the order
    while tiles the order holds dead come alive."""
    wd, ht = 616, 456
    cam = view(1, wd, ht)
    mats = W.scene_materials(SEED)
    uses = []

    def setup(t):
        volume64(t); t.set_tile_ordering(2)

    def note(t):
        uses.append(t.last_order_use()[0])

    def ball(t):
        t.volume_apply_brush((32.0, 42.0, 32.0), 8.0, 1.0, 0)
        t.volume_rebuild(mats)

    steps = []
    for _ in range(8):
        steps += [("frame", cam, None), (note,)]
    steps += [(lambda t: t.set_joint_prefix_limit(300),)] + frames(cam, 2) + [(note,), (lambda t: t.set_joint_prefix_limit(0),)]
    steps += [(ball,)] + frames(cam, 4) + [(note,)]
    counters, _ = check(tracer_cls, setup, steps, lockstep=True, wd=wd, ht=ht)
    assert counters[9] == (8, 1) and counters[-1] == (10, 2)
    on_uses = uses[len(uses) // 2:]                      # the tracer under test ran second
    assert on_uses[7] == 1 and on_uses[8] == 1, on_uses  # hits walked in the view's own order: prefix launches
