"""The finer bounds a view at rest keeps from its K-th hit on (blok_amd/csrc/hip/beam_cache.h: plan_beam_refine; api_launch.hip;
beam_refine_kernel, beam_fill_kernel), by tests/test_beam_cache_gpu.py's method: every frame of every scenario is compared byte for byte,
records and RGBA8, with the same launches made by a twin tracer whose cache is switched off — into output buffers filled with a garbage
pattern before every launch, so a pixel nobody rewrote shows — over three streams, and the counters say which launches searched, filled,
refined and walked from which bounds.  The bounds themselves are checked as numbers: against the pre-pass at 8 and at 32 pixels, and,
independently of any search, against the hit records of the frame.  Frames of 200 x 136 over the 64^3 scene; one test at 616 x 456, where the
view also gets its longest-first order and walk workgroups for the order's live prefix only."""
import numpy as np
import pytest

from blok_amd import world as W
from tests.conftest import SEED
from tests.test_beam_cache_gpu import GARBAGE, HT, WD, one_ulp, view, volume64

pytestmark = pytest.mark.gpu

NONE = np.float32(3.0e38)                                # trace_kernels.h: kBeamNone
CUT = (37, 19, 101, 55)                                  # a rectangle whose beam tiles and wave tiles are cut on all sides


@pytest.fixture(scope="module")
def tracer_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from blok_amd.tracer import HipTracer
    return HipTracer


class Runner:
    """One tracer and the launches of a scenario: ("frame", camera, rectangle or None) steps go round three streams into their own
    garbage-filled buffers, without a synchronisation in between unless `lockstep`; any other step is a callable applied to the tracer (behind
    a synchronisation).  -> the frames, and per frame (hits, fills, refines, action, fine state) as they stood after its launch."""

    def __init__(self, tracer, wd, ht):
        import torch
        self.torch, self.tr, self.wd, self.ht = torch, tracer, wd, ht
        self.streams = [torch.cuda.Stream() for _ in range(3)]

    def run(self, steps, lockstep):
        torch = self.torch
        frames, log, k = [], [], 0
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
            frames.append((hits, rgba))
            log.append(self.tr.beam_cache_counters() + (self.tr.beam_cache_refines(), self.tr.beam_cache_last_action(), self.tr.beam_cache_fine_state()))
            if lockstep:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return frames, log

    def close(self):
        self.torch.cuda.synchronize()
        for s in self.streams:
            self.tr.release_stream(s.cuda_stream)
        self.tr.shutdown()


def check(tracer_cls, setup, steps, after, lockstep=False, wd=WD, ht=HT, probe=None):
    """Runs the steps on the twin (cache off) and on the tracer under test (K = after), one after the other, and compares every frame.
    -> the log of the tracer under test, the twin's frames, and what probe(tracer under test, twin) returned at the end."""
    import torch
    on, off = tracer_cls(wd, ht).init(), tracer_cls(wd, ht).init()
    off.set_beam_cache(False)
    on.set_beam_refine_after(after)
    for t in (on, off):
        setup(t)
    on, off = Runner(on, wd, ht), Runner(off, wd, ht)
    try:
        want, ref_log = off.run(steps, lockstep)
        got, log = on.run(steps, lockstep)
        assert all(entry == (0, 0, 0, 0, 0) for entry in ref_log), "a tracer with the cache off never hits, fills or refines"
        assert len(got) == len(want)
        for k, ((gh, gc), (wh, wc)) in enumerate(zip(got, want)):
            assert torch.equal(gh, wh), f"frame {k}: records differ in {int((gh != wh).any(dim=1).sum())} pixels"
            assert torch.equal(gc, wc), f"frame {k}: RGBA8 differs in {int((gc != wc).sum())} pixels"
            assert not bool((wc == GARBAGE).any()), f"frame {k}: the reference left pixels unwritten"
        return log, want, (probe(on.tr, off.tr) if probe else None)
    finally:
        on.close(); off.close()


def world64(scene64):
    return lambda t: t.add_world(scene64[1])


def frames(cam, n, rect=None):
    return [("frame", cam, rect)] * n


def resting(n, after, fills=1, before=(0, 0, 0)):
    """The log of n launches of one view that nothing disturbs, from its first launch on: a search, a fill, `after` - 1 hits from the beam
    tiles' bounds, the hit that refines behind its walk, hits from the finer bounds.  before: the counters when the view arrived."""
    out = []
    for k in range(n):
        hits = max(k - 1, 0)
        out.append((before[0] + hits, before[1] + (fills if k >= 1 else 0), before[2] + (1 if hits >= after else 0),
                    0 if k == 0 else 1 if k == 1 else 2, 0 if hits < after else 1 if hits == after else 2))
    return out


def wave_grid(w, h):
    return (w + 7) // 8, (h + 7) // 8


def coarse_of_wave_tiles(coarse, w, h, beam_tile):
    """The beam tiles' bounds (row-major over the rectangle) looked up per 8 x 8 wave tile."""
    nx, ny = wave_grid(w, h)
    bx = (w + beam_tile - 1) // beam_tile
    ys, xs = np.divmod(np.arange(nx * ny), nx)
    return coarse[(ys * 8 // beam_tile) * bx + xs * 8 // beam_tile]


def bounds_probe(cam, rect, beam_tile=32):
    """-> probe for check(): the finer and the beam tiles' bounds of the latest launch of the tracer under test, and the twin's pre-pass of
    the same view at 8 pixels and at the beam tile."""
    def probe(on, off):
        state, fine = on.beam_cache_fine()
        action, coarse = on.beam_cache_last()
        off.set_beam(8); p8, _ = off.beam_prepass(cam, rect)
        off.set_beam(beam_tile); pb, _ = off.beam_prepass(cam, rect)
        return state, fine, action, coarse, p8, pb
    return probe


@pytest.mark.parametrize("rect", [None, CUT], ids=["whole_frame", "rectangle_cut_on_all_sides"])
def test_the_finer_bounds_as_numbers(tracer_cls, scene64, rect):
    """Part 1: bit for bit max(8-pixel pre-pass, 32-pixel pre-pass of the wave tile's beam tile), none wherever either says none.  Part 2,
    independent of the pre-pass: a finite bound is at most the smallest t among its wave tile's hit records in the twin's frame, and a wave
    tile without a bound has no hit record.  First of all: the view has wave tiles that are empty by their own search inside live beam tiles
    (any silhouette against the sky gives them), which is what the writer rule of the launches is about.  Frames compared on the way."""
    cam = view(1)
    w, h = (rect[2], rect[3]) if rect else (WD, HT)
    log, want, (state, fine, action, coarse, p8, p32) = check(tracer_cls, world64(scene64), frames(cam, 5, rect), after=1, lockstep=True,
                                                               probe=bounds_probe(cam, rect))
    assert log == resting(5, 1)
    nx, ny = wave_grid(w, h)
    assert state == 2 and action == 2 and len(fine) == nx * ny == len(p8) and len(coarse) == len(p32)
    assert np.array_equal(coarse.view(np.uint32), p32.view(np.uint32)), "the ordinary download goes on returning the beam tiles' bounds"
    c = coarse_of_wave_tiles(p32, w, h, 32)
    empty_inside_live = (fine >= NONE) & (c < NONE)
    print(f"wave tiles {nx * ny}: live {int((fine < NONE).sum())}, empty by their own search inside a live beam tile {int(empty_inside_live.sum())}, "
          f"raised above their beam tile's bound {int(((fine < NONE) & (fine > c)).sum())}")
    assert empty_inside_live.any()
    # part 1
    expect = np.where((p8 >= NONE) | (c >= NONE), NONE, np.maximum(p8, c)).astype(np.float32)
    assert np.array_equal(fine.view(np.uint32), expect.view(np.uint32)), f"{int((fine.view(np.uint32) != expect.view(np.uint32)).sum())} wave tiles differ"
    assert ((fine < NONE) & (fine > c)).any(), "no wave tile starts later than its beam tile: the finer bounds would buy nothing here"
    # part 2
    rec = want[0][0].cpu().numpy()
    t = rec[:, 0].copy().view(np.float32).reshape(h, w)
    hit = (((rec[:, 3] >> 24) & 0xFF) != 0).reshape(h, w)
    assert hit.any() and not hit.all()
    for k in range(nx * ny):
        ty, tx = divmod(k, nx)
        sub_hit = hit[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
        if fine[k] >= NONE:
            assert not sub_hit.any(), f"wave tile {k} has hit records and no bound"
        elif sub_hit.any():
            nearest = t[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8][sub_hit].min()
            assert fine[k] <= nearest, f"wave tile {k}: bound {fine[k]} beyond its nearest hit {nearest}"


@pytest.mark.parametrize("lockstep", [False, True], ids=["in_flight", "one_at_a_time"])
def test_frames_before_the_refinement_the_launch_that_refines_and_frames_after_it(tracer_cls, scene64, lockstep):
    """Three frames in flight (the launches after the refinement wait for it on the other two streams), and one frame at a time."""
    log, _, _ = check(tracer_cls, world64(scene64), frames(view(0), 9), after=2, lockstep=lockstep)
    assert log == resting(9, 2)
    assert [e[4] for e in log] == [0, 0, 0, 1, 2, 2, 2, 2, 2]


def test_a_rectangle_whose_tiles_are_cut_on_all_sides(tracer_cls, scene64):
    log, _, _ = check(tracer_cls, world64(scene64), frames(view(2), 6, CUT), after=1)
    assert log == resting(6, 1)


def test_the_pre_pass_as_miss_writer_the_fill_kernel_writes_the_empty_wave_tiles(tracer_cls, scene64):
    """Without the walk as miss writer every wave tile has its walk workgroup, and the one of a wave tile that is empty by its own bound
    writes nothing: its 64 misses are the fill wave's of its beam tile."""
    def setup(t):
        t.add_world(scene64[1]); t.set_miss_writer(False)
    log, _, _ = check(tracer_cls, setup, frames(view(1), 7), after=2)
    assert log == resting(7, 2)


@pytest.mark.parametrize("beam_tile", [16, 64, 8])
def test_beam_tiles_of_16_and_64_are_refined_and_of_8_never(tracer_cls, scene64, beam_tile):
    cam = view(3)

    def setup(t):
        t.add_world(scene64[1]); t.set_beam(beam_tile)
    log, _, got = check(tracer_cls, setup, frames(cam, 6), after=1, probe=bounds_probe(cam, None, beam_tile) if beam_tile != 8 else None)
    if beam_tile == 8:                                   # the beam tile IS the wave tile: nothing finer to keep
        assert log == [(max(k - 1, 0), 1 if k else 0, 0, min(k, 2), 0) for k in range(6)]
        return
    assert log == resting(6, 1)
    state, fine, _, _, p8, pb = got
    c = coarse_of_wave_tiles(pb, WD, HT, beam_tile)
    expect = np.where((p8 >= NONE) | (c >= NONE), NONE, np.maximum(p8, c)).astype(np.float32)
    assert state == 2 and np.array_equal(fine.view(np.uint32), expect.view(np.uint32))


def test_a_resting_view_with_its_order_walks_the_prefix_from_the_finer_bounds(tracer_cls):
    """616 x 456: enough wave tiles for the longest-first order, so launches at rest dispatch walk workgroups for the order's live prefix only.
    The refinement (K = 6) comes while such an order is in force: the walk workgroups of wave tiles that are empty by their own bound exit and
    the fill waves write their misses, until a re-sort (every 2 frames) drops them from the prefix.  Then a cap on the prefix — the fill waves walk
    the rest, each wave tile by its own bound first — and the brush edit of the order test: the finer bounds go with the tree they were
    searched in, and the view is refined again."""
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
    for _ in range(14):
        steps += [("frame", cam, None), (note,)]
    steps += [(lambda t: t.set_joint_prefix_limit(300),)] + frames(cam, 2) + [(note,), (lambda t: t.set_joint_prefix_limit(0),)]
    steps += [(ball,)] + frames(cam, 10) + [(note,)]

    def probe(on, off):
        state, fine = on.beam_cache_fine()
        off.set_beam(32); p32, _ = off.beam_prepass(cam, None)
        return state, fine, p32
    log, _, (state, fine, p32) = check(tracer_cls, setup, steps, after=6, lockstep=True, wd=wd, ht=ht, probe=probe)
    assert log[:16] == resting(16, 6)                    # (the launch that refines is the eighth)
    assert log[16:] == resting(10, 6, before=(14, 1, 1))
    on_uses = uses[len(uses) // 2:]                      # the tracer under test ran second
    print("order use per frame:", on_uses)
    assert on_uses[7] == 1 and on_uses[13] == 1 and on_uses[14] == 1, on_uses      # the refinement, frames after it and the capped ones walked in the view's own order: prefix launches
    assert state == 2 and ((fine >= NONE) & (coarse_of_wave_tiles(p32, wd, ht, 32) < NONE)).any()


def test_another_view_a_rebuilt_and_a_replaced_world_are_not_walked_from_these_bounds(tracer_cls, scene64):
    """One ulp of one camera float, a volume_rebuild and a second add_world: the launch that follows uses neither the finer bounds nor, for
    the two changes of the tree, any kept bounds at all; the view as it was still has its finer bounds when the camera returns to it."""
    cam = view(4)
    mats = W.scene_materials(SEED)

    def dig(t):
        t.volume_apply_brush((32.0, 20.0, 32.0), 9.0, 0.0, 1)
        t.volume_rebuild(mats)

    steps = frames(cam, 4)
    for word in (0, 4, 12):                              # pos.x, fwd.y, tan_half_fov
        steps += [("frame", one_ulp(cam, word), None), ("frame", cam, None)]
    steps += [(dig,)] + frames(cam, 4)
    steps += [(lambda t: t.add_world(scene64[1]),)] + frames(cam, 4)
    log, _, _ = check(tracer_cls, volume64, steps, after=1)
    assert log[:4] == resting(4, 1)
    for k in (4, 6, 8):
        assert log[k][3:] == (0, 0) and log[k + 1][3:] == (2, 2), (k, log[k], log[k + 1])      # the other view searches; the view itself walks on from its finer bounds
    assert log[9][:3] == (5, 1, 1)
    assert log[10:14] == resting(4, 1, before=(5, 1, 1))      # a rebuilt tree: search, fill, refine, walk — nothing of the old tree's is used
    assert log[14:18] == resting(4, 1, before=(7, 2, 2))      # a replaced world: the same
