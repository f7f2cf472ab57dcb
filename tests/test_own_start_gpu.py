"""Mode 4 of the beam cache: every listed ray of a view at rest restarts where its own counted walk ended (blok_amd/csrc/hip/beam_cache.h:
BeamStartKey, plan_beam_starts; trace_count_own_kernel, pack_starts_kernel, packed_walk_own_kernel), by tests/test_beam_list_gpu.py's method and
on its frames (200 x 136 over the 64^3 scene): every frame of every scenario is compared byte for byte, records and RGBA8, with the same
launches made by a twin tracer whose cache is switched off, into buffers filled with garbage; the starts are checked as numbers from their
download — against the frame's records, the finer bounds, and the walk compiled for the host started from them."""
import ctypes as C

import numpy as np
import pytest

from blok_amd import world as W
from tests.conftest import SEED
from tests.test_beam_cache_gpu import GARBAGE, HT, WD, one_ulp, view, volume64
from tests.test_beam_refine_gpu import CUT, NONE, frames, wave_grid, world64
from tests.test_beam_list_gpu import DOWN, SKY, SMALL, ListRunner, expected_areas, list_errors, wait
from tests import test_beam_list_gpu as base

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tracer_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from blok_amd import _ffi
    from blok_amd.tracer import HipTracer
    base.AREA = int(_ffi.hip_lib().blok_hip_pack_area())      # (expected_areas and list_errors read the module's)
    base.GROUPS = base.AREA * base.AREA // 64
    return HipTracer


class OwnRunner(ListRunner):
    """ListRunner, with the starts in the log: per frame (action, fine state, list state, builds so far, starts state, from the starts so
    far, other start keys so far)."""

    def run(self, steps, lockstep):
        torch = self.torch
        frames_, log, k = [], [], 0
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
            frames_.append((hits, rgba))
            log.append((self.tr.beam_cache_last_action(), self.tr.beam_cache_fine_state(), self.tr.beam_cache_list_state(), self.tr.beam_cache_list_builds(),
                        self.tr.beam_cache_starts_state()) + self.tr.beam_cache_start_counters())
            if lockstep:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return frames_, log


def check(tracer_cls, setup, steps, lockstep=False, after=1, probe=None):
    """Runs the steps on the twin (cache off) and on the tracer under test (mode 4, K = 1, N = after), one after the other, and compares
    every frame.  -> the log of the tracer under test, the twin's frames, and what probe(tracer under test) returned at the end."""
    import torch
    on, off = tracer_cls(WD, HT).init(), tracer_cls(WD, HT).init()
    off.set_beam_cache(False)
    on.set_beam_cache(4); on.set_beam_refine_after(1); on.set_beam_list_after(after)
    for t in (on, off):
        setup(t)
    on, off = OwnRunner(on, WD, HT), OwnRunner(off, WD, HT)
    try:
        want, ref_log = off.run(steps, lockstep)
        got, log = on.run(steps, lockstep)
        assert all(entry == (0,) * 7 for entry in ref_log), "a tracer with the cache off never hits, refines, builds or has starts"
        assert len(got) == len(want)
        for k, ((gh, gc), (wh, wc)) in enumerate(zip(got, want)):
            assert torch.equal(gh, wh), f"frame {k} {log[k]}: records differ in {int((gh != wh).any(dim=1).sum())} pixels"
            assert torch.equal(gc, wc), f"frame {k} {log[k]}: RGBA8 differs in {int((gc != wc).sum())} pixels"
            assert not bool((wc == GARBAGE).any()), f"frame {k}: the reference left pixels unwritten"
        return log, want, (probe(on.tr) if probe else None)
    finally:
        on.close(); off.close()


def resting(n, after=1):
    """The log of n launches of one view under one start key, one at a time: a search, a fill, the hit that refines, `after` - 1 hits from
    the finer bounds, the hit that counts the trips and the starts and builds, packed hits from the starts."""
    out = []
    for k in range(n):
        count = 2 + after
        out.append((min(k, 2), 0 if k < 2 else 1 if k == 2 else 2, 0 if k < count else 1 if k == count else 2, 1 if k >= count else 0,
                    1 if k >= count else 0, max(k - count, 0), 0))
    return out


def test_the_default_is_mode_4(tracer_cls, scene64):
    """A tracer nobody has configured earns its list with starts (K and N lowered so that the test is short; the mode is not touched)."""
    import torch
    t = tracer_cls(WD, HT).init()
    try:
        t.set_beam_refine_after(1); t.set_beam_list_after(1)
        t.add_world(scene64[1])
        hits = torch.zeros((WD * HT, 4), dtype=torch.int32, device="cuda")
        for _ in range(6):
            t.draw_frame_device(view(0), hits.data_ptr(), 0)
            torch.cuda.synchronize()
        assert t.beam_cache_list_state() == 2 and t.beam_cache_starts_state() == 1 and t.beam_cache_start_counters() == (2, 0)
    finally:
        t.shutdown()


# ---- frames --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lockstep", [False, True], ids=["in_flight", "one_at_a_time"])
@pytest.mark.parametrize("after", [1, 3])
def test_search_fill_refine_count_build_adoption_packed_hits_from_the_starts(tracer_cls, scene64, lockstep, after):
    steps = frames(view(0), 5 + after) + [(wait,)] + frames(view(0), 4)
    log, _, _ = check(tracer_cls, world64(scene64), steps, lockstep=lockstep, after=after)
    if lockstep:
        assert log == resting(9 + after, after)
    states = [e[2] for e in log]
    assert states[:2 + after] == [0] * (2 + after) and states[2 + after] == 1 and states[-4:] == [2] * 4, states
    assert [e[4] for e in log][-4:] == [1] * 4 and log[-1][3] == 1 and log[-1][5] >= 4 and log[-1][6] == 0
    assert all(e[4] == (1 if e[2] else 0) for e in log)       # every launch that counts or walks packed has to do with the starts, no other


@pytest.mark.parametrize("rect", [CUT, SMALL], ids=["cut_on_all_sides", "areas_of_5_rows"])
def test_a_rectangle_whose_last_areas_and_wave_tiles_are_cut(tracer_cls, scene64, rect):
    log, _, _ = check(tracer_cls, world64(scene64), frames(view(2), 5, rect) + [(wait,)] + frames(view(2), 3, rect))
    assert [e[2] for e in log][-3:] == [2, 2, 2] and [e[4] for e in log][-3:] == [1, 1, 1] and log[-1][3] == 1


# ---- the starts as numbers -----------------------------------------------------------------------------------------------------------

def starts_probe(w, h):
    def probe(t):
        if t.beam_cache_list(w, h) is None:                   # (the twin: it never has a list)
            return None
        state, n_groups, entries, table, trips = t.beam_cache_list(w, h)
        fine_state, fine = t.beam_cache_fine()
        starts, restarts = t.beam_cache_starts(w, h)
        return dict(state=state, n_groups=n_groups, entries=entries, table=table, trips=trips, fine=fine, starts=starts, restarts=restarts, starts_state=t.beam_cache_starts_state())
    return probe


def host_walk(scene64, cam, rect, t0):
    """The walk compiled for the host from per-pixel start parameters: records and trips of every ray of the rectangle, from the root."""
    from tests import harness_ffi as H
    x0, y0, w, h = rect
    hk = H.HostKernel(scene64[1].nodes, scene64[1].sub_chunks)
    L = H.lib()
    L.hh_trace_rect_stats.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 3
    out, iters = np.zeros(w * h, dtype=H.HIT), np.zeros(w * h, dtype=np.uint32)
    cam, t0 = np.ascontiguousarray(cam), np.ascontiguousarray(t0, dtype=np.float32)
    L.hh_trace_rect_stats(hk.h, C.c_void_p(cam.ctypes.data), WD, HT, x0, y0, w, h, C.c_void_p(t0.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(iters.ctypes.data))
    return out, iters.reshape(h, w), hk.levels


def starts_errors(got, records, scene64, cam, rect):
    """Everything that is wrong with a downloaded list with starts, as strings.  records: the frame's, (h, w, 4) uint32.  Also -> a summary."""
    x0, y0, w, h = rect
    bad = list_errors(got["entries"], got["table"], got["n_groups"], got["fine"], got["restarts"], w, h)      # the list, sorted by the RESTARTED trips
    nx, _ = wave_grid(w, h)
    t0 = np.zeros((h, w), dtype=np.float32)                   # a pixel nobody lists: from the interval's start (its record is a miss either way)
    listed = np.zeros((h, w), dtype=bool)
    for a, exp in enumerate(expected_areas(got["fine"], got["restarts"], w, h)):
        xs, ys = (exp & 0xFFFF).astype(int), (exp >> 16).astype(int)
        place = {int(e): i for i, e in enumerate(got["entries"][a, :len(exp)].tolist())}
        if set(place) != set(exp.tolist()):
            continue                                          # (reported by list_errors)
        at = np.array([place[int(e)] for e in exp.tolist()], dtype=int)
        t0[ys, xs] = got["starts"][a, at]
        listed[ys, xs] = True
    hit = ((records[..., 3] >> 24) & 0xFF) == 1
    if (listed & hit).sum() != hit.sum():
        bad.append(f"{int((hit & ~listed).sum())} hit pixels that are not listed")
    t_bits = records[..., 0]
    wrong = listed & hit & (t0.view(np.uint32) != t_bits)
    if wrong.any():
        bad.append(f"{int(wrong.sum())} listed hit pixels whose start is not their record's t, bit for bit")
    ys, xs = np.mgrid[0:h, 0:w]
    bound = got["fine"][(ys // 8) * nx + xs // 8]
    miss = listed & ~hit
    if not np.isfinite(t0[miss]).all():
        bad.append(f"{int((~np.isfinite(t0[miss])).sum())} listed miss pixels whose start is not finite")
    if (t0[miss] < bound[miss]).any():
        bad.append(f"{int((t0[miss] < bound[miss]).sum())} listed miss pixels whose start is below their wave tile's finer bound")
    out, iters, levels = host_walk(scene64, cam, rect, t0)
    host_records = out.view(np.uint32).reshape(h, w, 4)
    if not np.array_equal(host_records, records):
        bad.append(f"the host walk from the starts differs from the frame in {int((host_records != records).any(axis=2).sum())} records")
    restarts = got["restarts"]
    if not np.array_equal(iters[listed], restarts[listed]):
        d = iters[listed].astype(int) - restarts[listed]
        bad.append(f"{int((d != 0).sum())} listed pixels whose restarted count is not the host's trips from their start (host - device: {np.unique(d).tolist()})")
    if restarts[listed].size and restarts[listed].max() > levels:
        bad.append(f"restarted counts above the tree's {levels} levels")
    if (restarts[listed & hit] != levels).any():
        bad.append("hit pixels whose restarted count is not `levels`")
    summary = (f"{int(listed.sum())} listed pixels, {int((listed & hit).sum())} hits; trips per listed ray {got['trips'][listed].mean() if listed.any() else 0:.2f} counted, "
               f"{restarts[listed].mean() if listed.any() else 0:.2f} restarted; restarted counts {np.bincount(restarts[listed], minlength=levels + 1).tolist()}")
    return bad, summary


@pytest.mark.parametrize("rect", [None, CUT, SMALL], ids=["whole_frame", "rectangle_cut_on_all_sides", "last_areas_5_pixels_wide"])
def test_the_starts_as_numbers(tracer_cls, scene64, rect):
    """Every listed hit pixel's start is its record's t, bit for bit; every listed miss pixel's is finite and not below its wave tile's finer
    bound; the walk compiled for the host, started from the downloaded starts, reproduces the frame's records in exactly the downloaded
    restarted trips, none above `levels` — read behind the launch that built the list and behind a packed launch."""
    cam = view(1)
    x0, y0, w, h = rect or (0, 0, WD, HT)
    built = {}

    def after_build(t):
        built["got"] = starts_probe(w, h)(t)

    log, want, packed = check(tracer_cls, world64(scene64), frames(cam, 4, rect) + [(after_build,)] + frames(cam, 3, rect), lockstep=True, probe=starts_probe(w, h))
    assert log == resting(7)
    records = want[-1][0].cpu().numpy().view(np.uint32).reshape(h, w, 4)
    for name, got in (("behind its build", built["got"]), ("behind a packed launch", packed)):
        assert got["state"] == (1 if name == "behind its build" else 2) and got["starts_state"] == 1
        errors, summary = starts_errors(got, records, scene64, cam, (x0, y0, w, h))
        print(name + ":", summary)
        assert not errors, f"{name}: " + "; ".join(errors[:6])
    assert np.array_equal(built["got"]["entries"], packed["entries"]) and np.array_equal(built["got"]["starts"].view(np.uint32), packed["starts"].view(np.uint32)), \
        "the list and its starts are built once"              # (as bits: a padding slot's start is whatever the memory held)
    hit = ((records[..., 3] >> 24) & 0xFF) == 1
    assert hit.sum() > 500 and (~hit).sum() > 500
    assert len(np.unique(packed["restarts"])) > 2, "the restarted counts say nothing"


def test_the_checks_catch_a_start_that_is_off_by_one_ulp_and_a_miss_below_its_bound(tracer_cls, scene64):
    cam = view(1)
    log, want, got = check(tracer_cls, world64(scene64), frames(cam, 5), lockstep=True, probe=starts_probe(WD, HT))
    records = want[-1][0].cpu().numpy().view(np.uint32).reshape(HT, WD, 4)
    assert not starts_errors(got, records, scene64, cam, (0, 0, WD, HT))[0]
    hit = ((records[..., 3] >> 24) & 0xFF) == 1
    want_areas = expected_areas(got["fine"], got["restarts"], WD, HT)
    a = int(np.argmax([len(e) for e in want_areas]))
    e = got["entries"][a]
    is_hit = hit[(e[:len(want_areas[a])] >> 16).astype(int), (e[:len(want_areas[a])] & 0xFFFF).astype(int)]
    assert is_hit.any()
    k = int(np.argmax(is_hit))
    off = dict(got, starts=got["starts"].copy())
    off["starts"][a, k] = np.nextafter(off["starts"][a, k], np.float32(np.inf))
    assert any("is not their record's t" in s for s in starts_errors(off, records, scene64, cam, (0, 0, WD, HT))[0])
    if (~is_hit).any():
        k = int(np.argmax(~is_hit))
        low = dict(got, starts=got["starts"].copy())
        low["starts"][a, k] = 0.0
        assert any("below their wave tile's finer bound" in s for s in starts_errors(low, records, scene64, cam, (0, 0, WD, HT))[0])


# ---- edge views ----------------------------------------------------------------------------------------------------------------------

def test_an_all_sky_view_has_an_empty_table(tracer_cls, scene64):
    log, want, got = check(tracer_cls, world64(scene64), frames(SKY, 7), lockstep=True, probe=starts_probe(WD, HT))
    assert log == resting(7)
    assert got["state"] == 2 and got["n_groups"] == 0 and not got["table"].any() and (got["fine"] >= NONE).all()
    assert not ((want[-1][0][:, 3] >> 24) & 0xFF).cpu().numpy().any()


def test_a_view_where_every_pixel_hits(tracer_cls, scene64):
    log, want, got = check(tracer_cls, world64(scene64), frames(DOWN, 7), lockstep=True, probe=starts_probe(WD, HT))
    assert log == resting(7)
    records = want[-1][0].cpu().numpy().view(np.uint32).reshape(HT, WD, 4)
    assert (((records[..., 3] >> 24) & 0xFF) == 1).all() and (got["fine"] < NONE).all()
    errors, summary = starts_errors(got, records, scene64, DOWN, (0, 0, WD, HT))
    print(summary)
    assert not errors, "; ".join(errors[:6])
    assert len(np.unique(got["restarts"])) == 1               # `levels` everywhere: the list is in pixel order


# ---- the start key, drops, two views ---------------------------------------------------------------------------------------------------

def test_another_jitter_on_the_packed_hits_walks_the_list_from_the_finer_bounds_and_the_starts_return(tracer_cls, scene64):
    """The start key holds the jitter (a ray's own start is that ray's): a jittered frame of the view walks the same list from the finer
    bounds — no second build, the list's state unchanged — and at the counted jitter the starts serve again.  (tmin and tmax, the key's
    other two words, are constants of the library, BLOK_RAY_TMIN / _TMAX: no launch can change them; tests/test_own_start_host.py changes
    their bits in the policy.)"""
    steps = frames(view(4), 5) + [(wait,)]
    for j in ((0.31, -0.22), (-0.45, 0.4), (0.0, 0.0), (0.49, 0.49), (0.0, 0.0)):
        steps += [(lambda t, j=j: t.set_taa_jitter(j),)] + frames(view(4), 2)
    log, want, _ = check(tracer_cls, world64(scene64), steps)
    tail = log[-10:]
    assert [e[2] for e in tail] == [2] * 10 and log[-1][3] == 1
    assert [e[4] for e in tail] == [2, 2, 2, 2, 1, 1, 2, 2, 1, 1], [e[4] for e in tail]
    used, other = tail[0][5], tail[0][6]
    assert [e[5] - used for e in tail] == [0, 0, 0, 0, 1, 2, 2, 2, 3, 4] and [e[6] - other for e in tail] == [0, 1, 2, 3, 3, 3, 4, 5, 5, 5]
    assert not bool((want[5][0] == want[7][0]).all()), "the jitter changes nothing in this view"


def test_a_list_counted_under_a_jitter_serves_that_jitter(tracer_cls, scene64):
    steps = [(lambda t: t.set_taa_jitter((0.31, -0.22)),)] + frames(view(4), 5) + [(wait,)] + frames(view(4), 2)
    steps += [(lambda t: t.set_taa_jitter((0.0, 0.0)),)] + frames(view(4), 2) + [(lambda t: t.set_taa_jitter((0.31, -0.22)),)] + frames(view(4), 2)
    log, _, _ = check(tracer_cls, world64(scene64), steps)
    assert [e[4] for e in log][-6:] == [1, 1, 2, 2, 1, 1] and log[-1][3] == 1


def test_a_world_change_and_a_view_change_drop_the_starts_with_the_list(tracer_cls, scene64):
    """tests/test_beam_list_gpu.py's scenario: one ulp of one camera float is another view (it searches; the view itself still has its list
    and its starts when the camera returns); a rebuilt tree and a replaced world start the view over, and its new list has new starts."""
    cam = view(1)
    mats = W.scene_materials(SEED)

    def ball(t):
        t.volume_apply_brush((32.0, 42.0, 32.0), 8.0, 1.0, 0)
        t.volume_rebuild(mats)

    steps = frames(cam, 6)
    steps += [("frame", one_ulp(cam, 0), None), ("frame", cam, None)]
    steps += [(ball,)] + frames(cam, 6)
    steps += [(lambda t: t.add_world(scene64[1]),)] + frames(cam, 6)
    log, want, _ = check(tracer_cls, volume64, steps, lockstep=True)
    assert log[:6] == resting(6)
    assert log[6][:5] == (0, 0, 0, 1, 0) and log[7][:5] == (2, 2, 2, 1, 1)
    assert [e[:3] + e[4:5] for e in log[8:14]] == [e[:3] + e[4:5] for e in resting(6)] and log[13][3] == 2
    assert [e[:3] + e[4:5] for e in log[14:20]] == [e[:3] + e[4:5] for e in resting(6)] and log[19][3] == 3
    assert all(e[6] == 0 for e in log)
    before, behind = want[5][1].cpu().numpy(), want[13][1].cpu().numpy()
    assert (before != behind).any(), "the edit is not seen from this view"


def test_two_views_alternating_each_walk_from_their_own_starts(tracer_cls, scene64):
    a, b = view(0), view(3)
    steps = frames(a, 5) + [(wait,)] + frames(b, 5) + [(wait,)]
    for _ in range(4):
        steps += [("frame", a, None), ("frame", b, None)]
    log, _, _ = check(tracer_cls, world64(scene64), steps)
    assert [e[2] for e in log][-8:] == [2] * 8 and [e[4] for e in log][-8:] == [1] * 8 and log[-1][3] == 2 and log[-1][6] == 0
