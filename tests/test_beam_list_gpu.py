"""The packed walk of a view at rest (blok_amd/csrc/hip/beam_cache.h: plan_beam_list; api_launch.hip; trace_count_kernel, pack_build_kernel,
packed_walk_kernel), by tests/test_beam_refine_gpu.py's method: every frame of every scenario is compared byte for byte, records and RGBA8,
with the same launches made by a twin tracer whose cache is switched off — into output buffers filled with a garbage pattern before every
launch, so a pixel no wave walked or wrote shows (an entry dropped from a list) — over three streams, with and without a synchronisation
between the launches.  The list itself is checked as numbers from its download: the listed pixels, their order, the padding, the table, and
the counts against the walk compiled for the host (tests/host_harness).  Frames of 200 x 136 over the 64^3 scene."""
import ctypes as C

import numpy as np
import pytest

from blok_amd import world as W
from tests.conftest import SEED
from tests.test_beam_cache_gpu import GARBAGE, HT, WD, one_ulp, view, volume64
from tests.test_beam_refine_gpu import CUT, NONE, Runner, frames, wave_grid, world64

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF                                         # trace_kernels.h: kPackPad
AREA, GROUPS, KEY_SHIFT = 32, 16, 20                     # kPackArea (as the library reports it: tracer_cls), kPackGroups = area^2 / 64, kPackKeyShift
SMALL = (37, 19, 69, 69)                                 # 64 + 5 pixels a side: the last areas are 5 pixels wide or high, the corner area 5 x 5 (areas of 32 or of 64 pixels)
SKY = W.camera_look_at((32.0, 80.0, 32.0), (32.0, 200.0, 32.3), 60.0, WD, HT)      # above the world, looking up: no beam tile is live
DOWN = W.camera_look_at((32.0, 30.0, 32.0), (32.0, 0.0, 32.3), 60.0, WD, HT)       # over the ground, looking down: every pixel hits


@pytest.fixture(scope="module")
def tracer_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from blok_amd import _ffi
    from blok_amd.tracer import HipTracer
    global AREA, GROUPS
    AREA = int(_ffi.hip_lib().blok_hip_pack_area())
    GROUPS = AREA * AREA // 64
    return HipTracer


class ListRunner(Runner):
    """Runner, with the list's state in the log: per frame (action, fine state, list state, builds so far)."""

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
            log.append((self.tr.beam_cache_last_action(), self.tr.beam_cache_fine_state(), self.tr.beam_cache_list_state(), self.tr.beam_cache_list_builds()))
            if lockstep:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return frames_, log


def wait(t):
    """A step that does nothing: the runner synchronises in front of it, so a build in flight has finished."""


def check(tracer_cls, setup, steps, lockstep=False, after=1, probe=None):
    """Runs the steps on the twin (cache off) and on the tracer under test (packed walk on, K = 1, N = after), one after the other, and
    compares every frame.  -> the log of the tracer under test, the twin's frames, and what probe(tracer under test) returned at the end."""
    import torch
    on, off = tracer_cls(WD, HT).init(), tracer_cls(WD, HT).init()
    off.set_beam_cache(False)
    on.set_beam_cache(3); on.set_beam_refine_after(1); on.set_beam_list_after(after)
    for t in (on, off):
        setup(t)
    on, off = ListRunner(on, WD, HT), ListRunner(off, WD, HT)
    try:
        want, ref_log = off.run(steps, lockstep)
        got, log = on.run(steps, lockstep)
        assert all(entry == (0, 0, 0, 0) for entry in ref_log), "a tracer with the cache off never hits, refines or builds"
        assert len(got) == len(want)
        for k, ((gh, gc), (wh, wc)) in enumerate(zip(got, want)):
            assert torch.equal(gh, wh), f"frame {k} {log[k]}: records differ in {int((gh != wh).any(dim=1).sum())} pixels"
            assert torch.equal(gc, wc), f"frame {k} {log[k]}: RGBA8 differs in {int((gc != wc).sum())} pixels"
            assert not bool((wc == GARBAGE).any()), f"frame {k}: the reference left pixels unwritten"
        return log, want, (probe(on.tr) if probe else None)
    finally:
        on.close(); off.close()


def resting(n, after=1):
    """The log of n launches of one view, one at a time: a search, a fill, the hit that refines, `after` - 1 hits from the finer bounds, the
    hit that counts and builds, packed hits (the build has finished when the next launch asks)."""
    out = []
    for k in range(n):
        action = min(k, 2)
        fine = 0 if k < 2 else 1 if k == 2 else 2
        lst = 0 if k < 2 + after else 1 if k == 2 + after else 2
        out.append((action, fine, lst, 1 if k >= 2 + after else 0))
    return out


# ---- the list as numbers -------------------------------------------------------------------------------------------------------------

def expected_areas(fine, trips, w, h):
    """Per area of the rectangle, row-major: its listed pixels (those of the wave tiles with a finite finer bound, inside the rectangle) by
    descending trip count, stable in pixel order (wave tile by wave tile, row by row inside one), as entries x | y << 16."""
    nx, _ = wave_grid(w, h)
    out = []
    for ay in range(0, h, AREA):
        for ax in range(0, w, AREA):
            ys, xs = np.mgrid[ay:min(ay + AREA, h), ax:min(ax + AREA, w)]
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            pixel_order = np.lexsort((xs, ys, xs // 8, ys // 8))
            ys, xs = ys[pixel_order], xs[pixel_order]
            listed = fine[(ys // 8) * nx + xs // 8] < NONE
            ys, xs = ys[listed], xs[listed]
            order = np.argsort(-trips[ys, xs].astype(np.int64), kind="stable")
            out.append((xs[order] | (ys[order] << 16)).astype(np.uint32))
    return out


def list_errors(entries, table, n_groups, fine, trips, w, h):
    """Everything that is wrong with a downloaded list, as strings (none: the list is what trace_kernels.h says it is)."""
    bad = []
    want = expected_areas(fine, trips, w, h)
    if len(want) != len(entries):
        return [f"{len(entries)} areas, expected {len(want)}"]
    words = []
    for a, exp in enumerate(want):
        n = len(exp)
        padded = (n + 63) // 64 * 64
        got = entries[a, :n]
        if sorted(got.tolist()) != sorted(exp.tolist()):
            missing, extra = set(exp.tolist()) - set(got.tolist()), set(got.tolist()) - set(exp.tolist())
            doubled = n - len(set(got.tolist()))
            bad.append(f"area {a}: {len(missing)} listed pixels missing, {len(extra)} entries that are no listed pixel, {doubled} entries doubled")
        elif not np.array_equal(got, exp):
            t = trips[got >> 16, got & 0xFFFF].astype(int)
            bad.append(f"area {a}: " + ("counts not descending" if (np.diff(t) > 0).any() else "equal counts not in pixel order"))
        if not (entries[a, n:padded] == PAD).all():
            bad.append(f"area {a}: entries {n}..{padded} are not all padding")
        if (got == PAD).any():
            bad.append(f"area {a}: padding before the end of the stretch")
        for g in range(padded // 64):
            words.append(((int(trips[exp[g * 64] >> 16, exp[g * 64] & 0xFFFF]) + 1) << KEY_SHIFT) | (a * GROUPS + g))
    if n_groups != len(words):
        bad.append(f"{n_groups} groups in the table, expected {len(words)}")
    if table[:n_groups].tolist() != sorted(words, reverse=True):
        keys = table[:n_groups] >> KEY_SHIFT
        bad.append("table keys not descending" if (np.diff(keys.astype(int)) > 0).any() else "table words are not the groups' (largest count + 1, index)")
    if table[n_groups:].any():
        bad.append("words behind the table's last group are not 0")
    return bad


def list_probe(w, h):
    def probe(t):
        got = t.beam_cache_list(w, h)
        if got is None:                                       # (the twin: it never has a list)
            return None
        state, n_groups, entries, table, trips = got
        fine_state, fine = t.beam_cache_fine()
        return state, n_groups, entries, table, trips, fine_state, fine
    return probe


def host_trips(scene64, cam, rect, fine):
    """The walk compiled for the host: trips of every ray of the rectangle from the root, started behind its wave tile's finer bound."""
    from tests import harness_ffi as H
    x0, y0, w, h = rect
    nx, _ = wave_grid(w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    t0 = np.ascontiguousarray(np.where(fine[(ys // 8) * nx + xs // 8] < NONE, fine[(ys // 8) * nx + xs // 8], 0.0), dtype=np.float32)
    hk = H.HostKernel(scene64[1].nodes, scene64[1].sub_chunks)
    L = H.lib()
    L.hh_trace_rect_stats.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 3
    out, iters = np.zeros(w * h, dtype=H.HIT), np.zeros(w * h, dtype=np.uint32)
    cam = np.ascontiguousarray(cam)
    L.hh_trace_rect_stats(hk.h, C.c_void_p(cam.ctypes.data), WD, HT, x0, y0, w, h, C.c_void_p(t0.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(iters.ctypes.data))
    return iters.reshape(h, w), hk.levels


@pytest.mark.parametrize("rect", [None, CUT, SMALL], ids=["whole_frame", "rectangle_cut_on_all_sides", "an_area_with_fewer_than_64_listed_pixels"])
def test_the_list_as_numbers(tracer_cls, scene64, rect):
    """Every pixel of every wave tile with a finite finer bound exactly once, no other pixel, padding only at the end of a stretch, counts
    descending inside an area and stable in pixel order, the table's keys descending and equal to the groups' maxima — the same list read
    behind the launch that built it and behind a packed launch.  The counts EQUAL the host's: the trips of walk_loop from the root for the same
    rays from the same start parameters, saturated at 255 (the device enters a wave's rays together, walk_enter_wave, and counts the descents
    it shares as the trips of the walk from the root that they are)."""
    cam = view(1)
    x0, y0, w, h = rect or (0, 0, WD, HT)
    built = {}

    def after_build(t):
        built["list"] = list_probe(w, h)(t)

    log, _, packed = check(tracer_cls, world64(scene64), frames(cam, 4, rect) + [(after_build,)] + frames(cam, 3, rect), lockstep=True, probe=list_probe(w, h))
    assert log == resting(7)
    for name, (state, n_groups, entries, table, trips, fine_state, fine) in (("behind its build", built["list"]), ("behind a packed launch", packed)):
        assert state == (1 if name == "behind its build" else 2) and fine_state == 2
        errors = list_errors(entries, table, n_groups, fine, trips, w, h)
        assert not errors, f"{name}: " + "; ".join(errors[:5])
    assert np.array_equal(built["list"][2], packed[2]) and np.array_equal(built["list"][3], packed[3]), "the list is built once"
    state, n_groups, entries, table, trips, _, fine = packed
    listed = [len(a) for a in expected_areas(fine, trips, w, h)]
    print(f"{len(listed)} areas, {sum(1 for n in listed if n)} with listed pixels, {sum(listed)} listed pixels in {n_groups} groups, fewest in an area {min(n for n in listed if n)}")
    assert n_groups > 0 and sum(listed) < w * h
    if rect == SMALL:
        assert any(0 < n < 64 for n in listed), "no area with fewer than 64 listed pixels"
    host, levels = host_trips(scene64, cam, (x0, y0, w, h), fine)
    nx, ny = wave_grid(w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    on = fine[(ys // 8) * nx + xs // 8] < NONE
    want = np.minimum(host, 255)
    print("host's trips minus the device's, listed pixels:", np.bincount(np.abs(want.astype(int) - trips)[on].clip(0, 8)).tolist(), "largest count", int(trips[on].max()),
          "saturated", int((trips[on] == 255).sum()))
    assert np.array_equal(trips[on], want[on]), f"{int((trips != want)[on].sum())} listed pixels whose count is not the host's"
    assert len(np.unique(trips[on])) > 8, "the counts say nothing"


def test_a_second_count_of_the_same_view_gives_the_same_trips_and_the_same_list(tracer_cls, scene64):
    """The view loses its list (the cache is cleared) and earns it again, this time counted by its third launch from the finer bounds and
    with three frames in flight: the trips, the list and the table are the first build's, byte for byte."""
    cam = view(1)
    first = {}

    def keep(t):
        first["list"] = list_probe(WD, HT)(t)

    def again(t):
        if t.beam_cache_list_builds():                        # (not the twin: its cache stays off)
            t.set_beam_cache(3); t.set_beam_list_after(3)

    steps = frames(cam, 4) + [(wait,)] + frames(cam, 1) + [(keep,), (again,)] + frames(cam, 8) + [(wait,)] + frames(cam, 2)
    log, _, second = check(tracer_cls, world64(scene64), steps, probe=list_probe(WD, HT))
    assert log[-1][2:] == (2, 2) and first["list"][0] == 2 and second[0] == 2
    for name, a, b in zip(("groups", "entries", "table", "trips"), first["list"][1:5], second[1:5]):
        assert np.array_equal(a, b), f"the second build's {name} differ from the first's"
    assert not list_errors(second[2], second[3], second[1], second[6], second[4], WD, HT)


def test_the_checks_catch_a_dropped_and_a_doubled_entry(tracer_cls, scene64):
    """The mutations the list must not survive: an entry dropped (its place taken by padding, or by its neighbour) and an entry doubled are
    both reported by list_errors on an otherwise good list."""
    cam = view(1)
    w, h = SMALL[2], SMALL[3]                                 # (cut wave tiles: areas whose last group has padding)
    _, _, (state, n_groups, entries, table, trips, _, fine) = check(tracer_cls, world64(scene64), frames(cam, 5, SMALL), lockstep=True, probe=list_probe(w, h))
    assert state == 2 and not list_errors(entries, table, n_groups, fine, trips, w, h)
    a = int(np.argmax([len(e) for e in expected_areas(fine, trips, w, h)]))      # (the stretch of an area without listed pixels is undefined)
    dropped = entries.copy(); dropped[a, 5] = PAD
    assert any("missing" in e for e in list_errors(dropped, table, n_groups, fine, trips, w, h))
    shifted = entries.copy(); shifted[a, 5] = shifted[a, 6]
    errors = list_errors(shifted, table, n_groups, fine, trips, w, h)
    assert any("1 listed pixels missing" in e and "1 entries doubled" in e for e in errors), errors
    want = expected_areas(fine, trips, w, h)
    ragged = [k for k, e in enumerate(want) if len(e) % 64]
    assert ragged, "no area whose last group has padding"
    b = ragged[0]
    doubled = entries.copy(); doubled[b, len(want[b])] = doubled[b, 0]      # one entry more than the area has pixels, in the padding: a pixel walked twice
    errors = list_errors(doubled, table, n_groups, fine, trips, w, h)
    assert any("are not all padding" in e for e in errors), errors


# ---- frames --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lockstep", [False, True], ids=["in_flight", "one_at_a_time"])
@pytest.mark.parametrize("after", [1, 3])
def test_search_fill_hits_refine_count_build_adoption_packed_hits(tracer_cls, scene64, lockstep, after):
    """Three frames in flight (nobody waits for the build: launches go on walking from the finer bounds until one finds it finished), and
    one frame at a time.  A synchronisation in the middle makes the adoption certain for the frames behind it."""
    steps = frames(view(0), 5 + after) + [(wait,)] + frames(view(0), 4)
    log, _, _ = check(tracer_cls, world64(scene64), steps, lockstep=lockstep, after=after)
    if lockstep:
        assert log == resting(9 + after, after)
    states = [e[2] for e in log]
    assert states[:2 + after] == [0] * (2 + after) and states[2 + after] == 1 and states[-4:] == [2] * 4, states
    assert all(s in (0, 2) for s in states[3 + after:]) and sorted(states[3 + after:]) == states[3 + after:], states      # plain hits, then packed hits
    assert log[-1][3] == 1                                    # one build


@pytest.mark.parametrize("rect", [CUT, SMALL], ids=["cut_on_all_sides", "areas_of_5_rows"])
def test_a_rectangle_whose_last_areas_and_wave_tiles_are_cut(tracer_cls, scene64, rect):
    log, _, _ = check(tracer_cls, world64(scene64), frames(view(2), 5, rect) + [(wait,)] + frames(view(2), 3, rect))
    assert [e[2] for e in log][-3:] == [2, 2, 2] and log[-1][3] == 1


def test_an_all_sky_view_has_an_empty_table_and_the_fill_writes_everything(tracer_cls, scene64):
    log, want, (state, n_groups, entries, table, trips, _, fine) = check(tracer_cls, world64(scene64), frames(SKY, 7), lockstep=True, probe=list_probe(WD, HT))
    assert log == resting(7)
    assert state == 2 and n_groups == 0 and not table.any() and (fine >= NONE).all()
    hit = ((want[-1][0][:, 3] >> 24) & 0xFF).cpu().numpy()
    assert not hit.any()


def test_a_view_where_every_pixel_hits(tracer_cls, scene64):
    log, want, (state, n_groups, entries, table, trips, _, fine) = check(tracer_cls, world64(scene64), frames(DOWN, 7), lockstep=True, probe=list_probe(WD, HT))
    assert log == resting(7)
    hit = ((want[-1][0][:, 3] >> 24) & 0xFF).cpu().numpy()
    assert hit.all() and (fine < NONE).all()
    assert state == 2 and n_groups == sum((min(AREA, WD - ax) * min(AREA, HT - ay) + 63) // 64 for ay in range(0, HT, AREA) for ax in range(0, WD, AREA))
    assert not list_errors(entries, table, n_groups, fine, trips, WD, HT)


def test_two_views_alternating_each_walk_their_own_list(tracer_cls, scene64):
    a, b = view(0), view(3)
    steps = frames(a, 5) + [(wait,)] + frames(b, 5) + [(wait,)]
    for _ in range(4):
        steps += [("frame", a, None), ("frame", b, None)]
    log, _, _ = check(tracer_cls, world64(scene64), steps)
    assert [e[2] for e in log][-8:] == [2] * 8 and log[-1][3] == 2


def test_a_world_change_and_a_view_change_in_the_middle_drop_the_list(tracer_cls, scene64):
    """The brush adds a ball above the scene: wave tiles that were empty become live, so a list kept across the edit would leave their pixels
    to nobody (the garbage shows) — the list goes with the finer bounds it lists the pixels of, and the view earns a new one.  One ulp of
    one camera float is another view: it searches; the view itself still has its list when the camera returns."""
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
    assert log[6][:3] == (0, 0, 0) and log[7][:3] == (2, 2, 2)
    assert [e[:3] for e in log[8:14]] == [e[:3] for e in resting(6)] and log[13][3] == 2      # a rebuilt tree: search, fill, refine, count, packed — nothing of the old tree's
    assert [e[:3] for e in log[14:20]] == [e[:3] for e in resting(6)] and log[19][3] == 3      # a replaced world: the same
    before, behind = want[5][1].cpu().numpy(), want[13][1].cpu().numpy()
    assert (before != behind).any(), "the edit is not seen from this view"


def test_non_zero_jitter_on_the_packed_hits_the_list_survives_it(tracer_cls, scene64):
    """The key does not hold the jitter (the searches cover every sub-pixel offset), so a jittered frame of the view hits, walks packed from a
    list counted under another jitter — stale, never wrong — and no second build is made."""
    steps = frames(view(4), 5) + [(wait,)]
    for j in ((0.31, -0.22), (-0.45, 0.4), (0.0, 0.0), (0.49, 0.49)):
        steps += [(lambda t, j=j: t.set_taa_jitter(j),)] + frames(view(4), 2)
    log, want, _ = check(tracer_cls, world64(scene64), steps)
    assert [e[2] for e in log][-8:] == [2] * 8 and log[-1][3] == 1
    assert not bool((want[5][0] == want[7][0]).all()), "the jitter changes nothing in this view"
