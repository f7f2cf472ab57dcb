"""Mode 5 of the beam cache: every listed ray of a view at rest re-enters at the node its restarted walk ends in (blok_amd/csrc/hip/beam_cache.h;
trace_core.h: restart_node_word, walk_enter_node; trace_count_own_kernel, pack_starts_nodes_kernel, packed_frame_node_kernel), by
tests/test_own_start_gpu.py's method and on its frames (200 x 136 over the 64^3 scene): every frame of every scenario is compared byte for
byte, records and RGBA8, with the same launches made by a twin tracer whose cache is switched off, into buffers filled with garbage; the
node words are checked as numbers from their download — against the frame's records, the downloaded tree descended on the host, and the
count launch's side compiled for the host (tests/host_harness/node_restart_shim.cpp) over that tree."""
import numpy as np
import pytest

from blok_amd import world as W
from tests.conftest import SEED
from tests.test_beam_cache_gpu import GARBAGE, HT, WD, view, volume64
from tests.test_beam_refine_gpu import CUT, frames, world64
from tests.test_beam_list_gpu import SMALL, expected_areas, wait
from tests.test_own_start_gpu import OwnRunner, resting, starts_probe
from tests.test_own_start_gpu import tracer_cls      # noqa: F401  (the fixture: it also sets the list module's area)
from tests.test_brick_restart_host import HIT, NONE, HostWorld, shim, word_errors

pytestmark = pytest.mark.gpu

INSIDE = W.camera_look_at((30.3, 52.7, 33.1), (9.0, 11.0, 14.0), 70.0, WD, HT)      # tests/test_own_start_host.py: inside the world box, rays start at tmin


class NodeRunner(OwnRunner):
    """OwnRunner, with the node kernel's launches in the log: per frame OwnRunner's seven and (launches of packed_frame_node_kernel so far)."""

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
                        self.tr.beam_cache_starts_state()) + self.tr.beam_cache_start_counters() + (self.tr.beam_cache_node_counter(),))
            if lockstep:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return frames_, log


def check(tracer_cls, setup, steps, lockstep=False, after=1, probe=None, mode=5, size=(WD, HT)):
    """Runs the steps on the twin (cache off) and on the tracer under test (`mode`, K = 1, N = after), one after the other, and compares
    every frame.  -> the log of the tracer under test, the twin's frames, and what probe(tracer under test) returned at the end."""
    import torch
    on, off = tracer_cls(*size).init(), tracer_cls(*size).init()
    off.set_beam_cache(False)
    on.set_beam_cache(mode); on.set_beam_refine_after(1); on.set_beam_list_after(after)
    for t in (on, off):
        setup(t)
    on, off = NodeRunner(on, *size), NodeRunner(off, *size)
    try:
        want, ref_log = off.run(steps, lockstep)
        got, log = on.run(steps, lockstep)
        assert all(entry == (0,) * 8 for entry in ref_log), "a tracer with the cache off never hits, refines, builds, has starts or node words"
        assert len(got) == len(want)
        for k, ((gh, gc), (wh, wc)) in enumerate(zip(got, want)):
            assert torch.equal(gh, wh), f"frame {k} {log[k]}: records differ in {int((gh != wh).any(dim=1).sum())} pixels"
            assert torch.equal(gc, wc), f"frame {k} {log[k]}: RGBA8 differs in {int((gc != wc).sum())} pixels"
            assert not bool((wc == GARBAGE).any()), f"frame {k}: the reference left pixels unwritten"
        return log, want, (probe(on.tr) if probe else None)
    finally:
        on.close(); off.close()


def node_launches(log):
    """Per frame: did it run packed_frame_node_kernel?"""
    counts = [0] + [e[7] for e in log]
    return [b - a for a, b in zip(counts, counts[1:])]


def test_the_default_is_mode_5(tracer_cls, scene64):
    """A tracer nobody has configured earns its list with starts and node words (K and N lowered so that the test is short; the mode is not touched)."""
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
        assert t.beam_cache_has_nodes() and t.beam_cache_node_counter() == 2
    finally:
        t.shutdown()


# ---- frames --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lockstep", [False, True], ids=["in_flight", "one_at_a_time"])
@pytest.mark.parametrize("after", [1, 3])
def test_the_resting_sequence_ends_in_the_node_kernel(tracer_cls, scene64, lockstep, after):
    steps = frames(view(0), 5 + after) + [(wait,)] + frames(view(0), 4)
    log, _, _ = check(tracer_cls, world64(scene64), steps, lockstep=lockstep, after=after)
    if lockstep:
        assert [e[:7] for e in log] == resting(9 + after, after)
    assert [e[2] for e in log][-4:] == [2] * 4 and [e[4] for e in log][-4:] == [1] * 4 and log[-1][3] == 1
    ran = node_launches(log)
    assert ran[-4:] == [1] * 4 and ran[:3 + after] == [0] * (3 + after), ran
    assert log[-1][7] == log[-1][5], "every launch from the starts is a launch of the node kernel"


@pytest.mark.parametrize("rect", [CUT, SMALL], ids=["offset_37_19_width_101", "areas_of_5_rows"])
def test_a_rectangle_with_an_offset_whose_width_is_a_multiple_of_neither_8_nor_64(tracer_cls, scene64, rect):
    assert rect[0] and rect[1] and rect[2] % 8 and rect[2] % 64
    log, _, _ = check(tracer_cls, world64(scene64), frames(view(2), 5, rect) + [(wait,)] + frames(view(2), 3, rect))
    assert [e[2] for e in log][-3:] == [2, 2, 2] and node_launches(log)[-3:] == [1, 1, 1] and log[-1][3] == 1


def test_a_camera_inside_the_world_whose_rays_start_at_tmin(tracer_cls, scene64):
    log, want, _ = check(tracer_cls, world64(scene64), frames(INSIDE, 5) + [(wait,)] + frames(INSIDE, 3))
    assert node_launches(log)[-3:] == [1, 1, 1]
    hit = ((want[-1][0][:, 3] >> 24) & 0xFF).cpu().numpy() == 1
    assert hit.sum() > 5000


def test_another_jitter_walks_from_the_finer_bounds_and_the_node_kernel_returns_with_the_counted_one(tracer_cls, scene64):
    steps = frames(view(4), 5) + [(wait,)]
    for j in ((0.31, -0.22), (0.0, 0.0), (0.49, 0.49), (0.0, 0.0)):
        steps += [(lambda t, j=j: t.set_taa_jitter(j),)] + frames(view(4), 2)
    log, _, _ = check(tracer_cls, world64(scene64), steps)
    tail = log[-8:]
    assert [e[2] for e in tail] == [2] * 8 and log[-1][3] == 1
    assert [e[4] for e in tail] == [2, 2, 1, 1, 2, 2, 1, 1], [e[4] for e in tail]
    assert node_launches(log)[-8:] == [0, 0, 1, 1, 0, 0, 1, 1]


def test_a_volume_edit_and_a_re_upload_drop_the_words_with_the_list_and_a_new_count_follows(tracer_cls, scene64):
    cam = view(1)
    mats = W.scene_materials(SEED)

    def ball(t):
        t.volume_apply_brush((32.0, 42.0, 32.0), 8.0, 1.0, 0)
        t.volume_rebuild(mats)

    steps = frames(cam, 6) + [(ball,)] + frames(cam, 6) + [(lambda t: t.add_world(scene64[1]),)] + frames(cam, 6)
    log, want, _ = check(tracer_cls, volume64, steps, lockstep=True)
    for k in range(3):
        part = log[6 * k:6 * k + 6]
        assert [e[:3] + e[4:5] for e in part] == [e[:3] + e[4:5] for e in resting(6)] and part[-1][3] == k + 1
        assert node_launches(log)[6 * k:6 * k + 6] == [0, 0, 0, 0, 1, 1]
    assert (want[5][1].cpu().numpy() != want[11][1].cpu().numpy()).any(), "the edit is not seen from this view"


def test_four_views_alternating_each_from_their_own_words(tracer_cls, scene64):
    views = [view(0), view(3), view(5), INSIDE]
    steps = []
    for v in views:
        steps += frames(v, 5) + [(wait,)]
    for _ in range(3):
        steps += [("frame", v, None) for v in views]
    log, _, _ = check(tracer_cls, world64(scene64), steps)
    assert [e[2] for e in log][-12:] == [2] * 12 and [e[4] for e in log][-12:] == [1] * 12 and log[-1][3] == 4 and log[-1][6] == 0
    assert node_launches(log)[-12:] == [1] * 12


def test_a_resize_drops_the_words_and_the_view_earns_them_again(tracer_cls, scene64):
    big = (WD + 56, HT + 40)
    rect = (0, 0, WD, HT)
    steps = frames(view(0), 5, rect) + [(wait,)] + frames(view(0), 2, rect)
    steps += [(lambda t: t.resize(*big),)] + frames(view(0), 5, rect) + [(wait,)] + frames(view(0), 2, rect)
    steps += [(lambda t: t.resize(WD, HT),)] + frames(view(0), 5, rect) + [(wait,)] + frames(view(0), 2, rect)
    log, _, _ = check(tracer_cls, world64(scene64), steps, lockstep=True)
    ran = node_launches(log)
    for k in range(3):
        assert ran[7 * k:7 * k + 7] == [0, 0, 0, 0, 1, 1, 1], (k, ran)
    assert log[-1][3] == 3


def test_mode_4_set_explicitly_still_runs_the_own_start_kernel(tracer_cls, scene64):
    steps = frames(view(0), 6) + [(wait,)] + frames(view(0), 4)
    log, _, has = check(tracer_cls, world64(scene64), steps, lockstep=True, mode=4, probe=lambda t: t.beam_cache_has_nodes())
    assert [e[:7] for e in log] == resting(10)
    assert log[-1][5] >= 5 and log[-1][7] == 0 and not has, "mode 4 launched the node kernel"


def small_world(n):
    """A world of n^3 voxels: a floor with holes, a pillar and a floating slab."""
    def setup(t):
        xs, ys, zs = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        floor = (ys == 0) & ((xs + 2 * zs) % 5 != 0)
        pillar = (xs == n // 2) & (zs == n // 2)
        slab = (ys == n - 1) & (xs < n // 2)
        keep = floor | pillar | slab
        keep[0, 0, 0] = keep[n - 1, n - 1, n - 1] = True          # the world's box is the whole n^3
        xyz = np.stack([xs[keep], ys[keep], zs[keep]], 1).astype(np.int32)
        cm = W.ChunkManager(128, 1.0)
        cm.set_voxels(xyz, (1 + (xyz.sum(axis=1) % 7)).astype(np.uint32))
        cm.rebuild_dirty_chunks()
        t._brick_restart_cm = cm                                   # (the packed arrays are the manager's memory)
        t.set_host_build(n == 4)                                   # the device builder sizes the tree by whole sub-chunks (8^3: two levels); the host builder by the voxels
        stats = t.add_world(cm.pack_chunks_to_gpu_svo(W.scene_materials(SEED)))
        assert 4 ** stats.levels == n, f"a world of {n}^3 voxels has {stats.levels} levels"
    return setup


@pytest.mark.parametrize("n", [16, 4], ids=["two_levels_16", "one_level_4_the_brick_is_the_root"])
def test_a_world_of_two_levels_and_one_of_one(tracer_cls, n):
    """16^3: two levels.  4^3: add_world takes it, and through the host builder (the device builder rounds a world up to whole 8^3 sub-chunks,
    which is two levels again) it is one level — the root is the only brick, every word is node 0 at level 0 and the count launch's descent
    loads nothing."""
    cam = W.camera_look_at((n * 1.9, n * 1.1, n * 1.4), (n * 0.5, n * 0.35, n * 0.5), 40.0, WD, HT)

    def probe(t):
        return t.beam_cache_nodes(WD, HT), t.beam_cache_list(WD, HT)

    log, want, ((entry_words, pixel_words), listing) = check(tracer_cls, small_world(n), frames(cam, 5) + [(wait,)] + frames(cam, 3), probe=probe)
    assert node_launches(log)[-3:] == [1, 1, 1]
    hit = ((want[-1][0][:, 3] >> 24) & 0xFF).cpu().numpy().reshape(HT, WD) == 1
    assert hit.sum() > 200
    assert (pixel_words[hit] >> 29 == 0).all()
    if n == 4:
        assert (pixel_words[hit] == 0).all(), "one level: the brick is the root"


# ---- the words as numbers ------------------------------------------------------------------------------------------------------------

def nodes_probe(w, h):
    def probe(t):
        got = starts_probe(w, h)(t)
        got["entry_words"], got["pixel_words"] = t.beam_cache_nodes(w, h)
        got["has_nodes"] = t.beam_cache_has_nodes()
        got["tree"] = t.download_tree()
        st = t.world_stats()
        got["origin"], got["levels"] = np.array([st.origin[0], st.origin[1], st.origin[2]], dtype=np.int32), int(st.levels)
        return got
    return probe


def per_pixel(got, w, h):
    """From the list's order to the rectangle's: (listed (h, w) bool, start (h, w) float32, entry word (h, w) uint32, group of the pixel (h, w)
    int — area * groups per area + group, -1 for a pixel nobody lists)."""
    listed, start = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=np.float32)
    word, group = np.full((h, w), NONE, dtype=np.uint32), np.full((h, w), -1, dtype=int)
    per_area = got["entries"].shape[1] // 64
    for a, exp in enumerate(expected_areas(got["fine"], got["restarts"], w, h)):
        e = got["entries"][a, :len(exp)]
        assert sorted(e.tolist()) == sorted(exp.tolist()), f"area {a}: the list is not the area's listed pixels"
        xs, ys = (e & 0xFFFF).astype(int), (e >> 16).astype(int)
        listed[ys, xs] = True
        start[ys, xs] = got["starts"][a, :len(exp)]
        word[ys, xs] = got["entry_words"][a, :len(exp)]
        group[ys, xs] = a * per_area + np.arange(len(exp)) // 64
    return listed, start, word, group


def host_side(got, cam, rect, start):
    """The count launch's side on the host over the DOWNLOADED tree (the device's node order), every ray started at its downloaded start."""
    L = shim()
    world = HostWorld.adopt(L, got["tree"][0], got["tree"][1], got["origin"], got["levels"])
    try:
        return world.run(cam, (WD, HT), rect, tstart=start)[0]
    finally:
        world.close()


def nodes_errors(got, records, cam, rect):
    x0, y0, w, h = rect
    listed, start, word, _ = per_pixel(got, w, h)
    bad = []
    if not got["has_nodes"]:
        return ["the list has no node words"], ""
    if not np.array_equal(word[listed], got["pixel_words"][listed]):
        bad.append(f"{int((word != got['pixel_words'])[listed].sum())} entries whose word is not their pixel's of the count launch")
    rec = records.reshape(h, w, 4).copy().view(HIT).reshape(h, w)
    is_hit = rec["hit"] == 1
    host = host_side(got, cam, rect, start)
    if not np.array_equal(host["root"].view(np.uint32).reshape(h, w, 4)[listed], records.reshape(h, w, 4)[listed]):
        bad.append("the host walk from the starts over the downloaded tree differs from the frame")
    if not np.array_equal(host["word"][listed], word[listed]):
        d = host["word"][listed] != word[listed]
        bad.append(f"{int(d.sum())} listed pixels whose word is not the host's over the same tree (device {word[listed][d][:3].tolist()}, host {host['word'][listed][d][:3].tolist()})")
    bad += word_errors(word, is_hit, rec["voxel"], host["cell"], listed, got["tree"][0], got["origin"], got["levels"])
    none = listed & (word == NONE)
    if (none & is_hit).any():
        bad.append(f"{int((none & is_hit).sum())} listed hit pixels without a word")
    if (none & (got["restarts"] != 0)).any():
        bad.append(f"{int((none & (got['restarts'] != 0)).sum())} listed pixels that made a trip and have no word")
    summary = (f"{int(listed.sum())} listed pixels, {int((listed & is_hit).sum())} hits, {int(none.sum())} without a word; levels of the words "
               f"{np.bincount((word[listed & ~none] >> 29).astype(int), minlength=got['levels']).tolist()}")
    return bad, summary


@pytest.mark.parametrize("rect", [None, CUT], ids=["whole_frame", "rectangle_cut_on_all_sides"])
def test_the_words_as_numbers(tracer_cls, scene64, rect):
    """For every listed hit ray the word's level is 0, the node at its index has the bit of the record's voxel set, and that node is the one
    reached by descending the downloaded tree by the voxel's digits on the host; for a listed ray that misses and has a word, the cell at the
    word's level is empty in that node, which is the one the descent by the cell's digits reaches; every entry's word is its pixel's; and the
    count launch's side compiled for the host, over the same tree from the downloaded starts, gives the same words bit for bit."""
    cam = view(1)
    x0, y0, w, h = rect or (0, 0, WD, HT)
    log, want, got = check(tracer_cls, world64(scene64), frames(cam, 4, rect) + [(wait,)] + frames(cam, 3, rect), lockstep=True, probe=nodes_probe(w, h))
    assert node_launches(log)[-3:] == [1, 1, 1]
    records = want[-1][0].cpu().numpy().view(np.uint32).reshape(h, w, 4)
    errors, summary = nodes_errors(got, records, cam, (x0, y0, w, h))
    print(summary)
    assert not errors, "; ".join(errors[:6])
    hit = ((records[..., 3] >> 24) & 0xFF) == 1
    assert hit.sum() > 500 and (~hit).sum() > 500


def test_the_checks_catch_a_word_of_another_node_and_a_word_in_the_wrong_place(tracer_cls, scene64):
    cam = view(1)
    _, want, got = check(tracer_cls, world64(scene64), frames(cam, 5) + [(wait,)] + frames(cam, 1), lockstep=True, probe=nodes_probe(WD, HT))
    records = want[-1][0].cpu().numpy().view(np.uint32).reshape(HT, WD, 4)
    assert not nodes_errors(got, records, cam, (0, 0, WD, HT))[0]
    a = int(np.argmax([len(e) for e in expected_areas(got["fine"], got["restarts"], WD, HT)]))
    off = dict(got, entry_words=got["entry_words"].copy())
    off["entry_words"][a, 0] += 1
    assert any("is not their pixel's" in s for s in nodes_errors(off, records, cam, (0, 0, WD, HT))[0])
    both = dict(off, pixel_words=got["pixel_words"].copy())
    e = int(got["entries"][a, 0])
    both["pixel_words"][e >> 16, e & 0xFFFF] += 1
    assert any("is not the host's" in s for s in nodes_errors(both, records, cam, (0, 0, WD, HT))[0])


def test_few_groups_have_a_lane_that_its_last_trip_does_not_settle(tracer_cls, scene64):
    """The share of walk groups with an unsettled lane, computed on the host from the downloaded list and words — a listed ray without a
    word, or one the entry compiled for the host does not settle over the downloaded tree — is below 25 %: the frames above do not pass on
    the fallback alone.  (On this scene a lane is unsettled only where a ray of a live wave tile misses the world box.)"""
    cam = view(1)
    _, _, got = check(tracer_cls, world64(scene64), frames(cam, 5) + [(wait,)] + frames(cam, 1), lockstep=True, probe=nodes_probe(WD, HT))
    listed, start, word, group = per_pixel(got, WD, HT)
    host = host_side(got, cam, (0, 0, WD, HT), start)
    unsettled = listed & ((word == NONE) | (host["settled"] == 0))
    assert np.array_equal(unsettled, listed & (word == NONE)), "a ray with a word that its last trip does not settle"
    groups = np.unique(group[listed])
    fallback = np.unique(group[unsettled])
    share = len(fallback) / len(groups)
    print(f"{len(fallback)} of {len(groups)} groups have an unsettled lane ({100 * share:.1f} %); {int(unsettled.sum())} of {int(listed.sum())} listed rays")
    assert got["n_groups"] == len(groups)
    assert share < 0.25
