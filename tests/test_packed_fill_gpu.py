"""A packed frame of a view at rest in ONE launch (blok_hip_set_packed_fill; trace_kernels.hip: packed_frame_kernel, packed_frame_own_kernel;
fill_units.h): the walk's workgroups also write the miss pixels of the empty wave tiles as fill units, with fill-only workgroups behind them
where the units need them.  By tests/test_own_start_gpu.py's method and on its frames (200 x 136 or smaller over the 64^3 scene, K = N = 1):
every frame of every scenario is compared byte for byte, records and RGBA8, with the frame a twin tracer whose cache is switched off makes
of the same view, rectangle and jitter (computed once per module: such a tracer makes the same frame every time), in buffers filled with
garbage; the counters say which form ran.

The start key's tmin and tmax are constants of the library (tests/test_own_start_gpu.py), so the launch "under another start key" changes the
key's other two words, the jitter: it is the same branch of the launch code and the same second kernel."""
import numpy as np
import pytest

from tests.test_own_start_gpu import DOWN, GARBAGE, HT, SKY, WD, frames, view, wait, world64

pytestmark = pytest.mark.gpu

JITTER = (0.31, -0.22)
NEAR = view(2, radius=45.0)                                  # close enough that every rectangle below, the frame's top left corner too, holds hits and sky


@pytest.fixture(scope="module")
def tracer_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from blok_amd.tracer import HipTracer
    return HipTracer


@pytest.fixture(scope="module")
def twin(tracer_cls, scene64):
    """reference(cam, rect, jitter) -> (records, RGBA8) of the tracer with the cache off, kept per (view, rectangle, jitter)."""
    import torch
    off = tracer_cls(WD, HT).init()
    off.set_beam_cache(False)
    world64(scene64)(off)
    kept = {}

    def reference(cam, rect, jitter):
        key = (np.ascontiguousarray(cam).tobytes(), rect, jitter)
        if key not in kept:
            n = (rect[2] * rect[3]) if rect else WD * HT
            hits = torch.full((n, 4), GARBAGE, dtype=torch.int32, device="cuda")
            rgba = torch.full((n,), GARBAGE, dtype=torch.int32, device="cuda")
            off.set_taa_jitter(jitter)
            off.draw_frame_device(cam, hits.data_ptr(), rgba.data_ptr(), rect=rect)
            torch.cuda.synchronize()
            assert off.beam_cache_last_action() == 0 and off.beam_cache_list_state() == 0, "a tracer with the cache off never hits or lists"
            assert not bool((rgba == GARBAGE).any()) and not bool((hits == GARBAGE).all(dim=1).any()), "the reference left pixels unwritten"
            kept[key] = (hits, rgba)
        return kept[key]
    yield reference
    torch.cuda.synchronize()
    off.shutdown()


def run(tracer_cls, scene64, twin, steps, k, mode=4, lockstep=False, outputs=None):
    """The steps on a tracer under `mode` with K = N = 1 and the switch at k: ("frame", camera, rectangle or None) steps go round three
    streams into their own garbage-filled buffers; any other step is a callable applied to the tracer behind a synchronisation.  outputs:
    per frame "both", "records" or "rgba" (the other pointer is null, and its buffer must keep its garbage).  Every frame is compared with
    the twin's.  -> per frame (list state, starts state, one-launch frames so far, fill-only workgroups so far), and the frames."""
    import torch
    t = tracer_cls(WD, HT).init()
    streams = [torch.cuda.Stream() for _ in range(3)]
    try:
        t.set_beam_cache(mode); t.set_beam_refine_after(1); t.set_beam_list_after(1); t.set_packed_fill(k)
        world64(scene64)(t)
        made, log, jitter = [], [], None
        for step in steps:
            if step[0] != "frame":
                torch.cuda.synchronize()
                if step[0] is set_jitter:
                    jitter = step[1]
                step[0](t, *step[1:])
                continue
            _, cam, rect = step
            n = (rect[2] * rect[3]) if rect else WD * HT
            what = outputs[len(made)] if outputs else "both"
            s = streams[len(made) % 3]
            with torch.cuda.stream(s):
                hits = torch.full((n, 4), GARBAGE, dtype=torch.int32, device="cuda")
                rgba = torch.full((n,), GARBAGE, dtype=torch.int32, device="cuda")
            t.draw_frame_device(cam, hits.data_ptr() if what != "rgba" else 0, rgba.data_ptr() if what != "records" else 0, rect=rect, stream=s.cuda_stream)
            made.append((hits, rgba, cam, rect, jitter, what))
            log.append((t.beam_cache_list_state(), t.beam_cache_starts_state()) + t.packed_fill_counters())
            if lockstep:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        for i, (hits, rgba, cam, rect, jit, what) in enumerate(made):
            want_hits, want_rgba = twin(cam, rect, jit)
            if what != "rgba":
                assert torch.equal(hits, want_hits), f"frame {i} {log[i]}: records differ in {int((hits != want_hits).any(dim=1).sum())} pixels"
            else:
                assert bool((hits == GARBAGE).all()), f"frame {i} {log[i]}: records written through a null pointer's buffer"
            if what != "records":
                assert torch.equal(rgba, want_rgba), f"frame {i} {log[i]}: RGBA8 differs in {int((rgba != want_rgba).sum())} pixels"
            else:
                assert bool((rgba == GARBAGE).all()), f"frame {i} {log[i]}: RGBA8 written through a null pointer's buffer"
        return log, made
    finally:
        torch.cuda.synchronize()
        for s in streams:
            t.release_stream(s.cuda_stream)
        t.shutdown()


def set_jitter(t, jitter):
    t.set_taa_jitter(jitter)


def rest(cam, rect=None, tail=3):
    """A view from its first launch to its adopted list, then `tail` packed launches."""
    return frames(cam, 5, rect) + [(wait,)] + frames(cam, tail, rect)


def one_launch_tail(log, tail=3):
    """The last `tail` launches walked packed, each as one launch -> the fill-only workgroups of the last."""
    assert [e[0] for e in log][-tail:] == [2] * tail, log
    before = log[-tail - 1]
    assert [e[2] - before[2] for e in log[-tail:]] == list(range(1, tail + 1)), log
    return log[-1][3] - log[-2][3]


# ---- the full frame: 3 whole units and 8 pixels a row, 17 tile rows ------------------------------------------------------------------------

@pytest.mark.parametrize("lockstep", [False, True], ids=["in_flight", "one_at_a_time"])
@pytest.mark.parametrize("k", [4, 1, 1000])
def test_the_full_frame(tracer_cls, scene64, twin, k, lockstep):
    log, _ = run(tracer_cls, scene64, twin, rest(view(0)), k, lockstep=lockstep)
    tail = one_launch_tail(log)
    assert [e[1] for e in log][-3:] == [1, 1, 1]             # from the starts: packed_frame_own_kernel
    units = HT * 4
    if k == 1:
        assert tail > 0, "k = 1: more units than groups, and no fill-only workgroup"
        assert tail < units
    if k == 1000:
        assert tail == 0 and log[-1][3] == 0, "a large k: every unit rides on a walk wave"
    if lockstep:
        assert [e[0] for e in log] == [0, 0, 0, 1, 2, 2, 2, 2] and [e[2] for e in log] == [0, 0, 0, 0, 1, 2, 3, 4]


# ---- rectangles ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 1])
@pytest.mark.parametrize("rect", [(8, 16, 64, 64), (3, 5, 77, 61), (0, 0, 40, 24), (0, 0, 136, 8)],
                         ids=["one_exact_unit_per_row", "unaligned_origin_odd_width", "narrower_than_a_unit", "one_tile_row"])
def test_rectangles(tracer_cls, scene64, twin, rect, k):
    log, made = run(tracer_cls, scene64, twin, rest(NEAR, rect), k)
    one_launch_tail(log)
    hit = ((made[-1][0][:, 3] >> 24) & 0xFF) == 1
    print(f"{rect}: {int(hit.sum())} hits of {rect[2] * rect[3]} pixels")
    assert 30 <= int(hit.sum()) <= rect[2] * rect[3] - 30, "the rectangle wants pixels to walk and pixels to fill"


# ---- edge views ------------------------------------------------------------------------------------------------------------------------------

def test_an_all_sky_view_gets_the_fill_alone(tracer_cls, scene64, twin):
    log, made = run(tracer_cls, scene64, twin, rest(SKY), 4, lockstep=True)
    assert [e[0] for e in log][-3:] == [2, 2, 2]
    assert log[-1][2:] == (0, 0), "no group, no one-launch frame"
    assert not bool(((made[-1][0][:, 3] >> 24) & 0xFF).any())


@pytest.mark.parametrize("k", [4, 1])
def test_a_view_where_every_pixel_hits(tracer_cls, scene64, twin, k):
    log, made = run(tracer_cls, scene64, twin, rest(DOWN), k, lockstep=True)
    one_launch_tail(log)
    assert bool((((made[-1][0][:, 3] >> 24) & 0xFF) == 1).all())


# ---- null outputs ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 1])
def test_records_only_then_rgba_only(tracer_cls, scene64, twin, k):
    steps = rest(view(0), tail=4)
    log, _ = run(tracer_cls, scene64, twin, steps, k, outputs=["both"] * 5 + ["records", "records", "rgba", "rgba"])
    one_launch_tail(log, tail=4)


# ---- the second kernel -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 1])
def test_a_packed_launch_under_another_start_key_walks_from_the_finer_bounds(tracer_cls, scene64, twin, k):
    steps = frames(view(4), 5) + [(wait,), (set_jitter, JITTER)] + frames(view(4), 3) + [(set_jitter, (0.0, 0.0))] + frames(view(4), 2)
    log, made = run(tracer_cls, scene64, twin, steps, k)
    assert [e[0] for e in log][-5:] == [2] * 5 and [e[1] for e in log][-5:] == [2, 2, 2, 1, 1], log
    assert [e[2] - log[-6][2] for e in log[-5:]] == [1, 2, 3, 4, 5], log
    assert not bool((made[-1][0] == made[-3][0]).all()), "the jitter changes nothing in this view"


@pytest.mark.parametrize("k", [4, 1])
def test_the_list_under_cache_mode_3(tracer_cls, scene64, twin, k):
    log, _ = run(tracer_cls, scene64, twin, rest(view(0)), k, mode=3)
    one_launch_tail(log)
    assert all(e[1] == 0 for e in log)                        # no starts: packed_frame_kernel


# ---- the switch ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [4, 3])
def test_switch_0_against_switch_k(tracer_cls, scene64, twin, mode):
    import torch
    steps = rest(view(1))
    log0, made0 = run(tracer_cls, scene64, twin, steps, 0, mode=mode)
    logk, madek = run(tracer_cls, scene64, twin, steps, 4, mode=mode)
    assert [e[0] for e in log0][-3:] == [2, 2, 2] and all(e[2:] == (0, 0) for e in log0), "switch 0: two launches, never one"
    one_launch_tail(logk)
    for a, b in zip(made0, madek):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_switch_in_mid_life(tracer_cls, scene64, twin):
    """The switch is read by the next launch: the same list serves both forms."""
    def to(k):
        return (lambda t: t.set_packed_fill(k),)
    steps = rest(view(3), tail=2) + [to(0)] + frames(view(3), 2) + [to(2)] + frames(view(3), 2)
    log, _ = run(tracer_cls, scene64, twin, steps, 4)
    assert [e[0] for e in log][-6:] == [2] * 6
    assert [e[2] - log[-7][2] for e in log[-6:]] == [1, 2, 2, 2, 3, 4], log
