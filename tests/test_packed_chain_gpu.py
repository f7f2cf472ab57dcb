"""The packed frame's node kernel with its loads in front of its stores (trace_kernels.hip: packed_frame_node_kernel, fill_batch_load,
fill_batch_store, fill_units_of_workgroup): the bounds of a workgroup's first four fill units are loaded beside its group's entries and held
across the walk, a workgroup's later units load their bounds four at a time from an index brought into the array, a padding lane of a group
walks along unlisted instead of leaving, a workgroup of the grid's tail and a wave that falls back end behind units of their own, and a
settled hit loads its albedo whether or not the launch has an RGBA8 output.  tests/test_brick_restart_gpu.py runs that kernel at the
library's k = 4 only and tests/test_packed_fill_gpu.py sweeps k under modes 4 and 3 only; here mode 5 meets the other k: by the latter's
method and on its frames (200 x 136 or smaller over the 64^3 scene, K = N = 1), every frame compared byte for byte, records and RGBA8, with
the frame of a twin tracer whose cache is off, in buffers filled with garbage.

k = 1: more units than groups, so the grid has a tail of fill-only workgroups and a walk wave has one unit (three of its four bounds are
loaded from the clamped index and belong to nobody).  k = 4: the library's.  k = 1000: no tail, and a walk wave has more than four units
(544 units of the full frame over its groups), so the batches behind the first run, the last of them partly beyond the units."""
import pytest

from tests.test_beam_list_gpu import SMALL
from tests.test_beam_refine_gpu import CUT
from tests.test_brick_restart_gpu import INSIDE
from tests.test_own_start_gpu import HT, view
from tests.test_packed_fill_gpu import NEAR, one_launch_tail, rest, run
from tests.test_packed_fill_gpu import tracer_cls, twin      # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


def node_counter(seen):
    """A step that notes how many launches of packed_frame_node_kernel the tracer has made so far."""
    return (lambda t: seen.append(t.beam_cache_node_counter()),)


def rest_counted(cam, rect=None, tail=3):
    seen = []
    return rest(cam, rect, tail)[:-tail] + [node_counter(seen)] + rest(cam, rect, tail)[-tail:] + [node_counter(seen)], seen


@pytest.mark.parametrize("lockstep", [False, True], ids=["in_flight", "one_at_a_time"])
@pytest.mark.parametrize("k", [4, 1, 1000])
def test_the_full_frame_from_the_node_words(tracer_cls, scene64, twin, k, lockstep):
    steps, seen = rest_counted(view(0))
    log, _ = run(tracer_cls, scene64, twin, steps, k, mode=5, lockstep=lockstep)
    tail = one_launch_tail(log)
    assert seen[1] - seen[0] == 3, "the last three launches ran packed_frame_node_kernel"
    if k == 1:
        assert 0 < tail < HT * 4, "k = 1: a tail of fill-only workgroups"
    if k == 1000:
        assert tail == 0 and log[-1][3] == 0, "a large k: every unit rides on a walk wave, more than four on each"


@pytest.mark.parametrize("k", [4, 1, 1000])
@pytest.mark.parametrize("cam, rect", [(view(2), CUT), (view(2), SMALL), (NEAR, (0, 0, 40, 24))], ids=["offset_37_19_width_101", "areas_of_5_rows", "narrower_than_a_unit"])
def test_rectangles_whose_groups_end_in_padding(tracer_cls, scene64, twin, cam, rect, k):
    """Areas cut by the rectangle's edge have groups of fewer than 64 entries: the padding lanes walk along unlisted and store nothing, and
    the wave's units behind them are written all the same."""
    steps, seen = rest_counted(cam, rect)
    log, made = run(tracer_cls, scene64, twin, steps, k, mode=5)
    one_launch_tail(log)
    assert seen[1] - seen[0] == 3
    hit = ((made[-1][0][:, 3] >> 24) & 0xFF) == 1
    print(f"{rect}: {int(hit.sum())} hits of {rect[2] * rect[3]} pixels")
    assert int(hit.sum()) >= 30, "the rectangle wants pixels to walk"


@pytest.mark.parametrize("k", [4, 1, 1000])
def test_records_only_then_rgba_only_from_the_node_words(tracer_cls, scene64, twin, k):
    """The null pointer's buffer keeps its garbage: neither the walk's two stores nor the units' write through it, under every k."""
    steps, seen = rest_counted(view(0), tail=4)
    log, _ = run(tracer_cls, scene64, twin, steps, k, mode=5, outputs=["both"] * 5 + ["records", "records", "rgba", "rgba"])
    one_launch_tail(log, tail=4)
    assert seen[1] - seen[0] == 4


@pytest.mark.parametrize("k", [1, 1000])
def test_a_camera_inside_the_world(tracer_cls, scene64, twin, k):
    steps, seen = rest_counted(INSIDE)
    log, _ = run(tracer_cls, scene64, twin, steps, k, mode=5)
    one_launch_tail(log)
    assert seen[1] - seen[0] == 3
