"""GPU: the context's grow-on-demand buffers (blok_amd/csrc/hip/device_buffer.h; api_internal.h: StreamScratch, Models) grow while earlier
work of their stream is in flight, and nothing a frame computes changes.

A 256x256 context over the 64^3 scene launches a small rectangle and then the full frame on a side stream with nothing synchronised in
between: every per-stream buffer of the launch form is replaced behind the small launch.  The reference in every case is a fresh context
that only ever saw the large launch.  Primary frames (launch forms 0, 1, 2, 4, 5): records and RGBA bit-equal, no wave ever gave up a
wait.  Path frames (4 spp, 2 bounces: the tail pool) and instanced path frames (one instance of one model, then forty of seventeen: the
instance BVH, and the device copy of the descriptors past its first sixteen): the G-buffer planes bit-equal, the colour inside
test_paths.test_tail_pool_changes_only_the_order_of_a_pixels_sum's tolerance (the same terms, possibly in another order).  Instanced
primary frames: the bins and the world records of the instance pass.  Then the stream is released, a new one draws the same frames,
and the context is resized.  No test asks the device for memory it cannot give: the failure paths are
tests/test_device_buffer_cpu.py's."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import world as W
from blok_amd._ffi import HIT, INSTANCE, INSTANCE_NONE
from tests import instance_oracle as IO
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

SIZE = 256
FORMS = (0, 1, 2, 4, 5)
SMALL, SMALL_PATH = (0, 0, 64, 64), (0, 0, 32, 32)
FULL = (0, 0, SIZE, SIZE)
PATH = dict(spp=4, max_bounces=2, frame_index=5)
N_MODELS, N_INSTANCES = 17, 40       # one descriptor more than the device copy's first capacity


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def brick(k):
    """A one-brick model: an 8^3 cube whose materials depend on k."""
    xyz = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    return xyz, (1 + (xyz.sum(axis=1) + k) % 40).astype(np.uint32)


def one_instance():
    return np.array([IO.instance(0, (30, 70, 30))], dtype=INSTANCE)


def forty_instances():
    return np.array([IO.instance(i % N_MODELS, (4 + 7 * (i % 8), 40 + 9 * (i // 8), 6 + 11 * (i % 5)), *IO.SIGNED_PERMUTATIONS[i]) for i in range(N_INSTANCES)],
                    dtype=INSTANCE)


def tracer(pw, w=SIZE, h=SIZE, models=0):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(w, h).init()
    tr.add_world(pw)
    for k in range(models):
        assert tr.model_create(*brick(k)) == k
    return tr


def camera(w=SIZE, h=SIZE, pose=0):
    return W.scene_camera(64, pose, w, h, SEED)


def device_table(torch, table):
    return torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).copy()).cuda()


class Frames:
    """Launches whose outputs are allocated and zeroed BEFORE anything is launched (one synchronisation), so that the launches themselves
    follow each other on their stream with nothing in between; `fetch` synchronises and returns everything as bytes."""

    def __init__(self, torch):
        self.torch, self.jobs, self.outs = torch, [], []

    def _buffers(self, sizes):
        bufs = [self.torch.zeros(n, dtype=self.torch.uint8, device="cuda") for n in sizes]
        self.outs.append(bufs)
        return [b.data_ptr() for b in bufs]

    def primary(self, tr, cam, rect):
        n = rect[2] * rect[3]
        hits, rgba = self._buffers((n * HIT.itemsize, n * 4))
        self.jobs.append(lambda s: tr.draw_frame_device(cam, hits, rgba, rect=rect, stream=s))

    def primary_instanced(self, tr, cam, rect, table):
        n = rect[2] * rect[3]
        rgba, ids = self._buffers((n * 4, n * 4))       # no record output: the instance pass reads the stream's own world records
        self.jobs.append(lambda s: tr.trace_primary_instanced_device(cam, table.data_ptr(), table.numel() // INSTANCE.itemsize, 0, rgba, ids, rect=rect, stream=s))

    def paths(self, tr, cam, rect, table=None):
        n = rect[2] * rect[3]
        p = self._buffers([n * 16] * 4 + ([n * 4] if table is not None else []))
        if table is None:
            self.jobs.append(lambda s: tr.trace_paths_device(cam, p[0], rect=rect, world_pos_ptr=p[1], normal_roughness_ptr=p[2], albedo_metallic_ptr=p[3], stream=s, **PATH))
        else:
            self.jobs.append(lambda s: tr.trace_paths_instanced_device(cam, table.data_ptr(), table.numel() // INSTANCE.itemsize, p[0], p[1], p[2], p[3], p[4],
                                                                       rect=rect, stream=s, **PATH))

    def launch(self, stream):
        self.torch.cuda.synchronize()
        for job in self.jobs:
            job(stream.cuda_stream)
        self.jobs = []

    def fetch(self):
        self.torch.cuda.synchronize()
        return [[b.cpu().numpy().tobytes() for b in bufs] for bufs in self.outs]


def same_path_frame(got, want, what):
    """Every plane (and the id plane of an instanced frame) bit-equal, the colour inside the tail pool's tolerance (tests/test_paths.py)."""
    for k, (g, w) in enumerate(zip(got, want)):
        if k == 0:
            a, b = (np.frombuffer(x, dtype=np.float32).reshape(-1, 4)[:, :3].astype(np.float64) for x in (w, g))
            assert np.isfinite(b).all(), what
            worst = float((np.abs(a - b) / (1e-4 + 1e-3 * np.abs(a))).max())
            print(what, "colour: largest difference over its bound", worst / 1e-2)
            assert (np.abs(a - b) <= 1e-2 * (1e-4 + 1e-3 * np.abs(a))).all(), (what, worst)
        else:
            assert g == w, (what, "plane", k)


@pytest.fixture(scope="module")
def fresh(torch_cuda, scene64):
    """What contexts that only ever saw the large launch give: per launch form the primary frame, the path frame, the instanced frames."""
    torch = torch_cuda
    cm, pw = scene64
    ref = {}
    for form in FORMS:
        tr = tracer(pw); tr.set_fused(form)
        f = Frames(torch); f.primary(tr, camera(), FULL); f.launch(torch.cuda.Stream())
        ref["primary", form] = f.fetch()[0]
        tr.shutdown()
    tr = tracer(pw)
    f = Frames(torch); f.paths(tr, camera(), FULL); f.launch(torch.cuda.Stream())
    ref["paths"] = f.fetch()[0]
    tr.shutdown()
    tr = tracer(pw, models=N_MODELS)
    table = device_table(torch, forty_instances())
    f = Frames(torch); f.paths(tr, camera(), FULL, table); f.primary_instanced(tr, camera(), FULL, table); f.launch(torch.cuda.Stream())
    ref["paths_instanced"], ref["primary_instanced"] = f.fetch()
    seen = np.unique(np.frombuffer(ref["paths_instanced"][4], dtype=np.uint32))
    print("instances with a first hit in the frame:", len(seen[seen != INSTANCE_NONE]), "of", N_INSTANCES)
    assert len(seen[seen != INSTANCE_NONE]) >= N_INSTANCES // 2, "the instanced frames must show the instances"
    tr.shutdown()
    return ref


def draw_primary_pairs(torch, tr, stream, fresh, what):
    """Small rectangle, then the full frame, per launch form, nothing synchronised within a pair; the full frames against the fresh contexts'."""
    for form in FORMS:
        tr.set_fused(form)
        f = Frames(torch); f.primary(tr, camera(pose=1), SMALL); f.primary(tr, camera(), FULL); f.launch(stream)
        got = f.fetch()[1]
        assert got[0] == fresh["primary", form][0], (what, "records", form)
        assert got[1] == fresh["primary", form][1], (what, "RGBA", form)
    tr.set_fused(3)
    assert tr.frame_queue_stalls() == 0, what


def draw_path_pair(torch, tr, stream, fresh, what):
    f = Frames(torch); f.paths(tr, camera(pose=1), SMALL_PATH); f.paths(tr, camera(), FULL); f.launch(stream)
    same_path_frame(f.fetch()[1], fresh["paths"], what)


def test_primary_frames_while_the_stream_scratch_grows(torch_cuda, scene64, fresh):
    torch = torch_cuda
    tr = tracer(scene64[1])
    draw_primary_pairs(torch, tr, torch.cuda.Stream(), fresh, "grown")
    tr.shutdown()


def test_path_frames_while_the_tail_pool_grows(torch_cuda, scene64, fresh):
    torch = torch_cuda
    tr = tracer(scene64[1])
    draw_path_pair(torch, tr, torch.cuda.Stream(), fresh, "grown")
    tr.shutdown()


def test_instanced_frames_while_the_instance_buffers_grow(torch_cuda, scene64, fresh):
    """One instance of the only model, drawn; sixteen more models, so that the device copy of the descriptors is replaced (model_create
    waits for the device itself).  Then one instance in a small rectangle and forty in the full frame with nothing synchronised in between,
    as a path frame (the instance BVH grows) and as a primary frame without a record output (the bins and the world records grow)."""
    torch = torch_cuda
    tr = tracer(scene64[1], models=1)
    stream = torch.cuda.Stream()
    one, forty = device_table(torch, one_instance()), device_table(torch, forty_instances())
    f = Frames(torch); f.paths(tr, camera(), FULL, one); f.launch(stream)
    for k in range(1, N_MODELS):
        assert tr.model_create(*brick(k)) == k
    tr.check_instances(forty_instances())
    f = Frames(torch)
    f.paths(tr, camera(pose=1), SMALL_PATH, one); f.primary_instanced(tr, camera(pose=1), SMALL, one)
    f.paths(tr, camera(), FULL, forty); f.primary_instanced(tr, camera(), FULL, forty)
    f.launch(stream)
    got = f.fetch()
    same_path_frame(got[2], fresh["paths_instanced"], "grown, instanced")
    assert got[3] == fresh["primary_instanced"], "instanced primary frame: RGBA, ids"
    tr.shutdown()


def test_released_stream_and_resized_context(torch_cuda, scene64, fresh):
    torch = torch_cuda
    pw = scene64[1]
    tr = tracer(pw)
    side = torch.cuda.Stream()
    draw_primary_pairs(torch, tr, side, fresh, "before the release")
    draw_path_pair(torch, tr, side, fresh, "before the release")
    tr.release_stream(side.cuda_stream)
    other = torch.cuda.Stream()
    draw_primary_pairs(torch, tr, other, fresh, "new stream")
    draw_path_pair(torch, tr, other, fresh, "new stream")
    # twice as wide: the order and beam-cache buffers are replaced by the resize, the stream's scratch by the next launches
    wide = (0, 0, 2 * SIZE, SIZE)
    cam = camera(2 * SIZE, SIZE)
    tr.resize(2 * SIZE, SIZE)
    ref = tracer(pw, 2 * SIZE, SIZE)
    frames = []
    for t in (tr, ref):
        f = Frames(torch); f.primary(t, cam, wide); f.paths(t, cam, wide); f.launch(other)
        frames.append(f.fetch())
    assert frames[0][0] == frames[1][0], "resized: records, RGBA"
    same_path_frame(frames[0][1], frames[1][1], "resized")
    assert tr.frame_queue_stalls() == 0
    tr.shutdown(); ref.shutdown()
