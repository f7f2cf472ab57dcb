"""GPU (-m gpu): the walk loop after its second pass over the generated code (trace_core.h), where the device forms differ from the host's:
the bit-field extracts and chained counts of child_index, the one-bit extract of mask_bit, the sums kept as written.

  * a 128x128 rectangle of the 256^3 scene in poses A and B through the two-launch form (beam kernel, then trace kernel) and through the joint
    launch: every record and every pixel against the oracle;
  * an 8-spp, 3-bounce path frame of 64x64 with ray batching mode 3 — the capped loop and the tail pool run — against the same frame in mode 2,
    within the bound tests/test_paths.py uses for that pair: G-buffer planes bit-identical, colour inside a hundredth of the path tolerance."""
import numpy as np
import pytest

from blok_amd import world as W
from tests import oracle_ffi as O
from tests.conftest import SEED, records_equal

pytestmark = pytest.mark.gpu
FRAME = (1920, 1080)
RECT = (896, 300, 128, 128)


@pytest.fixture(scope="module")
def tracer256(scene256):
    from blok_amd.tracer import HipTracer
    tr = HipTracer(*FRAME).init()
    tr.add_world(scene256[1])
    yield tr
    tr.shutdown()


@pytest.fixture(scope="module")
def oracle_rects(scene256):
    """pose -> the oracle's records of RECT: computed once, shared by both launch forms, never changed."""
    pw = scene256[1]
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    out = {}
    for pose in (0, 1):
        cam = W.scene_camera(256, pose, *FRAME, SEED)
        ref, ctr = lat.trace_primary(cam, *FRAME, x0=RECT[0], y0=RECT[1], w=RECT[2], h=RECT[3], threads=8)
        ref.setflags(write=False)
        out[pose] = (cam, ref, int(ctr["hits"]))
    return out


def _expected_rgba(ref, mats):
    """trace_core.h's shade_rgba of the oracle's records (hit.rchit:58-67): albedo times the face factor, the sky colour on a miss."""
    face_k = np.array([0.8, 0.8, 1.0, 0.4, 0.6, 0.6], dtype=np.float32)
    alb = mats["albedo"][np.minimum(ref["material_id"], len(mats) - 1)] * face_k[np.minimum(ref["face"], 5)][:, None]
    q = (np.minimum(alb, np.float32(1.0)) * np.float32(255.0) + np.float32(0.5)).astype(np.uint32)
    return np.where(ref["hit"] == 1, 0xFF000000 | (q[:, 2] << 16) | (q[:, 1] << 8) | q[:, 0], 0xFF000000 | (230 << 16) | (200 << 8) | 160).astype(np.uint32)


@pytest.mark.parametrize("fused", [0, 2], ids=["trace_rect", "joint_launch"])
@pytest.mark.parametrize("pose", [0, 1], ids=["poseA", "poseB"])
def test_rectangle_records_and_pixels_equal_the_oracle(tracer256, oracle_rects, scene256, pose, fused):
    import torch
    tr = tracer256
    cam, ref, hits = oracle_rects[pose]
    assert hits > 1000 and hits < len(ref)                       # reports and misses both
    tr.set_fused(fused)
    n = RECT[2] * RECT[3]
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_rgba = torch.zeros(n, dtype=torch.int32, device="cuda")
    tr.draw_frame_device(cam, d_hits.data_ptr(), d_rgba.data_ptr(), rect=RECT)
    torch.cuda.synchronize()
    got = d_hits.cpu().numpy().view(O.HIT).reshape(-1)
    for f in O.HIT.names:
        assert np.array_equal(got[f], ref[f]), (f, int((~records_equal(got, ref)).sum()))
    assert records_equal(got, ref).all()
    assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32), _expected_rgba(ref, scene256[1].materials))
    assert records_equal(tr.draw_frame(cam, RECT).reshape(-1), ref).all()        # and through the host-output entry
    tr.set_fused(3)


def test_path_frame_through_the_capped_loop_and_the_tail_pool(tracer256):
    tr = tracer256
    cam = W.scene_camera(256, 0, *FRAME, SEED)
    kw = dict(rect=(928, 332, 64, 64), spp=8, max_bounces=3, frame_index=4)
    tr.set_ray_batching(2); plain = tr.trace_paths(cam, **kw)
    tr.set_ray_batching(3); pooled = tr.trace_paths(cam, **kw)
    for k in plain:
        if k == "color":
            a, b = plain[k][..., :3].astype(np.float64), pooled[k][..., :3].astype(np.float64)
            assert np.isfinite(b).all()
            worst = float((np.abs(a - b) / (1e-4 + 1e-3 * np.abs(a))).max())
            print(f"colour, worst |mode 3 - mode 2| over the path tolerance: {worst:.3e} (bound 1e-2)")
            assert (np.abs(a - b) <= 1e-2 * (1e-4 + 1e-3 * np.abs(a))).all(), worst
        else:
            assert pooled[k].tobytes() == plain[k].tobytes(), k
    assert float(plain["color"][..., :3].max()) > 0.0            # the frame shows something
