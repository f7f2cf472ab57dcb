"""CPU: the walk's far planes, evaluated once at the bottom of a trip (trace_core.h, enter_axis and walk_loop), against the oracle.

After a descent the far plane of the child slab is taken as plane_t(f + s) with the advanced corner f instead of being chosen among
the node's far plane and the two probes; the four cases of that identity are exercised here by rays whose entry parameter falls on or
next to the probed planes: rays through lattice points at node boundaries, rays running inside a node plane, grazing rays, rays that
cross the whole world (the root's far plane fW), and rays whose tmin is exactly the parameter of a node plane."""
import numpy as np
import pytest

from blok_amd import world as W
from tests import harness_ffi as H
from tests import oracle_ffi as O
from tests.conftest import SEED, edge_case_rays, random_rays, records_equal


def _rays(rows):
    rays = np.zeros(len(rows), dtype=O.RAY)
    for i, (o, d, tmin, tmax) in enumerate(rows):
        d = np.asarray(d, dtype=np.float64)
        d = d / np.linalg.norm(d)
        rays[i] = (tuple(np.float32(o)), np.float32(tmin), tuple(d.astype(np.float32)), np.float32(tmax))
    return rays


def plane_rays(n: int, seed: int):
    """Rays on and next to node planes of a world of edge n (levels of 4, 16, 64 voxels)."""
    rng = np.random.default_rng(seed)
    rows = []
    steps = [1, 4, 16, 64]
    dirs = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 1, 0), (1, -1, 0), (0, 1, 1), (1, 1, 1),
            (-1, -1, -1), (1, -1, 1), (2, 1, 0), (1, 2, 4), (-4, 1, 2), (4, 4, 1)]
    for _ in range(3000):
        s = steps[rng.integers(len(steps))]
        # an origin on a lattice point of that level, inside or outside the world, sometimes nudged off it by a hair
        o = rng.integers(-2, n // s + 2, size=3) * float(s)
        if rng.random() < 0.3:
            o = o + rng.choice([-1e-3, 1e-3, 0.5], size=3) * (rng.random(3) < 0.5)
        d = np.asarray(dirs[rng.integers(len(dirs))], dtype=np.float64)
        if rng.random() < 0.4:
            d = d + rng.normal(scale=1e-4, size=3)               # grazing: almost inside a plane
        if not np.any(d):
            continue
        tmin = 0.0 if rng.random() < 0.5 else float(s * rng.integers(0, 4))   # tmin on a plane crossing of an axis ray
        rows.append((o, d, tmin, 10000.0))
    # straight through the whole world, corner to corner and face to face: the root's far planes bound the walk
    for o, d in [((-1, -1, -1), (1, 1, 1)), ((n + 1, n + 1, n + 1), (-1, -1, -1)), ((-1, 0, 0), (1, 0, 0)), ((0, -1, n), (0, 1, 0)),
                 ((n, n, -1), (0, 0, 1)), ((-0.5, n * 0.5, n * 0.5), (1, 1e-7, 0)), ((n * 0.5, -3, n * 0.5), (1e-3, 1, -1e-3))]:
        rows.append((o, d, 0.001, 10000.0))
        rows.append((o, d, 0.0, float(n)))
    return _rays(rows)


def test_node_plane_and_grazing_rays_bit_exact(scene64):
    cm, pw = scene64
    rays = np.concatenate([plane_rays(64, 21), edge_case_rays(), random_rays(64, 8000, 33)])
    ref, ctr = O.Lattice(pw.nodes, pw.sub_chunks).trace(rays)
    got = H.HostKernel(pw.nodes, pw.sub_chunks).trace_rays(rays)
    assert ctr["hits"] > 1000
    bad = np.flatnonzero(~records_equal(got, ref))
    assert bad.size == 0, f"{bad.size} records differ, first rays: {rays[bad[:4]]}"


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_full_frames_bit_exact_64(scene64, pose):
    cm, pw = scene64
    cam = W.scene_camera(64, pose, 256, 192, SEED)
    ref, ctr = O.Lattice(pw.nodes, pw.sub_chunks).trace(O.primary_rays(cam, 256, 192))
    got = H.HostKernel(pw.nodes, pw.sub_chunks).trace_primary(cam, 256, 192)
    assert ctr["hits"] > 1000
    assert records_equal(got, ref).all()
