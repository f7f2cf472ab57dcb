"""CPU: the plain references of tests/test_volume_rebuild_gpu.py against what they restate — reference_tree against the host builder
(tree_build.cpp through the host harness), DenseModel's brush against the oracle's ChunkManager — byte for byte."""
import numpy as np
import pytest

from blok_amd import world as W
from tests import oracle_ffi as O
from tests.conftest import SEED
from tests.harness_ffi import HostKernel
from tests.volume_tree_reference import DenseModel, OutsideBox, box_levels, brick_table, reference_tree


def _pinned(xyz, mats):
    """The voxel list through the oracle's world and the host builder, and through the model and reference_tree."""
    ow = O.OracleWorld(128, 1.0)
    ow.set_voxels(xyz, mats)
    ow.rebuild()
    hk = HostKernel(*ow.pack())
    nodes, origin = hk.tree_nodes()
    hi = xyz.max(axis=0) + 1
    model = DenseModel(origin, tuple(int(hi[a]) - origin[a] for a in range(3)))
    model.set_voxels(xyz, mats)
    ref_nodes, ref_mats = reference_tree(model.filled, model.ids, hk.levels)
    assert ref_nodes.dtype == np.uint32 and ref_mats.dtype == np.uint32
    assert ref_nodes.tobytes() == nodes.tobytes()
    assert len(ref_mats) == hk.n_voxels == int(model.filled.sum())
    return hk, origin, ref_nodes, ref_mats


@pytest.mark.parametrize("seed", [SEED, 0xB10C0002])
def test_reference_tree_equals_the_host_builder_on_the_scene(seed):
    ids = W.scene_dense(64, seed)
    z, y, x = np.nonzero(ids)
    hk, origin, nodes, mats = _pinned(np.stack([x, y, z], 1).astype(np.int32), ids[z, y, x])
    assert hk.levels == 3 and origin == (0, 0, 0) and len(nodes) > 500
    # the materials in key order: brick i's ids are its voxels' in bit order
    bricks = nodes[len(nodes) - len(brick_table(ids > 0, ids)):]
    assert int(bricks[-1, 2]) + bin(int(bricks[-1, 0]) | int(bricks[-1, 1]) << 32).count("1") == len(mats)


def test_reference_tree_equals_the_host_builder_at_negative_coordinates():
    rng = np.random.default_rng(17)
    xyz = rng.integers(-90, 75, size=(6000, 3)).astype(np.int32)
    xyz[:500] = xyz[500:1000]                                  # duplicates: the last write wins
    mats = rng.integers(1, 1 << 16, size=len(xyz)).astype(np.uint32)
    hk, origin, nodes, _ = _pinned(xyz, mats)
    assert origin == (-96, -96, -96) and hk.levels == 4


def test_reference_tree_of_nothing_and_of_one_voxel():
    nodes, mats = reference_tree(np.zeros((3, 2, 5), bool), np.zeros((3, 2, 5), np.uint32), 2)
    assert nodes.tobytes() == bytes(16) and len(mats) == 0
    ids = np.zeros((1, 1, 1), np.uint32); ids[0, 0, 0] = 9
    nodes, mats = reference_tree(ids > 0, ids, box_levels((1, 1, 1)))
    assert nodes.tolist() == [[1, 0, 0, 0]] and mats.tolist() == [9]
    assert [box_levels((n, 1, 1)) for n in (1, 4, 5, 16, 17, 64, 65, 256, 257, 1024, 1025, 4096, 4097, 16384)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]


def test_model_brush_equals_the_oracle():
    """OracleWorld.apply_brush + chunk_dense for the six edits of tests/test_brush.py::edited_worlds, bit for bit."""
    from tests.test_brush import edited_worlds
    _, ow, edits = edited_worlds()
    C_ = 128
    model = DenseModel((-C_, 0, 0), (3 * C_, C_, C_))          # chunks (-1..1, 0, 0): everything the edits touch
    ids = W.scene_dense(64, SEED)
    z, y, x = np.nonzero(ids)
    model.set_voxels(np.stack([x, y, z], 1), ids[z, y, x])
    for c, r, v, mode in edits:
        model.brush(c, r, v, {"add": 0, "subtract": 1}[mode])
    assert ow.n_chunks() >= 3
    for i in range(ow.n_chunks()):
        (cx, cy, cz), _ = ow.chunk(i)
        od, om = ow.chunk_dense(i, C_)
        x0 = cx * C_ + C_
        assert cy == 0 and cz == 0 and 0 <= x0 < 3 * C_
        assert model.density[:, :, x0:x0 + C_].tobytes() == od.tobytes(), (cx, cy, cz)
        assert model.ids[:, :, x0:x0 + C_].tobytes() == om.tobytes(), (cx, cy, cz)
    with pytest.raises(OutsideBox):
        model.brush((60.0, 125.0, 30.0), 6.0, 1.0, 0)
    with pytest.raises(OutsideBox):
        model.set_voxels([[0, -1, 0]])
