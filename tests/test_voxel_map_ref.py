"""The numpy restatement of the voxel map (tests/voxel_map_ref.py) against the definition in include/m4depth_hip.h, case by
case: what the GPU tests compare the kernels with has to be right first."""
import numpy as np

from voxel_map_ref import VoxelMap, axis, pack, unpack, vertices_of, HALF, EMPTY

F = np.float32


def _scene(seed=5, n=400):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    return vertices_of(xyz, rng.integers(0, 256, (n, 3)))


def test_shuffling_the_vertices_changes_nothing():
    v = _scene()
    rng = np.random.default_rng(0)
    a = VoxelMap(0.25).integrate(v[:250], 1).integrate(v[250:], 2)
    b = VoxelMap(0.25).integrate(rng.permutation(v[:250]), 1).integrate(rng.permutation(v[250:]), 2)
    assert a.records == b.records and len(a.records) < 400 < a.observations + 1
    for m in (1, 2):
        (ka, va), (kb, vb) = a.extract(m), b.extract(m)
        assert np.array_equal(ka, kb) and np.array_equal(va, vb) and np.all(np.diff(ka.astype(np.int64)) > 0)
    assert 0 < len(a.extract(2)[0]) < len(a.extract(1)[0])


def test_a_small_negative_coordinate_lands_in_cell_minus_one():
    assert axis(F(-1e-3), 0.05)[0] == -1 and axis(F(0.0), 0.05)[0] == 0 and axis(F(-0.05), 0.05)[0] == -1
    m = VoxelMap(0.05).integrate(vertices_of([[-1e-3, 0.0, 0.049]], [[1, 2, 3]]), 1)
    (key,) = m.records
    assert unpack(key) == (-1, 0, 0) and key == pack(-1, 0, 0) != EMPTY
    xyz = m.extract()[1][0, :12].view(F)
    assert -0.05 < xyz[0] < 0 <= xyz[1] < 0.05 and 0 <= xyz[2] < 0.05


def test_offset_bins():
    """ox = floor(frac * 256) in 0..255, in float64 on the float32 operands; a negative coordinate so close to zero that
    gx - ix rounds to 1.0 stays in bin 255; the extracted position is the centre of the mean bin."""
    voxel = F(0.5)
    for frac, want in ((0.0, 0), (1 / 256, 1), (0.999, 255), (0.5, 128), (255 / 256, 255)):
        assert axis(F(3 * 0.5 + frac * 0.5), voxel) == (3, want), frac
        assert axis(F(-2 * 0.5 + frac * 0.5), voxel) == (-2, want), frac
    assert axis(F(-1e-30), voxel) == (-1, 255)
    m = VoxelMap(voxel).integrate(vertices_of([[1.5, 1.5, 1.5], [1.5 + 0.5 * 3 / 256, 1.5, 1.75]], [[0, 0, 0]] * 2), 1)
    (rec,) = m.records.values()
    assert rec[:4] == [2, 3, 0, 128]
    xyz = m.extract()[1][0, :12].view(F)
    want = [(3 + (s / 2 + 0.5) / 256.0) * 0.5 for s in (3, 0, 128)]
    assert np.array_equal(xyz, np.array(want, np.float64).astype(F))


def test_colour_rounding_rounds_half_up():
    m = VoxelMap(1.0).integrate(vertices_of([[0.5, 0.5, 0.5]] * 2, [[10, 0, 255], [11, 1, 254]]), 1)
    assert list(m.extract()[1][0, 12:]) == [11, 1, 255, 1]                # 10.5 -> 11, 0.5 -> 1, 254.5 -> 255
    m = VoxelMap(1.0).integrate(vertices_of([[0.5, 0.5, 0.5]] * 3, [[10, 0, 255], [11, 1, 254], [11, 1, 254]]), 1)
    assert list(m.extract()[1][0, 12:15]) == [11, 1, 254]                 # 10.67 -> 11, 0.67 -> 1, 254.33 -> 254


def test_two_observations_under_one_stamp_are_one_frame():
    v = vertices_of([[0.5, 0.5, 0.5]] * 2, [[9, 9, 9]] * 2)
    m = VoxelMap(1.0).integrate(v, 1)
    assert m.extract(1)[1][0, 15] == 1 and len(m.extract(2)[0]) == 0 and m.records[pack(0, 0, 0)][0] == 2
    m.integrate(v, 1)
    assert m.extract(1)[1][0, 15] == 1 and m.records[pack(0, 0, 0)][0] == 4
    m.integrate(v[:1], 2)
    assert m.extract(2)[1][0, 15] == 2 and m.records[pack(0, 0, 0)][0] == 5
    m.integrate(v, 7)
    assert m.extract(3)[1][0, 15] == 3
    many = VoxelMap(1.0)
    for stamp in range(1, 301):
        many.integrate(v[:1], stamp)
    assert many.extract(300)[1][0, 15] == 255                             # alpha = min(frames, 255)


def test_an_index_of_two_to_the_twenty_is_dropped():
    voxel = F(1.0)
    assert axis(F(HALF), voxel) is None and axis(F(HALF - 0.5), voxel) == (HALF - 1, 128)
    assert axis(F(-HALF), voxel) == (-HALF, 0) and axis(F(-HALF - 0.5), voxel) is None
    pts = [[HALF, 0, 0], [0, -HALF - 1, 0], [0, 0, 3e38], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [-HALF, HALF - 1, 0]]
    m = VoxelMap(voxel).integrate(vertices_of(pts, [[1, 2, 3]] * len(pts)), 1)
    assert m.observations == 7 and m.dropped_range == 6 and list(m.records) == [pack(-HALF, HALF - 1, 0)]
    assert pack(-HALF, HALF - 1, 0) == (HALF * 2 - 1) << 21 | HALF and pack(HALF - 1, HALF - 1, HALF - 1) == (1 << 63) - 1
    assert m.stats() == {"observations": 7, "dropped_range": 6, "dropped_full": 0, "occupied": 1}
