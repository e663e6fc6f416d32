"""The numpy restatement of the TSDF meshes (tests/tsdf_mesh_ref.py) against what a fused surface must be: what the GPU tests
compare the kernels with has to be right first.

The distance bars were measured on the float64 variant of the restatement (``exact=True``) against the analytic surfaces and
doubled for float32 rounding (profiles/tsdf_mesh.txt):
  sphere, 26 views at 48 x 48, voxel 0.125 m, K = 2: vertex radii 0.99103 .. 1.01630 m  -> band 0.98208 .. 1.03258 m
  plane, 4 views at 24 x 32, voxel 0.25 m, K = 3: |distance| <= 0.05577 voxel            -> bar 0.11152 voxel
An interpolation written as 1 - t, or a cell offset off by one, moves vertices by half a voxel and more."""
import numpy as np
import pytest

import tsdf_mesh_ref as T

SPHERE_BAND = (0.98208, 1.03258)                                               # rounded inwards
PLANE_BAR = 0.11152                                                            # voxels


def _fuse_sphere(exact=False):
    S = T.SPHERE
    return T.fuse(T.sphere_frames(), S["f"], S["c"], S["voxel"], S["trunc"], S["near"], S["far"], exact=exact)


def _fuse_plane(exact=False, order_seed=None):
    P = T.PLANE
    vol = T.TsdfVolume(P["voxel"], P["trunc"], P["near"], P["far"], exact=exact)
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    for depth, rgb, pose in T.plane_frames():
        vol.frame(depth, rgb, T.PLANE_F, T.PLANE_C, pose, order=None if rng is None else rng.permutation(depth.size))
    return vol


@pytest.fixture(scope="module")
def sphere():
    return _fuse_sphere()


@pytest.fixture(scope="module")
def plane():
    return _fuse_plane()


def _bits(vol):
    return {k: [np.float32(r[0]).view(np.uint32).item()] + r[1:] for k, r in vol.records.items()}


def test_shuffling_the_pixels_of_allocate_changes_nothing(plane):
    other = _fuse_plane(order_seed=3)
    assert list(other.records) != list(plane.records), "the shuffle did not change the arrival order"
    assert _bits(other) == _bits(plane) and other.stats() == plane.stats()
    for m in (1, 2):
        a, b = plane.extract(m), other.extract(m)
        assert all(np.array_equal(a[k], b[k]) for k in ("keys", "vertices", "triangles")) and len(a["keys"]) > 50
        assert np.all(np.diff(a["keys"].astype(np.int64)) > 0)


@pytest.mark.parametrize("min_frames", [1, 2])
def test_sphere_is_a_closed_outward_wound_surface(sphere, min_frames):
    assert len(sphere.records) == 3944 and sphere.dropped_range == 0
    m = sphere.extract(min_frames)
    V, Q = len(m["keys"]), len(m["quads"])
    assert (V, Q) == (1250, 1248) and m["quads_dropped"] == 0 and len(m["triangles"]) == 2 * Q
    edges, shared = T.edge_counts(m["quads"])
    assert (shared == 2).all(), "an edge that is not shared by exactly two faces"
    assert V - len(edges) + Q == 2
    normal, centre = T.quad_normals(m["xyz"], m["quads"])
    assert ((normal * centre).sum(axis=1) > 0).all(), "a face wound inwards"
    radius = np.linalg.norm(m["xyz"].astype(np.float64), axis=1)
    print(f"sphere min_frames {min_frames}: radii {radius.min():.5f} .. {radius.max():.5f}, band {SPHERE_BAND}")
    assert SPHERE_BAND[0] <= radius.min() and radius.max() <= SPHERE_BAND[1]
    assert m["rgba"][:, 3].min() >= min_frames and m["rgba"][:, :3].max() > 0


def test_the_bars_are_twice_what_float64_measures():
    m = _fuse_sphere(exact=True).extract(1)
    radius = np.linalg.norm(m["xyz"], axis=1)
    assert 0 <= SPHERE_BAND[0] - (1 - 2 * (1 - radius.min())) < 2e-5 and 0 <= (1 + 2 * (radius.max() - 1)) - SPHERE_BAND[1] < 2e-5
    m = _fuse_plane(exact=True).extract(2)
    dist = np.abs(m["xyz"] @ T.PLANE_NORMAL - T.PLANE_OFFSET) / T.PLANE["voxel"]
    assert 0 <= 2 * dist.max() - PLANE_BAR < 2e-5


def test_plane_faces_the_camera_and_lies_on_the_plane(plane):
    m = plane.extract(2)
    assert len(m["keys"]) > 100 and len(m["quads"]) > 100
    normal, _ = T.quad_normals(m["xyz"], m["quads"])
    assert (normal @ np.array([0.0, 0.0, 1.0]) < 0).all(), "a face turned away from the first camera"
    dist = np.abs(m["xyz"].astype(np.float64) @ T.PLANE_NORMAL - T.PLANE_OFFSET) / T.PLANE["voxel"]
    print(f"plane: max distance {dist.max():.5f} voxel, bar {PLANE_BAR}")
    assert dist.max() <= np.sqrt(3.0), "a sign-changing cell contains the zero set"
    assert dist.max() <= PLANE_BAR
    tri = m["triangles"].reshape(-1, 2, 3)
    assert np.array_equal(tri[:, 0], m["quads"][:, [0, 1, 2]]) and np.array_equal(tri[:, 1], m["quads"][:, [0, 2, 3]])
    assert m["quads_dropped"] > 0, "an open surface has a rim"


def test_free_space_carves_a_surface_away():
    """A wall at 3 m in one frame, then at 5 m in two more: the voxels behind the first wall, negative at first, are seen as free
    space twice, change sign and leave the mesh."""
    h, w, f, c = 16, 16, (16.0, 16.0), (8.0, 8.0)
    pose = np.array([1.0, 0, 0, 0, 0, 0, 0])
    rgb = np.full((h, w, 3), 0.5, np.float32)
    vol = T.TsdfVolume(0.25, 3, 1.0, 80.0)
    vol.frame(np.full((h, w), 3.0, np.float32), rgb, f, c, pose)
    behind = T.pack(0, 0, 12)                                                    # centre z = 3.125: 0.125 m behind the wall
    assert vol.records[behind][0] < 0 and vol.records[behind][1] == 1
    first = vol.extract(1)
    near3 = np.abs(first["xyz"][:, 2] - 3.0) < 0.5
    assert near3.sum() > 20 and near3.all()
    for _ in range(2):
        vol.frame(np.full((h, w), 5.0, np.float32), rgb, f, c, pose)
    S, n, _, _, _, nc = vol.records[behind]
    assert n == 3 and S > 0 and nc == 1, "two free-space observations of +1 outweigh one of -1/6"
    later = vol.extract(1)
    assert len(later["keys"]) > 20 and (np.abs(later["xyz"][:, 2] - 5.0) < 0.5).all(), "the first wall is still in the mesh"


def test_keys_samples_and_colour_rules():
    assert T.pack(-T.HALF, T.HALF - 1, 0) == (T.HALF * 2 - 1) << 21 | T.HALF and T.pack(T.HALF - 1, T.HALF - 1, T.HALF - 1) == (1 << 63) - 1
    assert T.unpack(T.pack(-3, 0, 7)) == (-3, 0, 7) and T.pack(0, 0, 0) != T.EMPTY
    assert T.rgb_bytes(np.array([np.nan, -1.0, 0.5, 2.0], np.float32)).tolist() == [0, 0, 128, 255]
    # one pixel, one ray along +z from the origin: 4K+1 samples half a voxel apart, those with z <= 0 left out
    vol = T.TsdfVolume(1.0, 2, 0.5, 80.0).allocate(np.array([[1.25]], np.float32), (1.0, 1.0), (0.5, 0.5), [1, 0, 0, 0, 0, 0, 0])
    assert sorted(T.unpack(k) for k in vol.records) == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3)]       # z = 0.25 .. 3.25
    far = T.TsdfVolume(1.0, 2, 0.5, 80.0).allocate(np.array([[2.0]], np.float32), (1.0, 1.0), (0.5, 0.5),
                                                   [1, 0, 0, 0, 0, 0, float(T.HALF) - 3.5])
    assert far.dropped_range == 2 and sorted(T.unpack(k)[2] for k in far.records) == [T.HALF - 3, T.HALF - 2, T.HALF - 1]
    nan = T.TsdfVolume(1.0, 2).frame(np.array([[2.0]], np.float32), np.zeros((1, 1, 3), np.float32), (1.0, 1.0), (0.5, 0.5),
                                     [np.nan, 0, 0, 0, 0, 0, 0])
    assert not nan.records and nan.stats() == {"occupied": 0, "dropped_range": 0, "dropped_full": 0, "updates": 0}
