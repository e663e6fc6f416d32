"""The numpy restatement of m4d_tsdf_raycast (tests/tsdf_raycast_ref.py) held to analytic scenes, so that the bit-for-bit GPU tests
of tests/test_gpu_tsdf_raycast.py inherit a meaning; and the entry's refusals on host pointers that are never dereferenced.

Measured with this restatement (error = rendered - analytic z-depth in voxels over the pixels both have; samples = positions
sampled per pixel, both modes of the coarse-to-fine march):

  plane 24x32, voxel 0.25, K 3, frames 0..3 fused, range 1..80
    pose      min_frames  window  hit share of valid  max |e|  mean |e|  mean e   samples/pixel  hits without a surface
    fused 3   1           -       0.9245              0.6983   0.1948    -0.0190  21.7           0
    fused 3   1           2       0.9219              0.6261   0.1919    -0.0174  14.0           0
    fused 3   2           -       0.8607              0.6983   0.1943    -0.0194  27.8           0
    fused 3   2           2       0.8646              0.6261   0.1942    -0.0159  13.3           0
    novel     1           -       0.7005              0.9613   0.1985    -0.0250  42.4           0
    novel     1           2       0.7031              0.6710   0.2057    -0.0276  11.5           0
    novel     2           -       0.6536              0.9613   0.1963    -0.0282  46.5           0
    novel     2           2       0.6510              0.6710   0.2029    -0.0319  10.6           0
  (the windowed march is guided by the analytic depth)
  sphere 48x48, voxel 0.125, K 2, 26 views, min_frames 2, range 0.5..10; 904 pixels inside the analytic silhouette
    pose         hit share  max |e|  mean |e|  mean e   rendered outside the silhouette  samples/pixel
    fused view   1.0000     1.4833   0.3467    -0.1618  114                              32.1
    novel view   1.0000     2.0924   0.3517    -0.1298  92                               32.4
  (outside the silhouette: the sphere dilated by its voxels)

The bars are these figures times 1.5 (errors) and minus 0.05 (hit shares).  A plane whose maximum exceeded one voxel or whose
mean exceeded 0.3 voxel would mean the restatement is wrong."""
import ctypes

import numpy as np
import pytest

import tsdf_mesh_ref as T
import tsdf_raycast_ref as RC

NOVEL_SPHERE_EYE = 3.0 * np.array([0.5, 0.3, -1.0]) / np.linalg.norm([0.5, 0.3, -1.0])


@pytest.fixture(scope="module")
def plane_volume():
    P = T.PLANE
    return T.fuse(T.plane_frames(n=4), T.PLANE_F, T.PLANE_C, P["voxel"], P["trunc"], P["near"], P["far"])


@pytest.fixture(scope="module")
def sphere_volume():
    S = T.SPHERE
    return T.fuse(T.sphere_frames(), S["f"], S["c"], S["voxel"], S["trunc"], S["near"], S["far"])


def _errors(depth, truth, valid, voxel):
    hit = np.isfinite(depth)
    e = (depth[hit & valid].astype(np.float64) - truth[hit & valid]) / voxel
    return hit, e


#            pose      min_frames window  share   max     mean
PLANE_CASES = [("fused", 1, None, 0.9245, 0.6983, 0.1948), ("fused", 1, 2, 0.9219, 0.6261, 0.1919),
               ("fused", 2, None, 0.8607, 0.6983, 0.1943), ("fused", 2, 2, 0.8646, 0.6261, 0.1942),
               ("novel", 1, None, 0.7005, 0.9613, 0.1985), ("novel", 1, 2, 0.7031, 0.6710, 0.2057),
               ("novel", 2, None, 0.6536, 0.9613, 0.1963), ("novel", 2, 2, 0.6510, 0.6710, 0.2029)]


@pytest.mark.parametrize("which,min_frames,window,share,e_max,e_mean", PLANE_CASES)
def test_plane_renders_within_a_voxel(plane_volume, which, min_frames, window, share, e_max, e_mean):
    P = T.PLANE
    pose = T.plane_poses(4)[3] if which == "fused" else T.plane_poses(6)[5]
    truth = T.render_plane(pose, T.PLANE_F, T.PLANE_C, P["h"], P["w"], T.PLANE_NORMAL, T.PLANE_OFFSET)
    valid = np.isfinite(truth) & (truth >= P["near"]) & (truth <= P["far"])
    assert valid.sum() > 700
    depth, hits = RC.raycast(plane_volume.records, T.PLANE_F, T.PLANE_C, pose, P["h"], P["w"], P["voxel"], P["trunc"], min_frames,
                             P["near"], P["far"], guide=truth if window else None, window=window)
    hit, e = _errors(depth, truth, valid, P["voxel"])
    print(which, min_frames, window, (hit & valid).sum() / valid.sum(), np.abs(e).max(), np.abs(e).mean(), e.mean())
    assert hits == hit.sum() and not (hit & ~valid).any()
    assert (hit & valid).sum() / valid.sum() >= share - 0.05
    assert np.abs(e).max() <= min(1.5 * e_max, 1.0) and np.abs(e).mean() <= min(1.5 * e_mean, 0.3)
    assert abs(e.mean()) < 0.1, "the signed error is unbiased"


@pytest.mark.parametrize("which,share,e_max,e_mean,outside", [("fused", 1.0, 1.4833, 0.3467, 114), ("novel", 1.0, 2.0924, 0.3517, 92)])
def test_sphere_renders_its_front(sphere_volume, which, share, e_max, e_mean, outside):
    S = T.SPHERE
    pose = T.sphere_frames()[0][2] if which == "fused" else T.look_at_pose(NOVEL_SPHERE_EYE)
    truth = T.render_sphere(pose, S["f"], S["c"], S["h"], S["w"])
    valid = np.isfinite(truth)
    depth, hits = RC.raycast(sphere_volume.records, S["f"], S["c"], pose, S["h"], S["w"], S["voxel"], S["trunc"], 2, S["near"], S["far"])
    hit, e = _errors(depth, truth, valid, S["voxel"])
    print(which, (hit & valid).sum() / valid.sum(), np.abs(e).max(), np.abs(e).mean(), e.mean(), (hit & ~valid).sum())
    assert hits == hit.sum()
    assert (hit & valid).sum() / valid.sum() >= share - 0.05
    assert np.abs(e).max() <= 1.5 * e_max and np.abs(e).mean() <= 1.5 * e_mean
    assert (hit & ~valid).sum() <= 1.5 * outside, "the silhouette is dilated by the voxels, no more"
    # every pixel rendered outside the silhouette touches it: within two pixels (0.33 voxel per pixel at 3 m) of a valid one
    grown = valid.copy()
    for _ in range(3):
        g = grown.copy()
        g[1:] |= grown[:-1]; g[:-1] |= grown[1:]; g[:, 1:] |= grown[:, :-1]; g[:, :-1] |= grown[:, 1:]
        grown = g
    assert not (hit & ~grown).any()


def test_nothing_known_renders_nothing(plane_volume):
    P = T.PLANE
    pose = T.plane_poses(4)[3]
    args = (T.PLANE_F, T.PLANE_C, pose, P["h"], P["w"], P["voxel"], P["trunc"])
    depth, hits = RC.raycast({}, *args, 1, P["near"], P["far"])
    assert hits == 0 and np.array_equal(depth.view(np.uint32), np.full((P["h"], P["w"]), 0x7FC00000, np.uint32))
    top = max(r[1] for r in plane_volume.records.values())
    fill = np.random.default_rng(3).random((P["h"], P["w"])).astype(np.float32)
    depth, hits = RC.raycast(plane_volume.records, *args, top + 1, P["near"], P["far"], fill=fill)
    assert hits == 0 and np.array_equal(depth, fill)
    depth, hits = RC.raycast(plane_volume.records, *args, top, P["near"], P["far"], fill=fill)
    assert 0 < hits == (depth != fill).sum()
    bad = np.array(pose)
    bad[5] = np.inf
    depth, hits = RC.raycast(plane_volume.records, T.PLANE_F, T.PLANE_C, bad, P["h"], P["w"], P["voxel"], P["trunc"], 1, fill=fill)
    assert hits == 0 and np.array_equal(depth, fill)


def _column(cells):
    """One-pixel camera looking along +z from the origin (ax = ay = 0), voxel 1, K 2, near 1: position i lies at z = 1 + i / 2 in
    cell (0, 0, floor(z)).  ``cells``: {z cell: (S, n)} -> the rendered depth (NaN: a miss)."""
    rec = {((0 + RC.HALF) << 42) | ((0 + RC.HALF) << 21) | (z + RC.HALF): [np.float32(S), n, 0, 0, 0, 0] for z, (S, n) in cells.items()}
    depth, hits = RC.raycast(rec, (1.0, 1.0), (0.5, 0.5), [1, 0, 0, 0, 0, 0, 0], 1, 1, 1.0, 2, 1, near=1.0, far=20.0)
    assert hits == int(np.isfinite(depth[0, 0]))
    return depth[0, 0]


def test_the_march_rule_on_a_hand_made_column():
    """Cells 5..8 lie beyond the first coarse positions (i = 0, 4, 8 -> z = 1, 3, 5): the walk backs up from the known coarse
    sample at z = 5 to just after the unknown one at z = 3."""
    # + + - : the crossing between the last sample of cell 6 (z = 6.5) and the first of cell 7 (z = 7.0)
    want = np.float32(6.5 + 0.5 * float(np.float32(0.5) / (np.float32(0.5) - np.float32(-0.25))))
    assert _column({5: (0.75, 1), 6: (0.5, 1), 7: (-0.25, 1)}) == want
    assert _column({5: (1.5, 2), 6: (1.0, 2), 7: (-0.5, 2)}) == want                 # D = S / n
    assert _column({4: (0.9, 1), 5: (0.75, 1), 6: (0.5, 1), 7: (-0.25, 1)}) == want     # a wider band in front
    assert _column({6: (0.0, 1), 7: (-0.25, 1)}) == np.float32(6.5)                  # prev = 0 counts as outside: t = 0
    # a crossing across an unknown sample is none
    assert np.isnan(_column({5: (0.75, 1), 7: (-0.25, 1)}))
    assert np.isnan(_column({5: (0.75, 1), 6: (0.5, 0), 7: (-0.25, 1)}))             # n = 0: allocated, never updated
    # a back face (inside to outside) is none; the front face behind it is
    assert np.isnan(_column({5: (-0.75, 1), 6: (-0.5, 1), 7: (0.25, 1)}))
    assert _column({5: (-0.75, 1), 6: (0.5, 1), 7: (0.5, 1), 8: (-0.5, 1)}) == np.float32(7.5 + 0.5 * 0.5)
    # a gap of 2K unknown positions returns to the coarse march, which finds the surface behind it
    far_wall = {5: (0.75, 1), 12: (0.5, 1), 13: (-0.5, 1)}
    assert _column(far_wall) == np.float32(12.5 + 0.5 * 0.5)
    # the first crossing wins
    assert _column({5: (0.5, 1), 6: (-0.5, 1), 7: (0.5, 1), 8: (-0.5, 1)}) == np.float32(5.5 + 0.5 * 0.5)


def test_a_camera_inside_the_surface_sees_no_back_face(sphere_volume):
    """From inside the sphere's band, looking out: every ray leaves through the surface from behind.  The same rays do hit once
    the field's sign is flipped, so the band is there and known."""
    S = T.SPHERE
    pose = T.look_at_pose(np.array([0.0, 0.0, 0.9]), target=(0.0, 0.0, 2.0))
    args = (S["f"], S["c"], pose, S["h"], S["w"], S["voxel"], S["trunc"], 1, 0.02, S["far"])
    depth, hits = RC.raycast(sphere_volume.records, *args)
    assert hits == 0 and np.isnan(depth).all()
    flipped = {k: [-r[0]] + r[1:] for k, r in sphere_volume.records.items()}
    depth, hits = RC.raycast(flipped, *args)
    centre = depth[16:32, 16:32]
    assert np.isfinite(centre).all() and np.abs(centre - 0.1).max() < 2 * S["voxel"]


def test_entry_refuses_bad_arguments_without_a_launch():
    """Every refusal include/m4depth_hip.h lists for m4d_tsdf_raycast, on host pointers that are never dereferenced."""
    from m4depth_amd._lib import lib
    buf = (ctypes.c_ulonglong * 64)()
    p = ctypes.addressof(buf)
    p += p % 16
    ok = dict(state=p, b=1, L=6, f=p, c=p, pose=p, h=3, w=4, near=1.0, far=80.0, voxel=0.05, trunc=4, min_frames=1, guide=None, gs=0,
              window=0, fill=None, fs=0, out=p, os=12, hits=None)

    def raycast(**kw):
        a = dict(ok, **kw)
        return lib.m4d_tsdf_raycast(a["state"], a["b"], a["L"], a["f"], a["c"], a["pose"], a["h"], a["w"], a["near"], a["far"],
                                    a["voxel"], a["trunc"], a["min_frames"], a["guide"], a["gs"], a["window"], a["fill"], a["fs"],
                                    a["out"], a["os"], a["hits"], None)

    bad = (dict(state=None), dict(f=None), dict(c=None), dict(pose=None), dict(out=None), dict(b=0), dict(b=65536), dict(L=5),
           dict(L=27), dict(h=0), dict(w=0), dict(h=4097, w=4097, os=1 << 25), dict(far=1.0), dict(far=0.5), dict(far=float("nan")),
           dict(near=float("nan")), dict(near=0.0), dict(near=-1.0), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")),
           dict(voxel=float("inf")), dict(trunc=1), dict(trunc=9), dict(min_frames=0), dict(guide=p, gs=12, window=0),
           dict(guide=p, gs=12, window=-1), dict(voxel=1e-4), dict(near=1.0, far=1.0 + 0.025 * (1 << 20) + 1.0), dict(os=11),
           dict(guide=p, gs=11, window=1), dict(fill=p, fs=11), dict(f=p + 2), dict(c=p + 2), dict(out=p + 2),
           dict(guide=p + 2, gs=12, window=1), dict(fill=p + 2, fs=12), dict(state=p + 4), dict(pose=p + 4), dict(hits=p + 4))
    for kw in bad:
        assert raycast(**kw) == 1, kw
    # the value refusals are the restatement's
    for kw in bad:
        a = dict(ok, **kw)
        names = set(kw) - {"os"}
        if names and names <= {"h", "w", "near", "far", "voxel", "trunc", "min_frames"}:
            assert RC.refused(a["h"], a["w"], a["near"], a["far"], a["voxel"], a["trunc"], a["min_frames"]), kw
    assert not RC.refused(3, 4, 1.0, 80.0, 0.05, 4, 1, 1)
    assert RC.refused(3, 4, 1.0, 80.0, 0.05, 4, 1, 0)
    # the bound itself: (far - near) / (voxel / 2) = 2^20 exactly passes the value checks (refused only by a later one here)
    assert not RC.refused(3, 4, 1.0, 1.0 + 0.125 * (1 << 20), 0.25, 4, 1) and RC.refused(3, 4, 1.0, 1.5 + 0.125 * (1 << 20), 0.25, 4, 1)
    assert raycast(near=1.0, far=1.5 + 0.125 * (1 << 20), voxel=0.25) == 1


def test_op_refuses_bad_arguments():
    import torch
    from m4depth_amd import network_ops as nops
    words = torch.zeros(4 + 4 * 64, dtype=torch.int64)
    state = nops.tsdf_state_views(words, 1, 6)
    f, c, pose = torch.ones((1, 2)), torch.ones((1, 2)), torch.zeros((1, 7), dtype=torch.float64)
    ok = dict(h=3, w=4, voxel=0.05, trunc=4, min_frames=1)

    def call(**kw):
        a = dict(ok, **kw)
        return nops.tsdf_raycast(state, a.pop("f", f), a.pop("c", c), a.pop("pose", pose), **a)

    for kw, match in ((dict(voxel=0.0), "voxel must be"), (dict(voxel=float("nan")), "voxel must be"), (dict(trunc=1), "trunc must be in 2..8"),
                      (dict(trunc=9), "trunc must be in 2..8"), (dict(min_frames=0), "min_frames must be >= 1"),
                      (dict(h=0), "need h, w >= 1"), (dict(h=4097, w=4097), "need h, w >= 1"), (dict(far=1.0), "need 0 < near < far"),
                      (dict(near=0.0), "need 0 < near < far"), (dict(near=float("nan")), "need 0 < near < far"),
                      (dict(voxel=1e-4), "more than 2\\^20 half voxels"), (dict(window=2), "come together or not at all"),
                      (dict(guide=torch.zeros((1, 3, 4, 1))), "come together or not at all"),
                      (dict(guide=torch.zeros((1, 3, 4, 1)), window=0), "window must be >= 1"),
                      (dict(f=torch.ones((2, 2))), "cam_f / cam_c"), (dict(pose=torch.zeros((1, 7))), "pose: expected"),
                      (dict(hits=torch.zeros(2, dtype=torch.int64)), "hits: expected")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    with pytest.raises(ValueError, match="not a tsdf_state"):
        nops.tsdf_raycast(dict(state, b=2), f, c, pose, **ok)
    with pytest.raises(TypeError, match="out: expected a float32 device tensor"):      # no CPU path: refused before the library
        call(out=torch.zeros((1, 3, 4, 1)))
