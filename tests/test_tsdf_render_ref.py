"""The numpy restatement of m4d_tsdf_render (tests/tsdf_render_ref.py) held to analytic scenes, so that the bit-for-bit GPU tests of
tests/test_gpu_tsdf_render.py inherit a meaning; the entry's and the op's refusals on host pointers that are never dereferenced;
the host side of --fused_interp / --save_fused_view.

Measured with this restatement, float32 as the header states it (error = rendered - analytic z-depth in voxels over the pixels
both have; normals: share of the hit pixels that have one, angle to the analytic normal in degrees):

  plane 24x32, voxel 0.25, K 3, frames 0..3 fused, range 1..80; nearest -> trilinear
    pose   min_frames window  hit share         max |e|           mean |e|          mean e    normals: share  mean   max
    fused  1          -       0.9245 -> 0.9245  0.6983 -> 0.4551  0.1948 -> 0.0429  0.0015    0.8479          1.65   5.41
    fused  1          2       0.9219 -> 0.9219  0.6261 -> 0.5962  0.1919 -> 0.0421  0.0019    0.8517          1.65   5.41
    fused  2          -       0.8607 -> 0.8594  0.6983 -> 0.4370  0.1943 -> 0.0399  0.0067    0.8606          1.59   5.41
    fused  2          2       0.8646 -> 0.8646  0.6261 -> 0.5747  0.1942 -> 0.0429  0.0067    0.8569          1.59   5.41
    novel  1          -       0.7005 -> 0.7005  0.9613 -> 0.6246  0.1985 -> 0.0500  0.0047    0.8439          1.76   5.02
    novel  1          2       0.7031 -> 0.7031  0.6710 -> 0.6246  0.2057 -> 0.0501  0.0057    0.8407          1.75   5.08
    novel  2          -       0.6536 -> 0.6536  0.9613 -> 0.6246  0.1963 -> 0.0514  0.0053    0.8466          1.70   5.02
    novel  2          2       0.6510 -> 0.6510  0.6710 -> 0.6246  0.2029 -> 0.0512  0.0080    0.8420          1.70   5.08
  (the windowed march is guided by the analytic depth; no case renders a pixel without a surface; samples per pixel 21.7 -> 21.8,
  42.4 -> 42.5: the KNOWN set is the nearest rule's)
  sphere 48x48, voxel 0.125, K 2, 26 views, min_frames 2, range 0.5..10; 904 pixels inside the analytic silhouette
    pose        hit share         max |e|           mean |e|          outside the silhouette  normals: share  mean  max
    fused view  1.0000 -> 1.0000  1.4833 -> 0.6264  0.3467 -> 0.0814  114 -> 20               1.0             7.43  23.58
    novel view  1.0000 -> 0.9989  2.0924 -> 0.9911  0.3517 -> 0.0948  92 -> 14                1.0             7.27  20.75
  (samples per pixel 32.1 -> 33.8; the projective distance bends the field of a sphere seen from 26 sides: the normals' error is
  the field's, a wrong gradient would show as tens of degrees on the plane too)

The bars are these figures times 1.5, next to the conditions on the two rules' ratio that do not depend on a figure."""
import ctypes
import os

import numpy as np
import pytest

from pose_ref import rot
import tsdf_mesh_ref as T
import tsdf_raycast_ref as RC
import tsdf_render_ref as RR

NOVEL_SPHERE_EYE = 3.0 * np.array([0.5, 0.3, -1.0]) / np.linalg.norm([0.5, 0.3, -1.0])
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def plane_volume():
    P = T.PLANE
    return T.fuse(T.plane_frames(n=4), T.PLANE_F, T.PLANE_C, P["voxel"], P["trunc"], P["near"], P["far"])


@pytest.fixture(scope="module")
def sphere_volume():
    S = T.SPHERE
    return T.fuse(T.sphere_frames(), S["f"], S["c"], S["voxel"], S["trunc"], S["near"], S["far"])


_cache = {}


def plane_render(volume, which, min_frames, window, interp):
    """(the restatement's records, the analytic depth, its valid mask, the pose): computed once per case."""
    key = ("plane", which, min_frames, window, interp)
    if key not in _cache:
        P = T.PLANE
        pose = T.plane_poses(4)[3] if which == "fused" else T.plane_poses(6)[5]
        truth = T.render_plane(pose, T.PLANE_F, T.PLANE_C, P["h"], P["w"], T.PLANE_NORMAL, T.PLANE_OFFSET)
        valid = np.isfinite(truth) & (truth >= P["near"]) & (truth <= P["far"])
        res = RR.render(volume.records, T.PLANE_F, T.PLANE_C, pose, P["h"], P["w"], P["voxel"], P["trunc"], min_frames, P["near"],
                        P["far"], guide=truth if window else None, window=window, interp=interp)
        _cache[key] = (res, truth, valid, pose)
    return _cache[key]


def sphere_render(volume, which, interp):
    key = ("sphere", which, interp)
    if key not in _cache:
        S = T.SPHERE
        pose = T.sphere_frames()[0][2] if which == "fused" else T.look_at_pose(NOVEL_SPHERE_EYE)
        truth = T.render_sphere(pose, S["f"], S["c"], S["h"], S["w"])
        res = RR.render(volume.records, S["f"], S["c"], pose, S["h"], S["w"], S["voxel"], S["trunc"], 2, S["near"], S["far"], interp=interp)
        _cache[key] = (res, truth, np.isfinite(truth), pose)
    return _cache[key]


def _errors(depth, truth, valid, voxel):
    hit = np.isfinite(depth)
    return hit, (depth[hit & valid].astype(np.float64) - truth[hit & valid]) / voxel


def _angles(res, analytic, on):
    """(mask of the pixels of ``on`` with a normal, their angles to ``analytic`` [h,w,3] in degrees)."""
    n = res["normal"].astype(np.float64)
    have = np.isfinite(n).all(-1) & on
    assert not (np.isnan(n).any(-1) & ~np.isnan(n).all(-1)).any(), "a normal is there or not, whole"
    return have, np.degrees(np.arccos(np.clip((n[have] * analytic[have]).sum(-1), -1.0, 1.0)))


def _view_dirs(f, c, h, w):
    col, row = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    ax = (((col + F(0.5)) - F(c[0])) / F(f[0])).astype(np.float64)
    ay = (((row + F(0.5)) - F(c[1])) / F(f[1])).astype(np.float64)
    return ax, ay


#            pose   min_frames window  share   max     mean    normals: share, mean, max
PLANE_CASES = [("fused", 1, None, 0.9245, 0.4551, 0.0429, 0.8479, 1.65, 5.41), ("fused", 1, 2, 0.9219, 0.5962, 0.0421, 0.8517, 1.65, 5.41),
               ("fused", 2, None, 0.8594, 0.4370, 0.0399, 0.8606, 1.59, 5.41), ("fused", 2, 2, 0.8646, 0.5747, 0.0429, 0.8569, 1.59, 5.41),
               ("novel", 1, None, 0.7005, 0.6246, 0.0500, 0.8439, 1.76, 5.02), ("novel", 1, 2, 0.7031, 0.6246, 0.0501, 0.8407, 1.75, 5.08),
               ("novel", 2, None, 0.6536, 0.6246, 0.0514, 0.8466, 1.70, 5.02), ("novel", 2, 2, 0.6510, 0.6246, 0.0512, 0.8420, 1.70, 5.08)]


@pytest.mark.parametrize("which,min_frames,window", [c[:3] for c in PLANE_CASES])
def test_nearest_is_the_raycast_bit_for_bit_on_the_plane(plane_volume, which, min_frames, window):
    P = T.PLANE
    res, truth, _, pose = plane_render(plane_volume, which, min_frames, window, 0)
    want, hits = RC.raycast(plane_volume.records, T.PLANE_F, T.PLANE_C, pose, P["h"], P["w"], P["voxel"], P["trunc"], min_frames,
                            P["near"], P["far"], guide=truth if window else None, window=window)
    assert hits > 300 and res["hits"] == hits and np.array_equal(bits(res["depth"]), bits(want))


@pytest.mark.parametrize("which", ["fused", "novel"])
def test_nearest_is_the_raycast_bit_for_bit_on_the_sphere(sphere_volume, which):
    S = T.SPHERE
    res, _, _, pose = sphere_render(sphere_volume, which, 0)
    want, hits = RC.raycast(sphere_volume.records, S["f"], S["c"], pose, S["h"], S["w"], S["voxel"], S["trunc"], 2, S["near"], S["far"])
    assert hits > 900 and res["hits"] == hits and np.array_equal(bits(res["depth"]), bits(want))


@pytest.mark.parametrize("which,min_frames,window,share,e_max,e_mean,n_share,a_mean,a_max", PLANE_CASES)
def test_trilinear_plane(plane_volume, which, min_frames, window, share, e_max, e_mean, n_share, a_mean, a_max):
    voxel = T.PLANE["voxel"]
    near_res, truth, valid, pose = plane_render(plane_volume, which, min_frames, window, 0)
    res = plane_render(plane_volume, which, min_frames, window, 1)[0]
    hit0, e0 = _errors(near_res["depth"], truth, valid, voxel)
    hit, e = _errors(res["depth"], truth, valid, voxel)
    got_share, share0 = (hit & valid).sum() / valid.sum(), (hit0 & valid).sum() / valid.sum()
    R = np.array(rot(pose), np.float64)
    n_cam = R.T @ np.asarray(T.PLANE_NORMAL, np.float64)
    n_cam = -n_cam if n_cam[2] > 0 else n_cam                   # towards the camera
    have, ang = _angles(res, np.broadcast_to(n_cam / np.linalg.norm(n_cam), res["normal"].shape), hit & valid)
    print(which, min_frames, window, got_share, np.abs(e).max(), np.abs(e).mean(), e.mean(), have.sum() / (hit & valid).sum(), ang.mean(), ang.max())
    assert res["hits"] == hit.sum() and not (hit & ~valid).any(), "no hit without a surface"
    # against the nearest rule
    assert np.abs(e).mean() <= 0.5 * np.abs(e0).mean() and np.abs(e).max() <= np.abs(e0).max()
    assert abs(got_share - share0) <= 0.01 and abs(e.mean()) < 0.1
    # against the measured figures
    assert got_share >= share - 0.05 and np.abs(e).max() <= 1.5 * e_max and np.abs(e).mean() <= 1.5 * e_mean
    # normals
    n = res["normal"].astype(np.float64)
    assert have.sum() >= 0.75 * (hit & valid).sum() and have.sum() >= (n_share - 0.05) * (hit & valid).sum()
    assert not np.isfinite(n[~hit]).any(), "a miss has no normal"
    assert np.abs(np.linalg.norm(n[have], axis=-1) - 1.0).max() <= 1e-6
    ax, ay = _view_dirs(T.PLANE_F, T.PLANE_C, T.PLANE["h"], T.PLANE["w"])
    assert ((n[..., 0] * ax + n[..., 1] * ay + n[..., 2])[have] < 0).all(), "the normals face the camera"
    assert ang.mean() <= 1.5 * a_mean and ang.max() <= 1.5 * a_max


@pytest.mark.parametrize("which,share,e_max,e_mean,outside,a_mean,a_max",
                         [("fused", 1.0, 0.6264, 0.0814, 20, 7.43, 23.58), ("novel", 0.9989, 0.9911, 0.0948, 14, 7.27, 20.75)])
def test_trilinear_sphere(sphere_volume, which, share, e_max, e_mean, outside, a_mean, a_max):
    S = T.SPHERE
    near_res, truth, valid, pose = sphere_render(sphere_volume, which, 0)
    res = sphere_render(sphere_volume, which, 1)[0]
    hit0, e0 = _errors(near_res["depth"], truth, valid, S["voxel"])
    hit, e = _errors(res["depth"], truth, valid, S["voxel"])
    dw, o = T._rays(pose, S["f"], S["c"], S["h"], S["w"])
    pw = o + dw * np.where(valid, truth, 1.0).astype(np.float64)[..., None]
    n_cam = (pw / np.linalg.norm(pw, axis=-1, keepdims=True)) @ np.array(rot(pose), np.float64)      # R^T of the outward normal
    have, ang = _angles(res, n_cam, hit & valid)
    print(which, (hit & valid).sum() / valid.sum(), np.abs(e).max(), np.abs(e).mean(), e.mean(), (hit & ~valid).sum(), ang.mean(), ang.max())
    assert res["hits"] == hit.sum()
    assert np.abs(e).mean() <= 0.5 * np.abs(e0).mean() and 2 * (hit & ~valid).sum() <= (hit0 & ~valid).sum()
    assert (hit & valid).sum() / valid.sum() >= share - 0.05
    assert np.abs(e).max() <= 1.5 * e_max and np.abs(e).mean() <= 1.5 * e_mean and (hit & ~valid).sum() <= 1.5 * outside
    n = res["normal"].astype(np.float64)
    assert np.isfinite(n[hit]).all() and not np.isfinite(n[~hit]).any(), "every hit pixel of the sphere has a normal, no miss has"
    assert np.abs(np.linalg.norm(n[hit], axis=-1) - 1.0).max() <= 1e-6
    assert ang.mean() <= 1.5 * a_mean and ang.max() <= 1.5 * a_max


COLOUR = (0.2, 0.6, 0.8)


def _has_colour(records, f, c, pose, z_star, voxel, min_frames):
    """bool [h,w]: the header's condition for a colour at the surface point of every pixel with a finite ``z_star``."""
    h, w = z_star.shape
    R, t = [[float(v) for v in r] for r in rot(pose)], [float(v) for v in pose[4:]]
    voxel = float(F(voxel))

    def with_colour(cell):
        if not all(-RC.HALF <= i < RC.HALF for i in cell):
            return False
        rec = records.get(((cell[0] + RC.HALF) << 42) | ((cell[1] + RC.HALF) << 21) | (cell[2] + RC.HALF))
        return rec is not None and rec[1] >= min_frames and rec[1] > 0 and rec[5] > 0

    out = np.zeros((h, w), bool)
    for row, col in np.argwhere(np.isfinite(z_star)).tolist():
        z = float(z_star[row, col])
        X, Y = float((F(col) + F(0.5) - F(c[0])) / F(f[0])) * z, float((F(row) + F(0.5) - F(c[1])) / F(f[1])) * z
        q = [(((R[j][0] * X + R[j][1] * Y) + R[j][2] * z) + t[j]) / voxel for j in range(3)]
        base = [int(np.floor(v - 0.5)) for v in q]
        around = all(with_colour((base[0] + dx, base[1] + dy, base[2] + dz)) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
        out[row, col] = around or with_colour(tuple(int(np.floor(v)) for v in q))
    return out


@pytest.mark.parametrize("interp", [0, 1])
def test_colour_and_view_of_a_one_colour_volume(interp):
    """Frames of one colour: every hit pixel has it, the view is the stated shading of it, a miss is NaN / 0."""
    P = T.PLANE
    frames = [(d, np.broadcast_to(np.array(COLOUR, F), rgb.shape).copy(), pose) for d, rgb, pose in T.plane_frames(n=4)]
    vol = T.fuse(frames, T.PLANE_F, T.PLANE_C, P["voxel"], P["trunc"], P["near"], P["far"])
    pose = T.plane_poses(6)[5]
    res = RR.render(vol.records, T.PLANE_F, T.PLANE_C, pose, P["h"], P["w"], P["voxel"], P["trunc"], 1, P["near"], P["far"], interp=interp)
    hit = np.isfinite(res["depth"])
    assert 300 < hit.sum() < hit.size
    want = T.rgb_bytes(np.array(COLOUR, F)).astype(np.float64) / 255.0
    # A hit pixel has a colour exactly when the eight voxels around its surface point are all KNOWN with nc > 0, or the voxel the
    # point lies in is -- worked out here from the records and z*, not by ``render``.  3 of the 538 hit pixels of this view, on
    # the rim of what the frames saw, have none: the crossing between two known half-voxel samples falls into a third voxel that
    # was allocated and never integrated (n = 0), so it is not KNOWN.  They are the grey ones of the view.
    coloured = np.isfinite(res["colour"]).all(-1)
    expected = _has_colour(vol.records, T.PLANE_F, T.PLANE_C, pose, res["z_star"], P["voxel"], 1)
    assert np.array_equal(coloured, expected) and not (coloured & ~hit).any() and (hit & ~coloured).any()
    assert not np.isnan(res["colour"][coloured]).any() and (np.isnan(res["colour"]).all(-1) | coloured).all()
    assert np.abs(res["colour"][coloured].astype(np.float64) - want).max() <= 1.0 / 255.0
    assert (bits(res["colour"][~coloured]) == 0x7FC00000).all()
    assert (bits(res["colour"][~hit]) == 0x7FC00000).all() and (bits(res["normal"][~hit]) == 0x7FC00000).all()
    assert (res["view"][~hit] == 0).all()
    n = res["normal"].astype(np.float64)
    have = np.isfinite(n).all(-1)
    assert have[hit].mean() > 0.75 and not have[hit].all(), "shaded pixels and pixels next to unknown space"
    ax, ay = _view_dirs(T.PLANE_F, T.PLANE_C, P["h"], P["w"])
    dot = ((n[..., 0] * ax + n[..., 1] * ay) + n[..., 2]) / np.sqrt((ax * ax + ay * ay) + 1.0)
    shade = np.where(have, 0.25 + 0.75 * np.maximum(0.0, -np.where(have, dot, 0.0)), 1.0).astype(F)
    assert (shade[have & hit] > 0.25).all() and (shade <= 1.0).all(), "a front face is lit"
    view = T.rgb_bytes(np.where(coloured[..., None], res["colour"], F(0.5)) * shade[..., None])
    assert np.array_equal(res["view"][hit], view[hit].astype(np.uint8))
    # a record nobody coloured (nc = 0) is grey in the view and NaN in the colour
    bare = {k: r[:2] + [0, 0, 0, 0] for k, r in vol.records.items()}
    res = RR.render(bare, T.PLANE_F, T.PLANE_C, pose, P["h"], P["w"], P["voxel"], P["trunc"], 1, P["near"], P["far"], interp=interp)
    assert np.array_equal(np.isfinite(res["depth"]), hit) and (bits(res["colour"]) == 0x7FC00000).all()
    assert np.array_equal(res["view"][hit], T.rgb_bytes(F(0.5) * shade[..., None] * np.ones(3, F))[hit].astype(np.uint8))


# ---- a hand-made column ----------------------------------------------------------------------------------------------------------
def column_case(layers, shift=(0, 0, 0), drop=(), x0=None, wrapped=False):
    """A one-pixel camera looking along +z (ax = ay = 0), voxel 1, K 2, near 1: position i lies at z = 1 + i / 2.  The camera
    stands at (shift + (0, 0, 0)) voxels, or at x = x0: its ray runs along the edge between four columns of voxels, so the base
    cell of every sample is (X - 1, Y - 1, .) with fractions (0.5, 0.5, .).  ``layers``: {z cell: D} for all four columns;
    ``drop``: (dx, dy, z cell) corners to leave out, dx / dy in {0, 1} from the base; ``wrapped``: the four-column block is also
    stored 2^21 cells further in x (where a wrapped index would find it).  -> (records, the arguments of ``render``)."""
    tx = float(shift[0]) if x0 is None else float(x0)
    bx, by = int(np.floor(tx - 0.5)), int(shift[1]) - 1
    rec = {}
    for z, D in layers.items():
        for dx in (0, 1):
            for dy in (0, 1):
                if (dx, dy, z) in drop:
                    continue
                for x in [bx + dx] + ([bx + dx + (1 << 21)] if wrapped else []):
                    if -RC.HALF <= x < RC.HALF:
                        rec[((x + RC.HALF) << 42) | ((by + dy + RC.HALF) << 21) | (z + int(shift[2]) + RC.HALF)] = [F(D), 1, 10, 20, 30, 1]
    pose = [1, 0, 0, 0, tx, float(shift[1]), float(shift[2])]
    return rec, ((1.0, 1.0), (0.5, 0.5), pose, 1, 1, 1.0, 2, 1)


def _column(interp, *a, **kw):
    rec, args = column_case(*a, **kw)
    res = RR.render(rec, *args, near=1.0, far=20.0, interp=interp)
    assert res["hits"] == int(np.isfinite(res["depth"][0, 0]))
    return res["depth"][0, 0]


LINEAR = {k: (6.25 - (k + 0.5)) * 0.25 for k in (4, 5, 6, 7, 8)}   # the field 0.25 (6.25 - z) at the voxel centres: a plane at z = 6.25


def test_the_trilinear_rule_on_a_hand_made_column():
    """The field is linear along z with its zero at 6.25.  The samples at z = 6.0 (base layer 5, fraction 0.5) and z = 6.5 (base
    layer 6, fraction 0) interpolate to +0.0625 and -0.0625: the crossing is exact.  The nearest rule sees -0.0625 (voxel 6) at
    z = 6.0 already, after +0.1875 (voxel 5) at z = 5.5."""
    nearest = F(5.5 + 0.5 * float(F(0.1875) / (F(0.1875) - F(-0.0625))))
    assert nearest == F(5.875)
    assert _column(0, LINEAR) == nearest
    assert _column(1, LINEAR) == F(6.25)
    # one corner of base layer 5 gone: the samples at z = 5.5 and z = 6.0 fall back to their nearest voxels, 5 and 6
    for dx, dy in ((0, 0), (1, 0), (0, 1)):
        assert _column(1, LINEAR, drop=[(dx, dy, 5)]) == nearest
    # ... and when the corner that is gone is the ray's own voxel 5 (column (1, 1)), both rules lose the samples in it: the
    # crossing lies across unknown space, which is none
    assert np.isnan(_column(1, LINEAR, drop=[(1, 1, 5)])) and np.isnan(_column(0, LINEAR, drop=[(1, 1, 5)]))
    # a corner of layer 7 gone: the sample at z = 6.5 falls back to voxel 6, which is what it interpolated to at fraction 0
    assert _column(1, LINEAR, drop=[(0, 0, 7)]) == F(6.25)
    # a field bent at voxel 6, by hand.  Every corner: z = 6.5 gives voxel 6 = 0.125 (fraction 0), z = 7.0 gives
    # (0.125 - 0.5) / 2 = -0.1875.  A corner of layer 7 gone: z = 6.5 is voxel 6 all the same, z = 7.0 is voxel 7 = -0.5
    bent = {4: 0.5, 5: 0.25, 6: 0.125, 7: -0.5, 8: -0.75}
    assert _column(1, bent) == F(6.5 + 0.5 * float(F(0.125) / (F(0.125) - F(-0.1875))))
    fallen = F(6.5 + 0.5 * float(F(0.125) / (F(0.125) - F(-0.5))))
    assert _column(1, bent, drop=[(0, 0, 7)]) == fallen and _column(0, bent) == fallen
    # the base cell straddles the world origin in x and y (cells -1 and 0): the same depth as three and two voxels further
    # (truncation instead of floor would look for cells 0 and 1, miss them and fall back to the nearest rule)
    assert _column(1, LINEAR, shift=(3, 2, 0)) == F(6.25) and _column(1, LINEAR, shift=(-4, -7, 0)) == F(6.25)
    assert _column(1, LINEAR, shift=(0, 0, -9)) == F(6.25), "the base layer below zero"
    # no interpolation in the coarse mode and none across unknown space: a lone layer pair far away is reached the same way
    assert np.isnan(_column(1, {5: 0.25, 7: -0.25}))


def test_a_corner_beyond_the_grid_is_missing_not_wrapped():
    """The camera 0.25 voxel inside the grid's low x end: the samples' cells are -2^20, their base cells -2^20 - 1.  A wrapped
    index would find the copy of the column at the grid's other end and interpolate; the rule says nearest."""
    x0 = -float(RC.HALF) + 0.25
    nearest = F(5.875)
    for wrapped in (False, True):
        assert _column(1, LINEAR, x0=x0, wrapped=wrapped) == nearest
        assert _column(0, LINEAR, x0=x0, wrapped=wrapped) == nearest
    # one voxel further in, every corner is on the grid: fractions (0.75, 0.5, .) of a field that does not depend on x
    assert _column(1, LINEAR, x0=x0 + 1.0) == F(6.25)
    # and at the high end: the base cell 2^20 - 1 has its upper corners at 2^20
    x1 = float(RC.HALF) - 0.25
    assert _column(1, LINEAR, x0=x1, wrapped=False) == nearest


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_without_a_launch():
    """Every refusal include/m4depth_hip.h lists for m4d_tsdf_render, on host pointers that are never dereferenced."""
    from m4depth_amd._lib import lib
    buf = (ctypes.c_ulonglong * 64)()
    p = ctypes.addressof(buf)
    p += p % 16
    ok = dict(state=p, b=1, L=6, f=p, c=p, pose=p, h=3, w=4, near=1.0, far=80.0, voxel=0.05, trunc=4, min_frames=1, guide=None, gs=0,
              window=0, fill=None, fs=0, interp=1, out=p, os=12, normal=p, ns=36, colour=p, cs=36, view=p, vs=36, hits=None)

    def render(**kw):
        a = dict(ok, **kw)
        return lib.m4d_tsdf_render(a["state"], a["b"], a["L"], a["f"], a["c"], a["pose"], a["h"], a["w"], a["near"], a["far"],
                                   a["voxel"], a["trunc"], a["min_frames"], a["guide"], a["gs"], a["window"], a["fill"], a["fs"],
                                   a["interp"], a["out"], a["os"], a["normal"], a["ns"], a["colour"], a["cs"], a["view"], a["vs"],
                                   a["hits"], None)

    raycast = (dict(state=None), dict(f=None), dict(c=None), dict(pose=None), dict(out=None), dict(b=0), dict(b=65536), dict(L=5),
               dict(L=27), dict(h=0), dict(w=0), dict(h=4097, w=4097, os=1 << 25, ns=1 << 27, cs=1 << 27, vs=1 << 27), dict(far=1.0),
               dict(far=0.5), dict(far=float("nan")), dict(near=float("nan")), dict(near=0.0), dict(near=-1.0), dict(voxel=0.0),
               dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(trunc=1), dict(trunc=9), dict(min_frames=0),
               dict(guide=p, gs=12, window=0), dict(guide=p, gs=12, window=-1), dict(voxel=1e-4),
               dict(near=1.0, far=1.0 + 0.025 * (1 << 20) + 1.0), dict(os=11), dict(guide=p, gs=11, window=1), dict(fill=p, fs=11),
               dict(f=p + 2), dict(c=p + 2), dict(out=p + 2), dict(guide=p + 2, gs=12, window=1), dict(fill=p + 2, fs=12),
               dict(state=p + 4), dict(pose=p + 4), dict(hits=p + 4))
    own = (dict(interp=-1), dict(interp=2), dict(ns=35), dict(cs=35), dict(vs=35), dict(ns=0), dict(normal=p + 2), dict(colour=p + 2),
           dict(normal=p + 1), dict(colour=p + 3))
    for kw in raycast + own:
        assert render(**kw) == 1, kw
        assert render(**dict(kw, interp=kw.get("interp", 0))) == 1, kw


def test_op_refuses_bad_arguments():
    import torch
    from m4depth_amd import network_ops as nops
    words = torch.zeros(4 + 4 * 64, dtype=torch.int64)
    state = nops.tsdf_state_views(words, 1, 6)
    f, c, pose = torch.ones((1, 2)), torch.ones((1, 2)), torch.zeros((1, 7), dtype=torch.float64)
    ok = dict(h=3, w=4, voxel=0.05, trunc=4, min_frames=1)

    def call(**kw):
        a = dict(ok, **kw)
        return nops.tsdf_render(state, a.pop("f", f), a.pop("c", c), a.pop("pose", pose), **a)

    for kw, match in ((dict(interp="cubic"), "interp must be one of nearest, trilinear"), (dict(interp=1), "interp must be one of"),
                      (dict(voxel=0.0), "voxel must be"), (dict(trunc=9), "trunc must be in 2..8"),
                      (dict(min_frames=0), "min_frames must be >= 1"), (dict(h=0), "need h, w >= 1"),
                      (dict(near=0.0), "need 0 < near < far"), (dict(voxel=1e-4), "more than 2\\^20 half voxels"),
                      (dict(window=2), "come together or not at all"), (dict(f=torch.ones((2, 2))), "cam_f / cam_c"),
                      (dict(hits=torch.zeros(2, dtype=torch.int64)), "hits: expected")):
        with pytest.raises(ValueError, match=match):
            call(**dict(dict(interp="trilinear"), **kw))
    with pytest.raises(ValueError, match="not a tsdf_state"):
        nops.tsdf_render(dict(state, b=2), f, c, pose, **ok)
    with pytest.raises(TypeError, match="out: expected a float32 device tensor"):      # no CPU path: refused before the library
        call(out=torch.zeros((1, 3, 4, 1)))
    assert nops.TSDF_INTERP == RR.INTERP


# ---- the host side of --fused_interp and --save_fused_view -------------------------------------------------------------------------
def _refused(argv, capsys, match):
    from m4depth_amd import main as MAIN
    with pytest.raises(SystemExit) as e:
        MAIN.main(argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def _checked(argv):
    from m4depth_amd import main as MAIN
    from m4depth_amd import options as O
    parser = MAIN.build_parser()
    args = parser.parse_args(argv)
    O.check_save_args(parser, args)
    O.check_fused_args(parser, args)
    return args


def test_driver_options(tmp_path, capsys):
    from m4depth_amd import main as MAIN
    out = str(tmp_path / "out")
    streams = ["--mode", "eval", "--dataset", "midair", "--eval_streams", "2"]
    predict = ["--mode", "predict", "--save_dir", out]
    _refused(streams + ["--fused_interp", "trilinear"], capsys, "--fused_interp needs --fused or --save_fused")
    _refused(streams + ["--fused_interp", "nearest"], capsys, "--fused_interp needs --fused or --save_fused")
    _refused(predict + ["--save_mesh", "0.1", "--fused_interp", "trilinear"], capsys, "--fused_interp needs --fused or --save_fused")
    _refused(streams + ["--fused", "0.1", "--fused_interp", "cubic"], capsys, "invalid choice")
    _refused(predict + ["--save_mesh", "0.1", "--save_fused_view"], capsys, "--save_fused_view needs --save_fused")
    _refused(streams + ["--fused", "0.1", "--save_fused_view"], capsys, "--save_fused_view needs --save_fused")
    assert not os.path.exists(out)
    a = _checked(streams + ["--fused", "0.1"])
    assert (a.fused_interp, a.save_fused_view) == ("nearest", False)
    a = _checked(streams + ["--fused", "0.1", "--fused_interp", "trilinear"])
    assert a.fused_interp == "trilinear"
    a = _checked(predict + ["--save_mesh", "0.1", "--save_fused", "--fused_interp", "trilinear", "--save_fused_view"])
    assert (a.fused_interp, a.save_fused, a.save_fused_view, a.fused) == ("trilinear", True, True, None)
    plain = vars(MAIN.build_parser().parse_args(["--mode", "predict"]))            # absent from the namespace until given
    assert not {"fused_interp", "save_fused_view"} & set(plain)


def test_writer_and_chain_keywords(tmp_path):
    from m4depth_amd.export import PredictionWriter
    from m4depth_amd.fusion import FusedDepth, TrajectoryChain
    out = str(tmp_path)
    with pytest.raises(ValueError, match="fused_interp needs save_fused"):
        PredictionWriter(out, "kitti16", save_mesh=0.1, fused_interp="trilinear")
    with pytest.raises(ValueError, match="save_fused_view needs save_fused"):
        PredictionWriter(out, "kitti16", save_mesh=0.1, save_fused_view=True)
    with pytest.raises(ValueError, match="fused_interp must be one of nearest, trilinear"):
        PredictionWriter(out, "kitti16", save_mesh=0.1, save_fused=True, fused_interp="cubic")
    w = PredictionWriter(out, "kitti16", save_mesh=0.1, save_fused=True, fused_interp="trilinear", save_fused_view=True)
    assert (w.fused_interp, w.save_fused_view, w.chain.interp) == ("trilinear", True, "trilinear")
    w.close()
    w = PredictionWriter(out, "kitti16", save_mesh=0.1, save_fused=True)
    assert (w.fused_interp, w.save_fused_view) == ("nearest", False)
    w.close()
    assert not os.listdir(out)
    with pytest.raises(ValueError, match="interp must be one of nearest, trilinear"):
        TrajectoryChain(0.1, interp="cubic")
    with pytest.raises(ValueError, match="--fused_interp must be one of"):
        FusedDepth(0.1, interp=1, names={"interp": "--fused_interp"})
    assert FusedDepth(0.1).interp == "nearest" and FusedDepth(0.1, interp="trilinear").interp == "trilinear"
