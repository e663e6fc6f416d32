"""The numpy restatement of m4d_depth_views (tests/depth_views_ref.py) on the scene the GPU tests use: what makes the cases
cases.  An analytic plane, 6 poses growing in translation and rotation, per-view depth rendered in float64 and rounded to
float32, three per-sample off-centre cameras, K = 4.  On clean maps the residuals of a tested view are the bilinear interpolation
error of a perspective plane (depth is not linear in the pixel; it grows with the focal ratio): their maxima per camera are
4.4e-5, 1.9e-4 and 4.7e-5 px and 1.1e-5, 7.7e-5 and 8.3e-6 relative, three to four orders of magnitude under 1 px / 1 %."""
import numpy as np
import pytest

import depth_views_ref as R
from helpers import F, cameras_np

B, K = 3, 4
CAM = cameras_np(B, R.H, R.W)
MAPS, POSES = R.scene(CAM)
for _a in (MAPS, POSES):
    _a.setflags(write=False)


def run(maps=MAPS, poses=POSES, cam=CAM, k_last=5, views=K, resets=None, **kw):
    """Frames 0..k_last through one state; the last frame's result and the state."""
    st = R.State(maps.shape[1], R.H, R.W, views)
    for k in range(k_last + 1):
        reset = None if resets is None else resets.get(k)
        out = st.step(maps[k], cam["f"], cam["c"], poses[k], force_all=(k == 0), reset=reset, **kw)
    return out, st


CLEAN, _ = run()


def test_clean_maps_are_confirmed_by_every_view_that_tests_them():
    tested = CLEAN["tested"].sum(0)
    assert np.array_equal(CLEAN["n_views"], tested)
    for s in range(B):
        hist = np.bincount(tested[s].ravel(), minlength=K + 1)
        print(f"sample {s}: tested-view histogram {hist}")
        assert (hist > 0).all(), "every count 0..K must occur"
    r_px = np.sqrt(np.nanmax(CLEAN["r_px2"], axis=(0, 2, 3)))
    r_rel = np.nanmax(CLEAN["r_z"] / CLEAN["zc"][None], axis=(0, 2, 3))
    print(f"largest residuals of a tested view per camera: {r_px} px, {r_rel} relative")
    assert (r_px < [5e-5, 2e-4, 5e-5]).all() and (r_rel < [1.2e-5, 8e-5, 9e-6]).all()   # the measured maxima, rounded up
    assert np.array_equal(CLEAN["age_out"], [K] * B)
    keep = CLEAN["n_views"] >= 2
    assert np.array_equal(CLEAN["depth_f"].view(np.uint32)[keep], MAPS[5].view(np.uint32)[keep])
    assert (CLEAN["depth_f"].view(np.uint32)[~keep] == 0x7FC00000).all() and (~keep).any() and keep.any()


def test_scaled_depth_is_rejected_everywhere():
    maps = MAPS.copy()
    maps[5] = (maps[5] * F(1.02)).astype(F)
    out, _ = run(maps)
    assert out["tested"].any() and (out["n_views"] == 0).all()


def test_scaled_block_gets_zero_and_the_rest_is_unchanged():
    maps = MAPS.copy()
    block = (slice(None), slice(10, 22), slice(15, 40))
    maps[5][block] = (maps[5][block] * F(1.2)).astype(F)
    out, _ = run(maps)
    assert (out["n_views"][block] == 0).all() and (CLEAN["n_views"][block] > 0).any()
    outside = np.ones(out["n_views"].shape, bool)
    outside[block] = False
    assert np.array_equal(out["n_views"][outside], CLEAN["n_views"][outside])


def test_a_wrong_patch_in_one_earlier_view_costs_exactly_that_view():
    maps = MAPS.copy()
    maps[3][:, 12:20, 20:32] = F(2.0)                                           # view j = 2 of frame 5
    out, _ = run(maps)
    diff = CLEAN["n_views"].astype(int) - out["n_views"].astype(int)
    assert set(np.unique(diff)) == {0, 1}
    lost = CLEAN["confirmed"][1] & ~out["confirmed"][1]
    assert np.array_equal(diff == 1, lost) and lost.sum() > 50
    for j in (0, 2, 3):
        assert np.array_equal(out["confirmed"][j], CLEAN["confirmed"][j])


@pytest.mark.parametrize("bad", [np.nan, np.inf, 0.0, -3.0])
def test_invalid_current_depths_get_zero(bad):
    maps = MAPS.copy()
    maps[5][:, 5:9, 7:19] = F(bad)
    out, _ = run(maps)
    assert (out["n_views"][:, 5:9, 7:19] == 0).all() and not out["tested"][:, :, 5:9, 7:19].any()
    assert (out["depth_f"].view(np.uint32)[:, 5:9, 7:19] == 0x7FC00000).all()
    mask = np.ones(out["n_views"].shape, bool)
    mask[:, 5:9, 7:19] = False
    assert np.array_equal(out["n_views"][mask], CLEAN["n_views"][mask])


def test_a_nan_tap_makes_the_view_not_test_the_pixel():
    maps = MAPS.copy()
    maps[4][:, 15, 25] = np.nan                                                 # view j = 1
    out, _ = run(maps)
    lost = CLEAN["tested"][0] & ~out["tested"][0]
    assert 1 <= lost.sum(axis=(1, 2)).min() and lost.sum(axis=(1, 2)).max() <= 9  # the pixels whose 2 x 2 taps hold (15, 25)
    assert not (out["tested"][0] & ~CLEAN["tested"][0]).any()
    assert np.array_equal(out["tested"][1:], CLEAN["tested"][1:])


def test_reset_sample_gets_zero_and_age_one():
    reset = np.array([0, 1, 0], np.uint8)
    out, _ = run(resets={5: reset})
    assert (out["n_views"][1] == 0).all() and not out["tested"][:, 1].any() and out["age_out"][1] == 1
    assert np.array_equal(out["n_views"][[0, 2]], CLEAN["n_views"][[0, 2]]) and list(out["age_out"][[0, 2]]) == [K, K]
    assert (out["depth_f"].view(np.uint32)[1] == 0x7FC00000).all()


def test_age_is_capped_and_head_wraps():
    cam = CAM
    maps, poses = R.scene(cam, n=K + 3, scale=0.6)
    st = R.State(B, R.H, R.W, K)
    heads, ages = [], []
    for k in range(K + 3):
        heads.append(st.head)
        out = st.step(maps[k], cam["f"], cam["c"], poses[k], force_all=(k == 0))
        ages.append(int(out["age_out"][0]))
        assert out["tested"].sum(0).max() == min(k, K)
        assert np.array_equal(st.ring_depth[heads[-1]], maps[k]) and np.array_equal(st.ring_pose[heads[-1]], poses[k])
    assert heads == [0, 1, 2, 3, 4, 0, 1] and ages == [1, 2, 3, 4, 4, 4, 4]
    # an age_in above K reads K views, not more
    out = R.depth_views(maps[-1], cam["f"], cam["c"], poses[-1], st.ring_depth.copy(), st.ring_pose.copy(), np.full(B, 99, np.int32),
                        st.head, K)
    assert list(out["age_out"]) == [K] * B and out["tested"].shape[0] == K


def test_nan_pose_confirms_nothing():
    poses = POSES.copy()
    poses[5, 2] = np.nan
    out, _ = run(poses=poses)
    assert (out["n_views"][2] == 0).all() and np.array_equal(out["n_views"][:2], CLEAN["n_views"][:2])
    poses = POSES.copy()
    poses[4, 0] = np.nan                                                        # an earlier view's pose
    out, _ = run(poses=poses)
    assert not out["tested"][0, 0].any() and np.array_equal(out["tested"][1:], CLEAN["tested"][1:])


def test_stationary_camera_confirms_every_valid_pixel():
    poses = np.ascontiguousarray(np.broadcast_to(POSES[2:3], POSES.shape))
    maps = np.ascontiguousarray(np.broadcast_to(MAPS[2:3], MAPS.shape))
    out, _ = run(maps, poses)
    # the reprojection of a border pixel may round to just outside the map (u = -1e-15): such a view does not test it
    assert (out["n_views"][:, 1:-1, 1:-1] == K).all() and np.array_equal(out["n_views"], out["tested"].sum(0))


# ---- a kernel reading the wrong thing must not pass ------------------------------------------------------------------------------
def test_wrong_reads_change_the_result():
    def differs(out):
        return not np.array_equal(out["n_views"], CLEAN["n_views"])
    swapped = {"f": np.stack([CAM["c"][:, 0], CAM["f"][:, 1]], 1), "c": np.stack([CAM["f"][:, 0], CAM["c"][:, 1]], 1)}
    assert differs(run(cam=swapped)[0]), "fx and cx swapped"
    other = {"f": np.roll(CAM["f"], 1, axis=0), "c": np.roll(CAM["c"], 1, axis=0)}
    assert differs(run(cam=other)[0]), "another sample's camera"
    st = R.State(B, R.H, R.W, K)
    for k in range(5):
        st.step(MAPS[k], CAM["f"], CAM["c"], POSES[k], force_all=(k == 0))
    ring_pose = np.roll(st.ring_pose, 1, axis=0)                                # every pose one slot off
    out = R.depth_views(MAPS[5], CAM["f"], CAM["c"], POSES[5], st.ring_depth.copy(), ring_pose, st.age, st.head, K)
    assert differs(out), "pose one slot off"
    ring_depth = np.roll(st.ring_depth, 1, axis=1)                              # another sample's ring map
    out = R.depth_views(MAPS[5], CAM["f"], CAM["c"], POSES[5], ring_depth, st.ring_pose.copy(), st.age, st.head, K)
    assert differs(out), "another sample's ring depth"
    inverse = POSES.copy()
    inverse[..., 1:4] *= -1                                                     # world-to-camera rotations
    assert differs(run(poses=inverse)[0]), "inverse rotation"
