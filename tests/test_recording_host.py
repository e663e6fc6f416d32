"""Host side of the recording front end (m4depth_amd/dataloaders/recording.py): parsing and refusals, pixel centre, output
camera, pose interpolation, trajectory breaks, frame selection, depth association, the motion convention, the loader's rows on
the CPU device, argument validation of the three entry points and the parser.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

from recording_ref import CAMERA_A, CAMERA_B, write_recording

F = np.float32


@pytest.fixture()
def R():
    from m4depth_amd.dataloaders import recording
    return recording


def _rewrite(path, fn):
    with open(path) as fh:
        text = fh.read()
    with open(path, "w") as fh:
        fh.write(fn(text))


def _set_camera(root, **changes):
    path = os.path.join(root, "camera.json")
    with open(path) as fh:
        cam = json.load(fh)
    for k, v in changes.items():
        if v is None:
            cam.pop(k, None)
        else:
            cam[k] = v
    with open(path, "w") as fh:
        json.dump(cam, fh)


# ---- parsing and refusals -----------------------------------------------------------------------------------------------------------
def test_read_recording_parses_the_four_files(R, tmp_path):
    root = str(tmp_path / "rec")
    stamps, times, poses = write_recording(root, CAMERA_A, 5, with_depth=True, extra={"T_body_cam": [2, 0, 0, 0, 0.1, 0.2, 0.3]})
    rec = R.read_recording(root)
    assert [t for t, _ in rec.frames] == pytest.approx(list(stamps)) and all(os.path.isabs(p) for _, p in rec.frames)
    assert rec.pose_times.shape == (6,) and rec.poses.shape == (6, 7)
    assert np.allclose(rec.poses, poses, atol=1e-12)                       # x y z w of the file -> w x y z
    assert len(rec.depth) == 5 and rec.camera["model"] == "radtan" and rec.camera["depth_scale"] == 5000.0
    assert np.array_equal(rec.camera["T_body_cam"], [1, 0, 0, 0, 0.1, 0.2, 0.3])     # normalised
    os.remove(os.path.join(root, "depth.txt"))
    assert R.read_recording(root).depth is None


@pytest.mark.parametrize("name", ["camera.json", "frames.txt", "poses.txt"])
def test_missing_file_is_refused(R, tmp_path, name):
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 3, with_depth=False)
    os.remove(os.path.join(root, name))
    with pytest.raises(ValueError, match=name.replace(".", r"\.") + ".*missing"):
        R.read_recording(root)


def test_unknown_model_and_wrong_distortion_length_are_refused(R, tmp_path):
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 3, with_depth=False)
    _set_camera(root, model="fov")
    with pytest.raises(ValueError, match=r"camera\.json.*unknown model 'fov'"):
        R.read_recording(root)
    _set_camera(root, model="radtan", distortion=[0.1, 0.2, 0.3, 0.4])
    with pytest.raises(ValueError, match=r"camera\.json.*5 distortion coefficients, got 4"):
        R.read_recording(root)
    _set_camera(root, model="equidistant", distortion=[0.1, 0.2, 0.3, 0.4, 0.5])
    with pytest.raises(ValueError, match=r"camera\.json.*4 distortion coefficients, got 5"):
        R.read_recording(root)
    _set_camera(root, model="pinhole", distortion=[0.1])
    with pytest.raises(ValueError, match=r"camera\.json.*0 distortion coefficients, got 1"):
        R.read_recording(root)
    _set_camera(root, model="pinhole", distortion=None)
    assert R.read_recording(root).camera["distortion"] == []


@pytest.mark.parametrize("name", ["frames.txt", "poses.txt", "depth.txt"])
def test_timestamps_must_strictly_increase(R, tmp_path, name):
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 4, with_depth=True)

    def repeat_third(text):                                       # line 1 is a comment in frames.txt / poses.txt
        lines = text.splitlines()
        first_data = 0 if name == "depth.txt" else 1
        lines[first_data + 2] = lines[first_data + 1]
        return "\n".join(lines) + "\n"
    _rewrite(os.path.join(root, name), repeat_third)
    line = 3 if name == "depth.txt" else 4
    with pytest.raises(ValueError, match=name.replace(".", r"\.") + f":{line}: timestamps must strictly increase"):
        R.read_recording(root)


@pytest.mark.parametrize("bad", ["0 0 0 0", "nan 0 0 1", "0 inf 0 1"])
def test_bad_quaternion_is_refused(R, tmp_path, bad):
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 3, with_depth=False)

    def spoil(text):
        lines = text.splitlines()
        f = lines[2].split()
        lines[2] = " ".join(f[:4]) + " " + bad
        return "\n".join(lines) + "\n"
    _rewrite(os.path.join(root, "poses.txt"), spoil)
    with pytest.raises(ValueError, match=r"poses\.txt:3: the quaternion is zero or not finite"):
        R.read_recording(root)


def test_image_size_is_checked_when_loaded(R, tmp_path):
    from PIL import Image
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 3, with_depth=True)
    loader = R.DataLoaderRecording()
    loader.recordings = [R.read_recording(root)]
    row = {"camera_l": os.path.join(root, "rgb", "0001.png"), "depth": os.path.join(root, "depth", "0001.png"), "rec": 0}
    raw = loader._load_raw(row)
    assert raw["rgb"].shape == (60, 94, 3) and raw["rgb"].dtype == np.uint8
    assert raw["depth"].shape == (60, 94) and raw["depth"].dtype == np.uint16 and raw["rec"] == 0
    Image.fromarray(np.zeros((60, 90, 3), np.uint8)).save(row["camera_l"])
    with pytest.raises(ValueError, match=r"0001\.png: the image is 60x90 .* camera\.json says 60x94"):
        loader._load_raw(row)


def test_paths_with_spaces_and_commas(R, tmp_path):
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 3, with_depth=False)
    os.rename(os.path.join(root, "rgb", "0001.png"), os.path.join(root, "rgb", "frame 1, left.png"))
    _rewrite(os.path.join(root, "frames.txt"), lambda text: text.replace("rgb/0001.png", "rgb/frame 1, left.png"))
    rec = R.read_recording(root)
    assert rec.frames[1][1] == os.path.join(root, "rgb", "frame 1, left.png") and os.path.isfile(rec.frames[1][1])


# ---- conventions ------------------------------------------------------------------------------------------------------------------
def test_pixel_centre_integer_shifts_the_principal_point(R, tmp_path):
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 3, with_depth=False)
    half = R.read_recording(root).camera
    assert (half["cx"], half["cy"]) == (45.964375, 31.109375)
    _set_camera(root, pixel_centre="integer")
    integer = R.read_recording(root).camera
    assert (integer["cx"], integer["cy"]) == (45.964375 + 0.5, 31.109375 + 0.5)
    _set_camera(root, pixel_centre=None)                           # the default is the OpenCV / Kalibr convention
    assert R.read_recording(root).camera["cx"] == 45.964375 + 0.5
    _set_camera(root, pixel_centre="centre")
    with pytest.raises(ValueError, match="pixel_centre"):
        R.read_recording(root)


def test_output_camera(R):
    cam = {"width": 94, "height": 60, "fx": 57.0, "fy": 56.0, "cx": 46.0, "cy": 31.0, "zoom": 1.0}
    # equal aspect: a plain scale by 1/2 about the corner (half-pixel convention: no offset)
    assert R.output_camera(cam, 30, 47) == pytest.approx((28.5, 28.0, 23.0, 15.5), abs=1e-12)
    # a crop: 60x94 -> 60x60 keeps the scale and cuts 17 columns on either side
    assert R.output_camera(cam, 60, 60) == pytest.approx((57.0, 56.0, 46.0 - 17.0, 31.0), abs=1e-12)
    # a crop and a scale: s = max(30/60, 20/94) = 0.5, visible source window 40 columns wide -> x0 = 27
    assert R.output_camera(cam, 30, 20) == pytest.approx((28.5, 28.0, (46.0 - 27.0) * 0.5, 15.5), abs=1e-12)
    # zoom 0.5 at the source's size: the image shrinks to half about its centre
    fx, fy, cx, cy = R.output_camera(dict(cam, zoom=0.5), 60, 94)
    assert (fx, fy) == pytest.approx((28.5, 28.0), abs=1e-12)
    assert (cx, cy) == pytest.approx((0.5 * 46.0 + 23.5, 0.5 * 31.0 + 15.0), abs=1e-12)
    # the image centre stays the image centre at any zoom
    for zoom in (0.6, 1.0, 1.7):
        c = dict(cam, cx=47.0, cy=30.0, zoom=zoom)
        assert R.output_camera(c, 40, 56)[2:] == pytest.approx((28.0, 20.0), abs=1e-12)


def _quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], axis * np.sin(angle / 2)])


def test_pose_interpolation(R):
    times = np.array([1.0, 2.0, 4.0])
    poses = np.array([np.concatenate([_quat([0, 0, 1], 0.0), [0, 0, 0]]),
                      np.concatenate([_quat([0, 0, 1], np.pi / 2), [2, 0, 4]]),
                      np.concatenate([-_quat([0, 0, 1], np.pi / 2 + 0.2), [2, 2, 4]])])
    for i in range(3):                                             # at a pose timestamp: that pose
        assert np.array_equal(R.interpolate_pose(times, poses, times[i]), poses[i])
    mid = R.interpolate_pose(times, poses, 1.5)                    # halfway through 90 degrees about z: 45 degrees
    assert np.allclose(mid[:4], _quat([0, 0, 1], np.pi / 4), atol=1e-15) and np.allclose(mid[4:], [1, 0, 2], atol=1e-15)
    # opposite signs: the short arc (0.2 rad), not the long way round (2 pi - 0.2)
    arc = R.interpolate_pose(times, poses, 3.0)
    want = _quat([0, 0, 1], np.pi / 2 + 0.1)
    assert min(np.abs(arc[:4] - want).max(), np.abs(arc[:4] + want).max()) < 1e-15 and np.allclose(arc[4:], [2, 1, 4])
    assert R.interpolate_pose(times, poses, 0.999) is None and R.interpolate_pose(times, poses, 4.001) is None
    assert R.interpolate_pose(times, poses, 3.0, max_gap=1.5) is None and R.interpolate_pose(times, poses, 1.5, max_gap=1.5) is not None


def _straight_recording(R, frame_times, pose_times, speed=1.0, depth=None):
    poses = np.array([[1, 0, 0, 0, 0, 0, speed * t] for t in pose_times], np.float64)
    cam = {"T_body_cam": np.array([1, 0, 0, 0, 0, 0, 0], np.float64)}
    return R.Recording("mem", cam, [(t, f"{t:.3f}.png") for t in frame_times], np.asarray(pose_times, np.float64), poses, depth)


def test_gap_splits_the_trajectory(R):
    pose_times = [0.0, 0.1, 0.2, 0.3, 1.3, 1.4, 1.5]              # a one-second hole in the trajectory file
    frames = [-0.05, 0.05, 0.15, 0.25, 0.5, 0.9, 1.35, 1.45, 1.6]
    trajs = R.select_frames(_straight_recording(R, frames, pose_times), max_gap=0.5)
    assert [[fr["t"] for fr in t] for t in trajs] == [[0.05, 0.15, 0.25], [1.35, 1.45]]
    assert np.allclose(trajs[1][0]["T_wc"], [1, 0, 0, 0, 0, 0, 1.35])
    # with a tolerance that spans the hole nothing splits; only the frames outside the span are dropped
    assert [len(t) for t in R.select_frames(_straight_recording(R, frames, pose_times), max_gap=2.0)] == [7]


def test_stride_and_min_baseline(R):
    pose_times = np.arange(0.0, 2.01, 0.1)
    frames = list(np.round(np.arange(0.05, 1.96, 0.1), 3))         # 20 frames, 0.1 m apart at 1 m/s
    rec = _straight_recording(R, frames, pose_times)
    ts = lambda trajs: [round(fr["t"], 3) for fr in trajs[0]]
    assert ts(R.select_frames(rec, stride=1)) == frames
    assert ts(R.select_frames(rec, stride=3)) == frames[::3]
    assert ts(R.select_frames(rec, min_baseline=0.25)) == frames[::3]           # 0.3 m is the first step >= 0.25 m
    assert ts(R.select_frames(rec, stride=2, min_baseline=0.5)) == frames[::6]   # of every 2nd frame (0.2 m) every 3rd
    assert ts(R.select_frames(rec, min_baseline=100.0)) == frames[:1]            # a trajectory's first frame is always kept
    with pytest.raises(ValueError, match="rec_stride"):
        R.select_frames(rec, stride=0)


def test_depth_association(R):
    frames = [1.0, 1.1, 1.2, 1.3]
    depth = [(1.015, "a"), (1.125, "b"), (1.21, "c"), (1.22, "d"), (1.281, "e")]
    # a: 0.015 s from frame 0 -> attached; b: 0.025 s from frame 1 -> beyond 0.02; c beats d at frame 2; e: 0.019 s from frame 3
    assert R.associate_depth(frames, depth) == ["a", None, "c", "e"]
    assert R.associate_depth(frames, None) == [None] * 4
    rec = _straight_recording(R, frames, [0.0, 2.0], depth=depth)
    assert [fr["depth"] for fr in R.select_frames(rec, max_gap=5.0)[0]] == ["a", None, "c", "e"]


def test_scoring_leaves_out_frames_without_a_depth_file(R, tmp_path, capsys):
    """A depth.txt that misses one frame (every real TUM sequence has some): the scoring use cases, and predict with
    ground-truth panels, leave the frame out -- every remaining row names a map and the motion spans the hole -- while a
    plain predict run keeps it."""
    from m4depth_amd import dataloaders as dl
    from m4depth_amd import main as M
    root = str(tmp_path / "rec")
    write_recording(root, CAMERA_A, 8, with_depth=True)
    _rewrite(os.path.join(root, "depth.txt"), lambda text: "\n".join(l for l in text.splitlines() if "0003.png" not in l) + "\n")
    settings = dl.DataloaderParameters(None, root, None, None, False)
    loader = dl.get_loader("recording")
    loader.get_dataset("predict", settings, batch_size=1, out_size=[64, 64], device="cpu")
    full = loader._get_trajectories()[0]
    assert len(full) == 8 and [bool(r["depth"]) for r in full] == [True] * 3 + [False] + [True] * 4
    for usecase in ("eval", "eval_streams", "train"):
        loader = dl.get_loader("recording")
        loader.get_dataset(usecase, dl.DataloaderParameters(None, root, 4 if usecase == "train" else None,
                                                             4 if usecase == "train" else None, False),
                           batch_size=1, out_size=[64, 64], device="cpu")
        assert "1 of 8 frames have no depth file" in capsys.readouterr().out
        rows = loader._get_trajectories()[0]
        assert [os.path.basename(r["camera_l"]) for r in rows] == [f"{i:04d}.png" for i in (0, 1, 2, 4, 5, 6, 7)]
        assert all(r["depth"] for r in rows) and [r["id"] for r in rows] == list(range(7))
        # the motion across the hole is the composition of the two motions it replaces
        a, b = (np.array([full[i][k] for k in ("qw", "qx", "qy", "qz", "tx", "ty", "tz")]) for i in (3, 4))
        want = R.compose(a, b)
        got = np.array([rows[3][k] for k in ("qw", "qx", "qy", "qz", "tx", "ty", "tz")])
        assert np.abs(got - want).max() < 1e-6
    args = M.build_parser().parse_args(["--mode", "predict", "--dataset", "recording", "--records_path", root, "--height", "64",
                                        "--width", "64", "--save_dir", str(tmp_path / "o"), "--save_panels", "rgb,err"])
    loader = M.recording_loader(args)
    assert loader.require_depth
    loader.get_dataset("predict", settings, batch_size=1, out_size=[64, 64], device="cpu")
    assert len(loader._get_trajectories()[0]) == 7
    args.save_panels = None
    assert not M.recording_loader(args).require_depth


def _pose_step(pose, rot, trans):
    """The rule stated at m4d_pose_accumulate, in float64."""
    from m4depth_amd.dataloaders import recording as R
    q = rot.astype(np.float64)
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    t = R.quat_rot(pose[:4]) @ trans.astype(np.float64) + pose[4:]
    qw = R.quat_mul(pose[:4], q)
    return np.concatenate([qw / np.linalg.norm(qw), t])


def test_relative_motions_closed_loop(R):
    """12 random poses with unit-scale motion and a non-trivial T_body_cam: the float32 motions, chained in float64 with the
    rule of m4d_pose_accumulate, reproduce T_wc[0]^-1 T_wc[t].  Bound: 7 float32 roundings of about 2^-24 relative per step
    over 12 steps of motion of order 1 -> 1e-5 m and 1e-6 per quaternion component."""
    rng = np.random.default_rng(5)
    T_bc = np.concatenate([_quat([1, -2, 0.5], 1.1), [0.1, -0.05, 0.2]])
    T_wb = np.array([np.concatenate([_quat(rng.normal(size=3), rng.uniform(0, 2 * np.pi)) * rng.choice([-1, 1]),
                                     rng.normal(0, 1.0, 3)]) for _ in range(12)])
    T_wc = R.compose(T_wb, T_bc)
    assert np.allclose(T_wc[3, 4:], R.quat_rot(T_wb[3, :4]) @ T_bc[4:] + T_wb[3, 4:])
    m = R.relative_motions(T_wc)
    assert m.dtype == np.float32 and m.shape == (12, 7) and np.array_equal(m[0], [1, 0, 0, 0, 0, 0, 0])
    assert (m[:, 0] >= 0).all() and np.abs(np.linalg.norm(m[:, :4].astype(np.float64), axis=1) - 1).max() < 1e-7
    pose = np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
    inv0_q = R.quat_conj(T_wc[0, :4])
    worst_t = worst_q = 0.0
    for t in range(1, 12):
        pose = _pose_step(pose, m[t, :4], m[t, 4:])
        want_q = R.quat_mul(inv0_q, T_wc[t, :4])
        want_t = R.quat_rot(T_wc[0, :4]).T @ (T_wc[t, 4:] - T_wc[0, 4:])
        worst_t = max(worst_t, np.abs(pose[4:] - want_t).max())
        worst_q = max(worst_q, min(np.abs(pose[:4] - want_q).max(), np.abs(pose[:4] + want_q).max()))
    print(f"closed loop over 12 poses: translation {worst_t:.3e} m, quaternion {worst_q:.3e}")
    assert worst_t <= 1e-5 and worst_q <= 1e-6
    # the direction: a camera that moves forward (+z in the world = +z of the first camera) has t = +step in the PREVIOUS camera
    fwd = R.relative_motions(np.array([[1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0.5]], np.float64))
    assert np.array_equal(fwd[1], [1, 0, 0, 0, 0, 0, 0.5])


# ---- the loader on the CPU device -------------------------------------------------------------------------------------------------
def test_loader_rows_cameras_and_new_traj_on_cpu(R, tmp_path):
    from m4depth_amd import dataloaders as dl
    root = str(tmp_path / "recs")
    write_recording(os.path.join(root, "a"), CAMERA_A, 8, with_depth=True, extra={"zoom": 0.9})
    write_recording(os.path.join(root, "b"), CAMERA_B, 6, with_depth=False)
    os.makedirs(os.path.join(root, "not_a_recording"))
    loader = dl.get_loader("recording")
    assert isinstance(loader, R.DataLoaderRecording) and loader.depth_type == "map"
    assert not loader.has_depth(root) and loader.has_depth(os.path.join(root, "a"))
    settings = dl.DataloaderParameters(None, root, None, None, False)
    with pytest.raises(ValueError, match="out_size"):
        loader.get_dataset("predict", settings, device="cpu")
    ds = loader.get_dataset("predict", settings, batch_size=1, out_size=[64, 64], device="cpu")
    assert ds.cardinality() == 14 and [r.root for r in loader.recordings] == [os.path.join(root, "a"), os.path.join(root, "b")]
    trajs = loader._get_trajectories()
    assert [len(t) for t in trajs] == [8, 6]
    for ri, traj in enumerate(trajs):
        assert [r["id"] for r in traj] == list(range(len(traj))) and all(r["rec"] == ri for r in traj)
        assert all(os.path.isfile(r["camera_l"]) for r in traj)
        assert all(bool(r["depth"]) == (ri == 0) for r in traj)
        assert [traj[0][k] for k in ("qw", "qx", "qy", "qz", "tx", "ty", "tz")] == [1, 0, 0, 0, 0, 0, 0]
        assert traj[1]["tz"] == pytest.approx(0.3, abs=0.02) and traj[1]["qw"] > 0.999
    want = R.output_camera(loader.recordings[0].camera, 64, 64)
    (fx, fy), (cx, cy) = loader._camera(trajs[0][3])
    assert (fx, fy, cx, cy) == tuple(float(F(v)) for v in want)
    s = 64 / 60 * 0.9
    assert want == pytest.approx((CAMERA_A["fx"] * s, CAMERA_A["fy"] * s, (CAMERA_A["cx"] - 47) * s + 32,
                                  (CAMERA_A["cy"] - 30) * s + 32), abs=1e-9)
    assert loader._camera(trajs[1][0]) == ((float(F(CAMERA_B["fx"])), float(F(CAMERA_B["fy"]))),
                                           (float(F(CAMERA_B["cx"])), float(F(CAMERA_B["cy"]))))
    pose = loader._pose(trajs[0][0])
    assert pose["new_traj"] is True and loader._pose(trajs[0][1])["new_traj"] is False
    assert pose["camera"]["f"].tolist() == [fx, fy]
    # the options of the driver: a stride, and a gap tolerance below the pose spacing (0.1 s) that drops every frame
    loader.stride = 3
    assert [len(t) for t in loader._get_trajectories()] == [3, 2]
    loader.stride, loader.max_gap = 1, 0.05
    with pytest.raises(ValueError, match="no frame of any recording"):
        loader._get_trajectories()
    # a use case that scores against ground truth refuses the recording without depth.txt
    loader.max_gap = 0.5
    for usecase in ("eval", "eval_streams"):
        with pytest.raises(ValueError, match=r"b: no depth\.txt"):
            loader.get_dataset(usecase, settings, batch_size=2, out_size=[64, 64], device="cpu")
    with pytest.raises(ValueError, match="neither a recording"):
        R.find_recordings(os.path.join(root, "not_a_recording"))


# ---- the library without a GPU ------------------------------------------------------------------------------------------------------
def test_argument_validation_of_the_remap_entry_points_without_gpu():
    from m4depth_amd._lib import lib
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)      # never dereferenced: validation fails first
    f4 = (ctypes.c_float * 4)(50.0, 50.0, 32.0, 32.0)
    d5 = (ctypes.c_float * 5)(0.1, 0.0, 0.0, 0.0, 0.0)
    assert lib.m4d_undistort_map(1, d5, f4, f4, 60, 94, 40, 56, None, None) == 1            # NULL map
    assert lib.m4d_undistort_map(1, None, f4, f4, 60, 94, 40, 56, fake, None) == 1          # NULL coefficients of a lens model
    assert lib.m4d_undistort_map(1, d5, None, f4, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_undistort_map(1, d5, f4, None, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_undistort_map(1, d5, f4, f4, 60, 94, 0, 56, fake, None) == 1             # a zero size
    assert lib.m4d_undistort_map(1, d5, f4, f4, 60, -1, 40, 56, fake, None) == 1
    assert lib.m4d_undistort_map(3, d5, f4, f4, 60, 94, 40, 56, fake, None) == 1            # unknown model
    assert lib.m4d_undistort_map(-1, d5, f4, f4, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_undistort_map(1, d5, f4, f4, 60, 94, 40, 56, odd, None) == 1             # map off 8 bytes
    assert lib.m4d_decode_rgb8_remap(None, fake, 1, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_rgb8_remap(fake, None, 1, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_rgb8_remap(fake, fake, 1, 60, 94, 40, 56, None, None) == 1
    assert lib.m4d_decode_rgb8_remap(fake, fake, 0, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_rgb8_remap(fake, fake, 1, 60, 94, 40, 0, fake, None) == 1
    assert lib.m4d_decode_rgb8_remap(fake, odd, 1, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_depth16_remap(None, fake, 0.0002, 1, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_depth16_remap(fake, None, 0.0002, 1, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_depth16_remap(fake, fake, 0.0002, 1, 60, 94, 40, 56, None, None) == 1
    assert lib.m4d_decode_depth16_remap(fake, fake, 0.0002, 1, 0, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_depth16_remap(ctypes.c_void_p(4097), fake, 0.0002, 1, 60, 94, 40, 56, fake, None) == 1
    assert lib.m4d_decode_depth16_remap(fake, fake, 0.0002, 1, 60, 94, 40, 56, ctypes.c_void_p(4098), None) == 1


# ---- the parser -------------------------------------------------------------------------------------------------------------------
def _parse(argv):
    from m4depth_amd import main as M
    parser = M.build_parser()
    args = parser.parse_args(argv)
    M.check_recording_args(parser, args)
    return args


def test_parser(tmp_path, capsys):
    write_recording(str(tmp_path / "r"), CAMERA_A, 2, with_depth=False)
    rec = ["--dataset", "recording", "--records_path", str(tmp_path / "r"), "--arch_depth", "2"]
    a = _parse(rec + ["--height", "64", "--width", "72", "--rec_stride", "3", "--rec_min_baseline", "0.1", "--rec_max_gap", "1"])
    assert (a.rec_stride, a.rec_min_baseline, a.rec_max_gap) == (3, 0.1, 1.0)
    from m4depth_amd import main as M
    loader = M.recording_loader(a)
    assert (loader.stride, loader.min_baseline, loader.max_gap) == (3, 0.1, 1.0)
    loader = M.recording_loader(_parse(rec + ["--height", "64", "--width", "64"]))
    assert (loader.stride, loader.min_baseline, loader.max_gap) == (1, 0.0, 0.5)
    for bad, message in ((rec, "needs --height and --width"),
                         (rec + ["--height", "64"], "needs --height and --width"),
                         (rec + ["--height", "64", "--width", "70"], "multiples of 2\\*\\*arch_depth = 4"),
                         (rec + ["--height", "64", "--width", "64", "--rec_stride", "0"], "--rec_stride must be >= 1"),
                         (["--dataset", "recording", "--records_path", str(tmp_path / "nowhere"), "--height", "64", "--width", "64",
                           "--arch_depth", "2"], "--records_path .*nowhere: neither a recording"),
                         (["--dataset", "midair", "--rec_stride", "2"], "--rec_stride is a --dataset=recording option"),
                         (["--rec_min_baseline", "0.1"], "--rec_min_baseline is a --dataset=recording option"),
                         (["--dataset", "kitti-raw", "--rec_max_gap", "1"], "--rec_max_gap is a --dataset=recording option")):
        with pytest.raises(SystemExit):
            _parse(bad)
        import re
        assert re.search(message, capsys.readouterr().err), bad


def test_save_panels_ask_the_loader_for_ground_truth(tmp_path, capsys):
    from m4depth_amd import main as M
    write_recording(str(tmp_path / "a"), CAMERA_A, 3, with_depth=True)
    write_recording(str(tmp_path / "b"), CAMERA_B, 3, with_depth=False)
    base = ["--mode", "predict", "--dataset", "recording", "--height", "64", "--width", "64", "--arch_depth", "2", "--save_dir",
            str(tmp_path / "out"), "--save_panels", "rgb,gt,err"]
    parser = M.build_parser()
    args = parser.parse_args(base + ["--records_path", str(tmp_path / "a")])
    M.check_save_args(parser, args)
    assert args.save_panels == ("rgb", "gt", "err") and M.records_have_depth(args)
    for path in (tmp_path / "b", tmp_path):
        args = parser.parse_args(base + ["--records_path", str(path)])
        with pytest.raises(SystemExit):
            M.check_save_args(parser, args)
        assert "name no ground-truth map" in capsys.readouterr().err


def test_bench_tool_restates_the_equidistant_table_like_the_reference(R):
    """tools/bench_recording_decode.py stands alone and carries its own copy of the equidistant formula: it must be the
    restatement's, bit for bit, in both precisions, on the fixture it reports on."""
    import importlib.util
    from recording_ref import undistort_map
    spec = importlib.util.spec_from_file_location(
        "bench_recording_decode", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                               "bench_recording_decode.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = tuple(CAMERA_B[k] for k in ("fx", "fy", "cx", "cy"))
    out_cam = R.output_camera(dict(CAMERA_B, zoom=1.0), 40, 56)
    for T in (np.float32, np.float64):
        ref = undistort_map("equidistant", CAMERA_B["distortion"], src, out_cam, 64, 64, 40, 56, T)
        assert (ref[..., 0] >= -0.5).all()                          # a source everywhere: the tool's copy has no validity test
        got = tool.equidistant_table(CAMERA_B["distortion"], src, out_cam, 40, 56, T)
        assert got.dtype == ref.dtype and np.array_equal(got, ref)
