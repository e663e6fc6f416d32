"""Host side of the point-cloud export: the PLY writer and reader, argument validation of m4d_pose_accumulate and
m4d_depth_cloud without a device, the workspace helper, the driver's refusals and the header's declarations."""
import ctypes
import os

import numpy as np
import pytest

F = np.float32


# ---- PLY ---------------------------------------------------------------------------------------------------------------------
def _vertices(n, seed=0):
    from m4depth_amd.export import PLY_VERTEX
    rng = np.random.default_rng(seed)
    v = np.zeros(n, PLY_VERTEX)
    for k in ("x", "y", "z"):
        v[k] = rng.normal(0, 30, n).astype(F)
    for k in ("red", "green", "blue"):
        v[k] = rng.integers(0, 256, n)
    v["alpha"] = 255
    return v


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_ply_round_trip(tmp_path, n):
    from m4depth_amd.export import write_cloud_ply, read_cloud_ply, PLY_VERTEX
    assert PLY_VERTEX.itemsize == 16
    v = _vertices(n)
    pose = np.array([0.1234567890123456789, -1 / 3, 2 ** -40, np.sqrt(0.5), 1e9 + 0.125, -5e-324, 12.5])
    path = str(tmp_path / "c.ply")
    write_cloud_ply(path, v.view(np.uint8).reshape(n, 16), pose)
    raw = open(path, "rb").read()
    head, body = raw[:raw.index(b"end_header\n") + len(b"end_header\n")], raw[raw.index(b"end_header\n") + len(b"end_header\n"):]
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and f"element vertex {n}" in lines
    assert lines[2].startswith("comment pose ") and len(lines[2].split()) == 9
    assert [l for l in lines if l.startswith("property")] == [
        "property float x", "property float y", "property float z", "property uchar red", "property uchar green",
        "property uchar blue", "property uchar alpha"]
    assert body == v.tobytes()                                                  # verbatim
    xyz, rgba, got_pose = read_cloud_ply(path)
    assert xyz.dtype == np.float32 and xyz.shape == (n, 3) and rgba.dtype == np.uint8 and rgba.shape == (n, 4)
    assert np.array_equal(xyz.view(np.uint32), np.stack([v["x"], v["y"], v["z"]], 1).view(np.uint32).reshape(n, 3))
    assert np.array_equal(rgba, np.stack([v["red"], v["green"], v["blue"], v["alpha"]], 1).reshape(n, 4))
    assert got_pose.dtype == np.float64 and np.array_equal(got_pose, pose)      # %.17g round-trips a double


def test_ply_reader_refuses_other_files(tmp_path):
    from m4depth_amd.export import write_cloud_ply, read_cloud_ply
    path = str(tmp_path / "c.ply")
    write_cloud_ply(path, _vertices(5).view(np.uint8).reshape(5, 16), np.arange(7.0))
    raw = open(path, "rb").read()
    for name, data in (("short", raw[:-3]), ("ascii", raw.replace(b"binary_little_endian", b"ascii")),
                       ("nopose", raw.replace(b"comment pose", b"comment nose")), ("empty", b""),
                       ("noalpha", raw.replace(b"property uchar alpha\n", b""))):
        bad = str(tmp_path / (name + ".ply"))
        open(bad, "wb").write(data)
        with pytest.raises(ValueError):
            read_cloud_ply(bad)


# ---- argument validation, no device --------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)                 # never dereferenced: validation fails first


def _cloud(**over):
    from m4depth_amd._lib import lib
    a = dict(depth=FAKE, depth_stride=12, rgb=FAKE, rgb_stride=36, cam_f=FAKE, cam_c=FAKE, pose=FAKE, b=2, h=3, w=4, step=1,
             near=1.0, far=80.0, vertices=FAKE, counts=FAKE, workspace=FAKE)
    a.update(over)
    return lib.m4d_depth_cloud(a["depth"], a["depth_stride"], a["rgb"], a["rgb_stride"], a["cam_f"], a["cam_c"], a["pose"],
                               a["b"], a["h"], a["w"], a["step"], a["near"], a["far"], a["vertices"], a["counts"],
                               a["workspace"], None)


CLOUD_REFUSED = {
    "null depth": dict(depth=None), "null rgb": dict(rgb=None), "null cam_f": dict(cam_f=None), "null cam_c": dict(cam_c=None),
    "null vertices": dict(vertices=None), "null counts": dict(counts=None), "null workspace": dict(workspace=None),
    "empty batch": dict(b=0), "negative batch": dict(b=-1), "batch above the grid": dict(b=65536),
    "no rows": dict(h=0), "no columns": dict(w=0), "step zero": dict(step=0), "step negative": dict(step=-2),
    "far equals near": dict(far=1.0), "far below near": dict(near=10.0, far=5.0), "nan far": dict(far=float("nan")),
    "nan near": dict(near=float("nan")), "depth stride": dict(depth_stride=11), "rgb stride": dict(rgb_stride=35),
    "misaligned depth": dict(depth=ctypes.c_void_p(4098)), "misaligned rgb": dict(rgb=ctypes.c_void_p(4097)),
    "misaligned pose": dict(pose=ctypes.c_void_p(4100)), "misaligned vertices": dict(vertices=ctypes.c_void_p(4104)),
    "misaligned counts": dict(counts=ctypes.c_void_p(4098)), "misaligned workspace": dict(workspace=ctypes.c_void_p(4097)),
}


@pytest.mark.parametrize("why", sorted(CLOUD_REFUSED))
def test_depth_cloud_refuses_without_a_device(why):
    assert _cloud(**CLOUD_REFUSED[why]) == 1, why


def _pose(**over):
    from m4depth_amd._lib import lib
    a = dict(reset=FAKE, force_all=0, rot=FAKE, trans=FAKE, b=2, pose=FAKE)
    a.update(over)
    return lib.m4d_pose_accumulate(a["reset"], a["force_all"], a["rot"], a["trans"], a["b"], a["pose"], None)


POSE_REFUSED = {
    "null rot": dict(rot=None), "null trans": dict(trans=None), "null pose": dict(pose=None), "empty batch": dict(b=0),
    "negative batch": dict(b=-3), "misaligned rot": dict(rot=ctypes.c_void_p(4098)),
    "misaligned trans": dict(trans=ctypes.c_void_p(4097)), "misaligned pose": dict(pose=ctypes.c_void_p(4100)),
}


@pytest.mark.parametrize("why", sorted(POSE_REFUSED))
def test_pose_accumulate_refuses_without_a_device(why):
    assert _pose(**POSE_REFUSED[why]) == 1, why


def test_refusals_launch_nothing():
    from m4depth_amd._lib import lib
    n0 = lib.m4d_launch_count()
    assert _cloud(step=0) == 1 and _pose(b=0) == 1
    assert lib.m4d_launch_count() == n0


def test_cloud_workspace_and_capacity():
    """One int per workgroup of 256 candidates and sample; a refused geometry needs none."""
    from m4depth_amd._lib import lib
    from m4depth_amd.network_ops import cloud_capacity
    for b, h, w, step in ((1, 1, 1, 1), (3, 37, 53, 1), (3, 37, 53, 2), (3, 37, 53, 3), (8, 384, 384, 1), (2, 384, 1280, 5)):
        cap = -(-h // step) * -(-w // step)
        assert cloud_capacity(h, w, step) == cap
        assert lib.m4d_depth_cloud_workspace_ints(b, h, w, step) == b * -(-cap // 256), (b, h, w, step)
    assert lib.m4d_depth_cloud_workspace_ints(0, 4, 4, 1) == 0 and lib.m4d_depth_cloud_workspace_ints(1, 4, 4, 0) == 0
    # the write pass's prefix is quadratic in cap: 2^24 candidates per sample is the most the entry point takes
    assert lib.m4d_depth_cloud_workspace_ints(1, 4096, 4096, 1) == 65536 and lib.m4d_depth_cloud_workspace_ints(1, 4097, 4096, 1) == 0
    assert lib.m4d_depth_cloud_workspace_ints(1, 8192, 8192, 2) == 65536 and _cloud(h=4097, w=4096) == 1


def test_wrappers_refuse_before_any_pointer_is_taken():
    import torch
    from m4depth_amd import network_ops as nops
    pose = torch.zeros((2, 7), dtype=torch.float64)
    with pytest.raises(ValueError, match="small-angle"):
        nops.pose_accumulate(torch.zeros(2, 3), torch.zeros(2, 3), pose)
    with pytest.raises(ValueError, match="float64"):
        nops.pose_accumulate(torch.zeros(2, 4), torch.zeros(2, 3), pose.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nops.pose_accumulate(torch.zeros(2, 4), torch.zeros(2, 3), pose)
    with pytest.raises(ValueError, match="step"):
        nops.depth_cloud(torch.zeros(2, 3, 4, 1), torch.zeros(2, 3, 4, 3), torch.ones(2, 2), torch.ones(2, 2), step=0)
    with pytest.raises(ValueError, match="near < far"):
        nops.depth_cloud(torch.zeros(2, 3, 4, 1), torch.zeros(2, 3, 4, 3), torch.ones(2, 2), torch.ones(2, 2), near=5, far=5)
    with pytest.raises(TypeError, match="float32 device tensor"):
        nops.depth_cloud(torch.zeros(2, 3, 4, 1), torch.zeros(2, 3, 4, 3), torch.ones(2, 2), torch.ones(2, 2))


def test_writer_refuses_bad_cloud_options(tmp_path):
    from m4depth_amd.export import PredictionWriter
    with pytest.raises(ValueError, match="cloud_step"):
        PredictionWriter(str(tmp_path), "kitti16", cloud=True, cloud_step=0)
    with pytest.raises(ValueError, match="cloud_frame"):
        PredictionWriter(str(tmp_path), "kitti16", cloud=True, cloud_frame="body")
    w = PredictionWriter(str(tmp_path), "kitti16")
    assert (w.cloud, w.cloud_step, w.cloud_frame) == (False, 2, "world")
    w.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _refused(argv, capsys, match):
    from m4depth_amd import main as MAIN
    with pytest.raises(SystemExit) as e:
        MAIN.main(argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def test_driver_refusals(tmp_path, capsys):
    out = str(tmp_path / "out")
    _refused(["--mode", "predict", "--save_cloud"], capsys, "--save_cloud needs --save_dir")
    _refused(["--mode", "predict", "--cloud_stride", "3"], capsys, "--cloud_stride needs --save_dir")
    _refused(["--mode", "predict", "--cloud_frame", "camera"], capsys, "--cloud_frame needs --save_dir")
    _refused(["--mode", "predict", "--save_dir", out, "--save_cloud", "--cloud_stride", "0"], capsys, "--cloud_stride must be >= 1")
    _refused(["--mode", "predict", "--save_dir", out, "--save_cloud", "--cloud_stride", "-2"], capsys, "--cloud_stride must be >= 1")
    _refused(["--mode", "predict", "--save_dir", out, "--cloud_stride", "2"], capsys, "--cloud_stride needs --save_cloud")
    _refused(["--mode", "predict", "--save_dir", out, "--save_cloud", "--cloud_frame", "body"], capsys, "invalid choice")
    _refused(["--mode", "eval", "--save_dir", out, "--save_cloud"], capsys, "--save_dir is a --mode=predict option")
    assert not os.path.exists(out)


def test_driver_defaults():
    from m4depth_amd import main as MAIN
    parser = MAIN.build_parser()
    args = parser.parse_args(["--mode", "predict", "--save_dir", "x", "--save_cloud"])
    MAIN.check_save_args(parser, args)
    assert args.save_cloud and args.cloud_stride == 2 and args.cloud_frame == "world" and args.save_range == (1.0, 80.0)
    args = parser.parse_args(["--mode", "predict", "--save_dir", "x"])
    MAIN.check_save_args(parser, args)
    assert not args.save_cloud


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "m4depth_hip.h")).read()
    for decl in ("int m4d_pose_accumulate(", "int m4d_depth_cloud(", "long long m4d_depth_cloud_workspace_ints("):
        assert decl in txt, decl
    assert "get_rot_mat" in txt[txt.index("One camera-to-world pose"):txt.index("int m4d_pose_accumulate(")]
    assert "#define M4D_ABI_VERSION 6 " in txt
