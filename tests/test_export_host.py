"""Host side of the prediction export: argument validation of m4d_depth_export without a device, the colour table, the frame
namer, the PNG reader and the driver's refusals."""
import ctypes
import os

import numpy as np
import pytest

F = np.float32


def _export_args(**over):
    """A call of m4d_depth_export that passes validation (pointers are never dereferenced on the host), with overrides."""
    fake = ctypes.c_void_p(4096)
    a = dict(est=fake, est_stride=12, gt=fake, gt_stride=12, rgb=fake, rgb_stride=36, b=2, h=3, w=4, format=1, depth16=fake,
             kinds=(0, 1, 2, 3), lut=fake, near=1.0, far=80.0, err_max=0.5, panels=fake)
    a.update(over)
    return a


def _export(a, n_panels=None):
    from m4depth_amd._lib import lib
    kinds = (ctypes.c_int * 8)(*a["kinds"]) if a["kinds"] is not None else None
    n = len(a["kinds"] or ()) if n_panels is None else n_panels
    return lib.m4d_depth_export(a["est"], a["est_stride"], a["gt"], a["gt_stride"], a["rgb"], a["rgb_stride"], a["b"], a["h"],
                                a["w"], a["format"], a["depth16"], n, kinds, a["lut"], a["near"], a["far"], a["err_max"],
                                a["panels"], None)


REFUSED = {
    "null est": dict(est=None),
    "format below": dict(format=-1),
    "format above": dict(format=3),
    "no depth16 for a format": dict(depth16=None),
    "nothing asked for": dict(format=0, kinds=()),
    "gt panel without gt": dict(gt=None, kinds=(2,)),
    "err panel without gt": dict(gt=None, kinds=(3,)),
    "rgb panel without rgb": dict(rgb=None, kinds=(0,)),
    "est panel without lut": dict(lut=None, kinds=(1,)),
    "panels without a destination": dict(panels=None),
    "five panels": dict(kinds=(0, 1, 2, 3, 1)),
    "unknown kind": dict(kinds=(1, 4)),
    "negative kind": dict(kinds=(-1,)),
    "near zero": dict(near=0.0),
    "near negative": dict(near=-1.0),
    "far equals near": dict(far=1.0),
    "far below near": dict(near=10.0, far=5.0),
    "err_max zero": dict(err_max=0.0),
    "nan range": dict(far=float("nan")),
    "est stride": dict(est_stride=11),
    "gt stride": dict(gt_stride=11),
    "rgb stride": dict(rgb_stride=35),
    "misaligned est": dict(est=ctypes.c_void_p(4098)),
    "misaligned gt": dict(gt=ctypes.c_void_p(4097)),
    "misaligned rgb": dict(rgb=ctypes.c_void_p(4102)),
    "misaligned depth16": dict(depth16=ctypes.c_void_p(4097)),
    "empty batch": dict(b=0),
    "empty rows": dict(w=0),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_depth_export_refuses_without_a_device(why):
    assert _export(_export_args(**REFUSED[why])) == 1, why


def test_depth_export_refuses_a_missing_kind_list():
    assert _export(_export_args(kinds=None), n_panels=2) == 1


def test_default_lut():
    from m4depth_amd.export import default_lut
    lut = default_lut()
    assert lut.shape == (257, 3) and lut.dtype == np.uint8
    assert np.array_equal(lut, default_lut())
    assert tuple(lut[256]) == (0, 0, 0) and not (lut[:256] == lut[256]).all(axis=1).any()      # invalid is told apart
    assert len(np.unique(lut[:256], axis=0)) == 256
    assert np.abs(np.diff(lut[:256].astype(int), axis=0)).max() <= 4                             # no jumps: interpolated


def test_frame_namer():
    import torch
    from m4depth_amd.export import FrameNamer
    one = FrameNamer(1)
    got = [one(torch.tensor([f]))[0] for f in (True, False, False, True, False)]
    assert got == ["s00_t0000/000000", "s00_t0000/000001", "s00_t0000/000002", "s00_t0001/000000", "s00_t0001/000001"]
    three = FrameNamer(3)
    assert three([True, True, True]) == ["s00_t0000/000000", "s01_t0000/000000", "s02_t0000/000000"]
    assert three(np.array([False, True, False])) == ["s00_t0000/000001", "s01_t0001/000000", "s02_t0000/000001"]
    assert three([False, False, True]) == ["s00_t0000/000002", "s01_t0001/000001", "s02_t0001/000000"]
    assert FrameNamer(2)([False, False]) == ["s00_t0000/000000", "s01_t0000/000000"]             # a stream joined mid-way
    with pytest.raises(ValueError):
        three([True])


def test_read_depth_png_round_trip(tmp_path):
    from PIL import Image
    from m4depth_amd.export import read_depth_png
    rng = np.random.default_rng(0)
    depth = rng.uniform(0.5, 200.0, (9, 13)).astype(F)
    kitti = np.rint(depth * F(256)).astype(np.uint16)
    kitti[0, 0] = 0
    midair = (F(512.0) / depth).astype(np.float16).view(np.uint16)
    midair[0, 0] = 0x7C00
    for fmt, bits in (("kitti16", kitti), ("midair16", midair)):
        path = str(tmp_path / (fmt + ".png"))
        Image.fromarray(bits).save(path, format="PNG", compress_level=1)
        got = read_depth_png(path, fmt)
        want = bits.astype(F) / F(256) if fmt == "kitti16" else F(512.0) / np.where(bits == 0x7C00, F(np.inf),
                                                                                     bits.view(np.float16).astype(F))
        assert got.dtype == np.float32 and got.shape == (9, 13) and got[0, 0] == 0
        assert np.array_equal(got.view(np.uint32), want.astype(F).view(np.uint32))
    assert np.abs(read_depth_png(str(tmp_path / "kitti16.png"), "kitti16")[1:] - depth[1:]).max() <= 1 / 512
    with pytest.raises(ValueError):
        read_depth_png(str(tmp_path / "kitti16.png"), "tartanair")


def _refused(argv, capsys, match):
    from m4depth_amd import main as MAIN
    with pytest.raises(SystemExit) as e:
        MAIN.main(argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def test_driver_refusals(tmp_path, capsys):
    out = str(tmp_path / "out")
    _refused(["--mode", "eval", "--save_dir", out], capsys, "--save_dir is a --mode=predict option")
    _refused(["--mode", "train", "--save_dir", out], capsys, "--save_dir is a --mode=predict option")
    _refused(["--mode", "predict", "--save_format", "midair16"], capsys, "--save_format needs --save_dir")
    _refused(["--mode", "predict", "--save_panels", "est"], capsys, "--save_panels needs --save_dir")
    _refused(["--mode", "predict", "--save_range", "1", "80"], capsys, "--save_range needs --save_dir")
    _refused(["--mode", "predict", "--save_err_max", "0.2"], capsys, "--save_err_max needs --save_dir")
    _refused(["--mode", "predict", "--save_dir", out, "--save_panels", "est,depth"], capsys, "--save_panels")
    _refused(["--mode", "predict", "--save_dir", out, "--save_panels", "est,est,est,est,est"], capsys, "--save_panels")
    _refused(["--mode", "predict", "--save_dir", out, "--save_format", "tartanair"], capsys, "invalid choice")
    _refused(["--mode", "predict", "--save_dir", out, "--save_range", "80", "1"], capsys, "--save_range")
    _refused(["--mode", "predict", "--save_dir", out, "--save_err_max", "0"], capsys, "--save_err_max")
    assert not os.path.exists(out)


def test_driver_refuses_ground_truth_panels_without_ground_truth(tmp_path, capsys):
    """Records whose csv files have no depth column (a capture without ground truth): gt / err panels cannot be drawn."""
    from m4depth_amd import main as MAIN
    rec = tmp_path / "records" / "set_0"
    rec.mkdir(parents=True)
    cols = ["id", "camera_l", "qw", "qx", "qy", "qz", "tx", "ty", "tz"]
    (rec / "traj_0000.csv").write_text("\t".join(cols) + "\n" + "\t".join(["0", "a.JPEG", "1", "0", "0", "0", "0", "0", "0"]) + "\n")
    base = ["--mode", "predict", "--dataset", "midair", "--records_path", str(tmp_path / "records"), "--save_dir",
            str(tmp_path / "out")]
    for panels in ("gt", "rgb,err"):
        _refused(base + ["--save_panels", panels], capsys, "no ground-truth map")
    parser = MAIN.build_parser()
    args = parser.parse_args(base + ["--save_panels", "rgb,est"])
    MAIN.check_save_args(parser, args)                                          # panels that need no ground truth pass
    assert args.save_panels == ("rgb", "est") and args.save_format == "kitti16" and args.save_range == (1.0, 80.0)
    (rec / "traj_0000.csv").write_text("\t".join(cols + ["disp"]) + "\n")
    args = parser.parse_args(base + ["--save_panels", "gt"])
    MAIN.check_save_args(parser, args)
